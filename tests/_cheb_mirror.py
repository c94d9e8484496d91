"""Numpy mirror of the Chebyshev preconditioner's apply (module_a/preconditioners.py: ChebyshevPreconditioner), shared by
tests/test_chebyshev.py and tests/test_gpu_chebyshev.py: the oracle's SpMV for the row sums (the kernels' one summation order), numpy
element-wise steps in the documented order, every step a separate rounding."""
import json
import math
import os

import numpy as np
import torch

from conftest import GOLDEN


def runs():
    with open(os.path.join(GOLDEN, "cheb_index.json")) as f:
        return json.load(f)["runs"]


def rid(r):
    return f"{r['case']}-{r['tag']}"


def csr(d, device="cpu", dtype=torch.float64):
    n = int(d["n"])
    return torch.sparse_csr_tensor(torch.from_numpy(d["crow"]).long(), torch.from_numpy(d["col"]).long(),
                                   torch.from_numpy(d["val"]).to(dtype), size=(n, n)).to(device)


def coefficients(lmax, lmin, m):
    """c0, c1[1..m], c2[1..m] of the issue's recurrence, in Python floats."""
    theta, delta = (lmax + lmin) / 2, (lmax - lmin) / 2
    sigma = theta / delta
    rho = 1 / sigma
    c0, c1, c2 = 1 / theta, [], []
    for _ in range(m):
        rho_k = 1 / (2 * sigma - rho)
        c1.append(rho_k * rho)
        c2.append(2 * rho_k / delta)
        rho = rho_k
    return c0, c1, c2


def scale_of(lmax, lmin, m, dinv_max):
    c0, c1, c2 = coefficients(lmax, lmin, m)
    d = z = c0                                   # p_m(0): the recurrence on a = 0, dinv = 1, r = 1
    for k in range(m):
        d = c1[k] * d + c2[k]
        z = z + d
    sigma = ((lmax + lmin) / 2) / ((lmax - lmin) / 2)
    return 1 / (max(z, (1 + 1 / math.cosh(m * math.acosh(sigma))) / lmin) * dinv_max)


def mirror(oracle, crow, col, val, M, r, dtype=np.float64):
    """M(r) for the preconditioner object's coefficients, in `dtype` arithmetic."""
    f = dtype
    spmv = oracle.spmv if dtype == np.float64 else oracle.spmv32
    val, r, dinv = np.asarray(val, dtype=f), np.asarray(r, dtype=f), M.dinv.cpu().numpy().astype(f)
    d = f(M.c0) * (dinv * r)
    z = d
    for k in range(M.degree):
        res = dinv * spmv(crow, col, val, z, bsub=r)         # r - A z, then the row scaling
        d = (f(M.c1[k]) * d) + (f(M.c2[k]) * res)
        z = z + d
    if M.scale != 1.0:
        z = f(M.scale) * z
    assert z.dtype == f
    return z
