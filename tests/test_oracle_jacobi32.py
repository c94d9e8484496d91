"""The fp32-storage Jacobi wrappers of the oracle (bicgstab_jacobi32, gmres_jacobi32) against their fp64 forms on a small
Jacobi-preconditioned nonsymmetric system (no GPU needed): same verdict, and an x within fp32 reach of the fp64 one."""
import numpy as np
import pytest
import scipy.sparse as sp


def _convdiff_varcoef(nx, seed=0):
    """5-point upwind convection-diffusion on an nx x nx grid with a diagonal that varies by a factor ~4 (so that Jacobi
    scaling is not a uniform multiple of the identity); b = A x_true."""
    rng = np.random.default_rng(seed)
    n = nx * nx
    I = sp.identity(nx, format="csr")
    D = sp.diags([-1.3, 2.6, -1.3], [-1, 0, 1], shape=(nx, nx))       # diffusion + upwind convection in x
    E = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(nx, nx))
    A = (sp.kron(I, D) + sp.kron(E, I)).tocsr()
    A = (A + sp.diags(rng.uniform(0.0, 12.0, n))).tocsr()
    A.sort_indices()
    x_true = rng.standard_normal(n)
    return A, A @ x_true


@pytest.mark.parametrize("solver", ["bicgstab_jacobi", "gmres_jacobi"])
def test_fp32_jacobi_wrapper_agrees_with_fp64(oracle, solver):
    A, b = _convdiff_varcoef(24)
    dinv = 1.0 / A.diagonal()
    kw = dict(tol=1e-5, maxiter=400)
    if solver == "gmres_jacobi":
        kw["restart"] = 20
    r64 = getattr(oracle, solver)(A.indptr, A.indices, A.data, dinv, b, **kw)
    r32 = getattr(oracle, solver + "32")(A.indptr, A.indices, A.data.astype(np.float32), dinv.astype(np.float32),
                                        b.astype(np.float32), **kw)
    assert r64.info == 0 and r32.info == r64.info, (r64.info, r32.info)
    assert r32.x.dtype == np.float32 and r32.x.shape == b.shape
    # both stop at a relative residual of about tol = 1e-5; with cond(A) of a few tens their solutions agree to about 1e-4
    rel = np.linalg.norm(r32.x.astype(np.float64) - r64.x) / np.linalg.norm(r64.x)
    assert rel < 1e-3, rel
    # and the fp32 solve's own stats describe a converged run
    assert r32.residual_norm <= r32.threshold and r32.iterations >= 1
