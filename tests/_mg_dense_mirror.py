"""Mirror of the dense coarsest level of `AggregationMultigridPreconditioner.from_graph(coarse_rows=K)` (module_a/multigrid.py), shared
by tests/test_dense_coarse.py and tests/test_gpu_dense_coarse.py.  None of it uses the class's code:
  dense_matrix()      a level's matrix written out densely by a loop over the stored entries, entries of one (row, col) added in
                      stored order (the first one starts the sum);
  stored_inverse()    what `levels[-1].cinv` must hold: torch.linalg.inv of that matrix in fp64 on the CPU, rounded once to the
                      storage dtype, as the flat column-by-column array of the kernels (element (i, j) at j * ld + i, padding 0);
  inverse_of()        the (n, n) inverse an object stores, element [i, j], read back from that layout;
  segmented()         z = C r by the rounding spec: p_q = 0, p_q = p_q + (C[i, j] * r[j]) over the 64 columns of segment q ascending,
                      s = 0, s = s + p_q over q ascending -- numpy, one product and one sum per column, each a separate rounding;
  vcycle() / apply()  the V-cycle of tests/_mg_graph_mirror.py on the object's levels, with the dense last level.
The V-cycle WRAPS `_mg_graph_mirror.vcycle`: that function ends its recursion with `levels[-1].dinv.cpu().numpy().astype(dtype) * r`,
so it is handed a view of the object whose last level carries a `dinv` that answers this chain with the segmented product."""
import numpy as np
import torch

import _mg_graph_mirror as GM
from _mg_graph_mirror import bits, csr_tensor, same_bits  # noqa: F401  (re-exported for the tests)

SEGMENT = 64


def dense_matrix(crow, col, val):
    n = len(crow) - 1
    seen = {}
    for i in range(n):
        for k in range(int(crow[i]), int(crow[i + 1])):
            key = (i, int(col[k]))
            seen[key] = seen[key] + val[k] if key in seen else val[k]
    D = np.zeros((n, n), dtype=val.dtype)
    for (i, j), v in seen.items():
        D[i, j] = v
    return D


def padded(n):
    return (n + 3) & ~3


def stored_inverse(D, ld=None):
    """The flat array of n * ld elements for the dense matrix D of a level (ld: the class's (n + 3) & ~3 unless given)."""
    n = D.shape[0]
    ld = padded(n) if ld is None else ld
    inv = torch.linalg.inv(torch.from_numpy(D.astype(np.float64))).to(torch.from_numpy(D).dtype).numpy()
    out = np.zeros(n * ld, dtype=D.dtype)
    for j in range(n):
        out[j * ld:j * ld + n] = inv[:, j]
    return out


def inverse_of(lev):
    """C with C[i, j] = element (i, j) of the inverse the level stores."""
    n, ld = lev.n, lev.ld
    flat = lev.cinv.cpu().contiguous().reshape(-1).numpy()
    assert flat.size == n * ld
    return np.stack([flat[j * ld:j * ld + n] for j in range(n)], axis=1)


def segmented(C, r):
    n = len(r)
    assert C.shape == (n, n) and C.dtype == r.dtype
    s = np.zeros(n, dtype=r.dtype)
    for j0 in range(0, n, SEGMENT):
        p = np.zeros(n, dtype=r.dtype)
        for j in range(j0, min(j0 + SEGMENT, n)):
            p = p + (C[:, j] * r[j])
        s = s + p
    assert s.dtype == r.dtype
    return s


class _DenseAsDinv:
    """Stands where `_mg_graph_mirror.vcycle` reads the last level's `dinv`: `.cpu().numpy().astype(dtype) * r` is segmented(C, r)."""

    def __init__(self, C):
        self.C = C

    def cpu(self):
        return self

    def numpy(self):
        return self

    def astype(self, dtype):
        assert self.C.dtype == dtype
        return self

    def __mul__(self, r):
        return segmented(self.C, r)


class _View:
    """The attributes `_mg_graph_mirror.vcycle` reads of the object (`levels`, `omega`), the dense last level replaced."""

    class _Last:
        def __init__(self, C):
            self.n, self.dinv = C.shape[0], _DenseAsDinv(C)

    def __init__(self, M):
        self.omega = M.omega
        self.levels = list(M.levels[:-1]) + [self._Last(inverse_of(M.levels[-1]))] if M.dense else list(M.levels)


def vcycle(oracle, M, l, r):
    return GM.vcycle(oracle, _View(M), l, r)


def apply(oracle, M, r, scale=None):
    """M(r): scale * V(0, r) when scale != 1 (scale: the object's unless given)."""
    r = np.ascontiguousarray(r)
    z = vcycle(oracle, M, 0, r)
    s = M.scale if scale is None else scale
    return r.dtype.type(s) * z if s != 1.0 else z
