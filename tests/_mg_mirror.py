"""Numpy mirror of the aggregation multigrid preconditioner (module_a/multigrid.py), shared by tests/test_multigrid.py and
tests/test_gpu_multigrid.py, and the grid matrices those tests build.

Three parts, none of which uses the class's code:
  galerkin()            the coarse matrix as a plain loop over the stored entries in storage order (a dict keyed by (I, J));
  restrict() / prolong_add()   the transfer steps as strided slices of the level's box;
  vcycle() / apply()    V(l, r) composed from the oracle's SpMV (the kernels' one summation order) and _cheb_mirror.mirror, on the
                        level matrices and coefficients the object under test holds.
Every step is a separate rounding in the storage dtype."""
import numpy as np

from _cheb_mirror import mirror as cheb_mirror


def box(dims):
    d = tuple(int(v) for v in dims)
    return (1,) * (3 - len(d)) + d


def coarse(dims):
    return tuple((int(v) + 1) // 2 for v in dims)


def level_dims(grid):
    """dims of every level, down to the one with a single unknown."""
    out = [tuple(int(v) for v in grid)]
    while int(np.prod(out[-1])) > 1:
        out.append(coarse(out[-1]))
    return out


def aggregate(i, dims):
    n0, n1, n2 = box(dims)
    m0, m1, m2 = box(coarse(dims))
    i = np.asarray(i, dtype=np.int64)
    return ((i // (n1 * n2)) // 2 * m1 + (i // n2 % n1) // 2) * m2 + (i % n2) // 2


def galerkin(crow, col, val, dims):
    """(crow, col, val) of P^T A P: entry (I, J) = the stored entries with agg(row) = I, agg(col) = J added in storage order."""
    crow, col = np.asarray(crow, dtype=np.int64), np.asarray(col, dtype=np.int64)
    n = len(crow) - 1
    nc = int(np.prod(coarse(dims)))
    rows = np.repeat(np.arange(n), np.diff(crow))
    I, J = aggregate(rows, dims), aggregate(col, dims)
    acc = {}
    for k in range(len(col)):
        key = (int(I[k]), int(J[k]))
        acc[key] = acc[key] + val[k] if key in acc else val[k]
    keys = sorted(acc)
    out_val = np.array([acc[k] for k in keys], dtype=val.dtype)
    out_col = np.array([k[1] for k in keys], dtype=np.int64)
    out_crow = np.concatenate([[0], np.cumsum(np.bincount([k[0] for k in keys], minlength=nc))]).astype(np.int64)
    return out_crow, out_col, out_val


def restrict(t, dims):
    """rc[I] = sum of t over aggregate I in ascending fine index: the member (0, 0, 0) starts, the others that exist are added."""
    T = np.asarray(t).reshape(box(dims))
    rc = T[0::2, 0::2, 0::2].copy()
    for d0 in (0, 1):
        for d1 in (0, 1):
            for d2 in (0, 1):
                if (d0, d1, d2) == (0, 0, 0):
                    continue
                sub = T[d0::2, d1::2, d2::2]
                view = rc[:sub.shape[0], :sub.shape[1], :sub.shape[2]]
                view[...] = view + sub
    assert rc.dtype == T.dtype
    return rc.reshape(-1)


def prolong_add(z, e, omega, dims):
    """z + (omega * e[agg(i)]), omega rounded to the storage dtype once."""
    f = z.dtype.type
    n0, n1, n2 = box(dims)
    E = np.asarray(e).reshape(box(coarse(dims)))[np.ix_(np.arange(n0) // 2, np.arange(n1) // 2, np.arange(n2) // 2)]
    out = z + (f(omega) * E.reshape(-1))
    assert out.dtype == z.dtype
    return out


def _csr_np(lev):
    c = lev.csr.cpu()
    return c.crow_indices().numpy(), c.col_indices().numpy(), c.values().numpy()


def vcycle(oracle, M, l, r):
    """V(l, r) on the object's level matrices, with its smoother coefficients and omega."""
    lev = M.levels[l]
    f = r.dtype.type
    if lev.n == 1:
        return lev.dinv.cpu().numpy().astype(r.dtype) * r
    crow, col, val = _csr_np(lev)
    spmv = oracle.spmv if r.dtype == np.float64 else oracle.spmv32
    S = lambda v: cheb_mirror(oracle, crow, col, val, lev.smoother, v, dtype=f)
    z = S(r)
    t = spmv(crow, col, val, z, bsub=r)
    e = vcycle(oracle, M, l + 1, restrict(t, lev.dims))
    z = prolong_add(z, e, M.omega, lev.dims)
    t = spmv(crow, col, val, z, bsub=r)
    z = z + S(t)
    assert z.dtype == r.dtype
    return z


def apply(oracle, M, r, level=0, scale=None):
    """M(r): scale * V(level, r) when scale != 1 (scale: the object's unless given)."""
    r = np.ascontiguousarray(r)
    z = vcycle(oracle, M, level, r)
    s = M.scale if scale is None else scale
    return r.dtype.type(s) * z if s != 1.0 else z


# ----------------------------------------------------------------------------------------------------------- matrices on a grid
def grid_matrix(dims, radius=1, full_box=False, seed=None, dtype=np.float64):
    """A symmetric M-matrix on the grid `dims` (CSR, sorted rows): off-diagonal -w_ij for every neighbour pair -- the 2 d axis
    neighbours, or with `full_box` all points within `radius` in the maximum norm --, w = 1 or seeded in [0.5, 2); the diagonal is
    the number of stencil neighbours an interior point has (w = 1: the Dirichlet Laplacian) or the row's weights + 0.05."""
    d3 = box(dims)
    n = int(np.prod(d3))
    idx = np.arange(n).reshape(d3)
    rng = np.random.default_rng([77, n] if seed is None else [seed, n])
    offs = []
    rr = range(-radius, radius + 1)
    for o in ((a, b, c) for a in rr for b in rr for c in rr):
        if o <= (0, 0, 0) or any(abs(v) > 0 and d3[k] == 1 for k, v in enumerate(o)):
            continue
        if full_box or sum(v != 0 for v in o) == 1:
            offs.append(o)
    r_, c_, v_ = [], [], []
    for o in offs:
        src = tuple(slice(0, d3[k] - o[k]) if o[k] >= 0 else slice(-o[k], d3[k]) for k in range(3))
        dst = tuple(slice(o[k], d3[k]) if o[k] >= 0 else slice(0, d3[k] + o[k]) for k in range(3))
        i, j = idx[src].reshape(-1), idx[dst].reshape(-1)
        w = np.ones(i.size) if seed is None else rng.uniform(0.5, 2.0, i.size)
        r_ += [i, j]
        c_ += [j, i]
        v_ += [-w, -w]
    r_, c_, v_ = (np.concatenate(a) if a else np.zeros(0, dtype=t) for a, t in ((r_, np.int64), (c_, np.int64), (v_, np.float64)))
    diag = np.full(n, float(2 * len(offs))) if seed is None else np.bincount(r_, weights=-v_, minlength=n) + 0.05
    if n == 1 and not offs:
        diag = np.array([4.0])
    r_, c_, v_ = np.concatenate([r_, np.arange(n)]), np.concatenate([c_, np.arange(n)]), np.concatenate([v_, diag])
    order = np.lexsort((c_, r_))
    crow = np.concatenate([[0], np.cumsum(np.bincount(r_, minlength=n))]).astype(np.int64)
    return crow, c_[order].astype(np.int64), v_[order].astype(dtype)


def csr_tensor(crow, col, val, device="cpu"):
    import torch
    n = len(crow) - 1
    return torch.sparse_csr_tensor(torch.from_numpy(np.asarray(crow, dtype=np.int64)), torch.from_numpy(np.asarray(col, dtype=np.int64)),
                                   torch.from_numpy(np.ascontiguousarray(val)), size=(n, n)).to(device)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))
