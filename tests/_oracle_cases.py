"""Shared by the case-table modules that pin solver loops to the CPU oracle (test_gpu_mid_oracle.py, _form_cases.py and
test_gpu_solver_forms.py): the seeded scipy matrix builders and the long-double check of the returned stats."""
import numpy as np
import scipy.sparse as sp


def _band(n, offs, match=0, sym=True, seed=0):
    """Rows with entries at column offsets +-o (o in offs, clipped at the edges) and, when match > 0, one more at the row's
    partner in a perfect matching at distance `match` (a symmetric pattern with an even entry count per row).  Off-diagonal
    values in [-1, -0.1] (symmetric or independent), diagonal = row's off-diagonal absolute sum + 0.5: SPD when symmetric,
    strictly diagonally dominant either way."""
    rng = np.random.default_rng(seed)
    rows, cols = [], []
    for o in offs:
        i = np.arange(n - o)
        rows += [i, i + o]
        cols += [i + o, i]
    if match:
        i = np.arange(n)
        p = np.where((i // match) % 2 == 0, i + match, i - match)
        keep = (p < n) & (i < p)
        rows += [i[keep], p[keep]]
        cols += [p[keep], i[keep]]
    r, c = np.concatenate(rows), np.concatenate(cols)
    v = rng.uniform(-1.0, -0.1, r.size)
    M = sp.csr_matrix((v, (r, c)), shape=(n, n))
    if sym:
        U = sp.triu(M, 1)
        M = U + U.T
    d = np.asarray(abs(M).sum(axis=1)).ravel() + 0.5
    M = (M + sp.diags(d)).tocsr()
    M.sort_indices()
    return M


def _signed_band(n, offs, seed=0):
    """Nonsymmetric: entries at the signed offsets `offs` only, diagonally dominant."""
    rng = np.random.default_rng(seed)
    M = sp.diags([rng.uniform(-1.0, -0.1, n - abs(o)) for o in offs], list(offs), shape=(n, n))
    M = (M + sp.diags(np.asarray(abs(M).sum(axis=1)).ravel() + 0.5)).tocsr()
    M.sort_indices()
    return M


def _ldc(nx):
    """Pressure matrix of the lid-driven-cavity caller (singular Neumann Laplacian; boundary rows of 3 and 4 entries)."""
    from pytorch_sparse_solver.utils.matrix_utils import create_ldc_pressure_csr
    A = create_ldc_pressure_csr(nx)
    M = sp.csr_matrix((A.values().numpy(), A.col_indices().numpy(), A.crow_indices().numpy()), shape=A.shape)
    M.sort_indices()
    return M


def _row_sums(a, indptr):
    """Per row the sum of its entries of `a`, 0 for a row without stored entries (np.add.reduceat alone gives a[indptr[i]] there)."""
    out = np.zeros(len(indptr) - 1, dtype=a.dtype)
    ne = np.flatnonzero(np.diff(indptr) > 0)
    if ne.size:
        out[ne] = np.add.reduceat(a, indptr[:-1][ne])
    return out


def _check_stats_long_double(solver, dt, M, dinv, b, x, st, kw):
    """The returned stats against long-double arithmetic on the stored A, b, (dinv) and the returned x.

    Bound used (u: unit roundoff of the storage dtype, W: longest row, n: rows): the library forms r = b - A x (times dinv for
    the Jacobi forms) row by row from W products, rounds it to storage and sums the squares in fp64, so
        | st.residual_norm - ||r|| |  <=  gamma * || |d| (|b| + |A| |x|) ||_2  +  n u ||r||,   gamma = (W + 2) u,
    with d = dinv (1 without M).  Norms of stored vectors (||x||, ||b||) are fp64 sums of exact squares:
    relative error <= gamma_n + u64, gamma_n = n u64 / (1 - n u64)."""
    n = M.shape[0]
    u = float(np.finfo(dt).eps) / 2
    u64 = float(np.finfo(np.float64).eps) / 2
    gn = n * u64 / (1 - n * u64) + u64
    W = int(np.diff(M.indptr).max())
    ld = np.longdouble
    xl, bl, vl = x.astype(ld), b.astype(ld), M.data.astype(ld)
    dl = np.ones(n, dtype=ld) if dinv is None else dinv.astype(ld)
    Ax = _row_sums(vl * xl[M.indices], M.indptr)
    aAx = _row_sums(np.abs(vl) * np.abs(xl[M.indices]), M.indptr)
    b_norm = np.sqrt(np.sum(bl * bl))
    assert abs(st.b_norm - b_norm) <= gn * b_norm, (st.b_norm, b_norm)
    tolf = float(np.float32(kw["tol"]))
    if solver in ("gmres", "pgmres"):   # TSL:735-753, 769 (gpu tolerances)
        cand = 1e-12 * np.sqrt(float(n))
        adaptive = cand if cand > kw["tol"] else tolf
        base_atol = float(np.float32(np.finfo(np.float64).eps * 1000 * float(n)))
        thr = 10 * max(adaptive * b_norm, base_atol)
        assert abs(st.threshold - thr) <= (gn + 2 * u64) * thr, (st.threshold, thr)
    else:                               # TSL:1010-1011
        thr = tolf * b_norm
        assert abs(st.threshold - thr) <= (gn + u64) * thr, (st.threshold, thr)
    if np.isnan(x).any():
        assert st.info == -1
        return
    x_norm = np.sqrt(np.sum(xl * xl))
    assert abs(st.x_norm - x_norm) <= gn * x_norm, (st.x_norm, x_norm)
    r = dl * (bl - Ax)
    r_norm = np.sqrt(np.sum(r * r))
    scale = np.sqrt(np.sum((np.abs(dl) * (np.abs(bl) + aAx)) ** 2))
    slack = (W + 2) * u * scale + n * u * r_norm
    assert abs(st.residual_norm - r_norm) <= slack, (st.residual_norm, float(r_norm), float(slack))
    if st.info == 0:
        assert r_norm <= st.threshold + slack, (float(r_norm), st.threshold)
    else:
        assert st.info == -1 and r_norm > st.threshold - slack, (st.info, float(r_norm), st.threshold)
