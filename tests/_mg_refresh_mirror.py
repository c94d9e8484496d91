"""Mirror of what `AggregationMultigridPreconditioner.update` recomputes per level (module_a/multigrid.py, include/hipk.h
"the refresh of a hierarchy"), shared by tests/test_mg_refresh.py and tests/test_gpu_mg_refresh.py, and the matrices of those tests.
None of it uses the class's code:
  level_scan()     hipk_mg_level_scan as scalar loops: per row d = 0, d = d + a over the stored diagonal entries and s = 0,
                   s = s + |a| over all entries, both in stored order in the storage dtype; dinv = 1 / d; the maximum of
                   (double)s / (double)d with a NaN winning as in torch.max; the number of rows with d <= 0;
  t_family()       the face-coefficient 5-point operator of the iteration tests: k = exp((4 - 6 t) x + 3 sin(6 y + 5 t)) at the
                   cell faces of an n x n grid of the unit square, Dirichlet boundaries;
  same_pattern()   the transforms of tests/_order_cases.py applied to two matrices of one pattern give one pattern."""
import numpy as np


def level_scan(crow, col, val, want_lmax=True):
    """(dinv, lmax, bad) of one level; lmax is 0.0 when `want_lmax` is False."""
    n = len(crow) - 1
    f = val.dtype.type
    crow_l, col_l = [int(v) for v in crow], [int(v) for v in col]
    dinv = np.empty(n, dtype=val.dtype)
    lmax, nan, bad = -np.inf, False, 0
    with np.errstate(all="ignore"):
        for i in range(n):
            d, s = f(0), f(0)
            for k in range(crow_l[i], crow_l[i + 1]):
                a = val[k]
                if col_l[k] == i:
                    d = f(d + a)
                s = f(s + f(abs(a)))
            dinv[i] = f(1) / d
            if d <= 0:
                bad += 1
            q = np.float64(s) / np.float64(d)
            if q != q:
                nan = True
            elif q > lmax:
                lmax = float(q)
    if not want_lmax:
        return dinv, 0.0, float(bad)
    return dinv, (float("nan") if nan else lmax), float(bad)


def t_family(n, t, dtype=np.float64):
    """(crow, col, val): cell (i, j), row i n + j, has its centre at x = (i + 1/2) / n, y = (j + 1/2) / n; the face between two
    cells carries k at its midpoint, -k off the diagonal of both rows and +k on both diagonals; a boundary face adds its k to the
    diagonal alone (Dirichlet).  Sorted rows, the same pattern for every t."""
    h = 1.0 / n
    k = lambda x, y: np.exp((4.0 - 6.0 * t) * x + 3.0 * np.sin(6.0 * y + 5.0 * t))
    c = (np.arange(n) + 0.5) * h                      # cell centres
    e = np.arange(n + 1) * h                          # face positions
    kx = k(e[:, None], c[None, :])                    # kx[i, j]: the face between cells (i - 1, j) and (i, j)
    ky = k(c[:, None], e[None, :])                    # ky[i, j]: the face between cells (i, j - 1) and (i, j)
    crow, col, val = [0], [], []
    for i in range(n):
        for j in range(n):
            d = kx[i, j] + kx[i + 1, j] + ky[i, j] + ky[i, j + 1]
            for a, b, w in ((i - 1, j, -kx[i, j]), (i, j - 1, -ky[i, j]), (i, j, d), (i, j + 1, -ky[i, j + 1]), (i + 1, j, -kx[i + 1, j])):
                if 0 <= a < n and 0 <= b < n:
                    col.append(a * n + b)
                    val.append(w)
            crow.append(len(col))
    return np.array(crow, dtype=np.int64), np.array(col, dtype=np.int64), np.array(val, dtype=dtype)


def same_pattern(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
