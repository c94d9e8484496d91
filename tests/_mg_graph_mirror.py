"""Mirror of `AggregationMultigridPreconditioner.from_graph` and `pairwise_aggregates` (module_a/multigrid.py) in plain Python and
numpy loops, shared by tests/test_graph_multigrid.py and tests/test_gpu_graph_multigrid.py, and the matrices those tests build.

None of it uses the class's code, and none of it computes the way the class does:
  galerkin_agg()          the coarse matrix as a loop over the stored entries in storage order (a dict keyed by (I, J));
  matching_pass()         the matching as the SEQUENTIAL greedy walk over the strong edges sorted by (hash, u n + v) -- the class runs
                          handshake rounds of scatter-minima; the two agree because every rank is distinct;
  pairwise_aggregates()   the passes, each on the Galerkin matrix of the composite aggregates so far;
  hierarchy()             the levels (crow, col, val, agg) down to the first one without a pair;
  restrict() / prolong_add()   the transfers as loops over member lists;
  vcycle() / apply()      V(l, r) composed from the oracle's SpMV (the kernels' one summation order) and _cheb_mirror.mirror, on the
                          level matrices, maps and coefficients the object under test holds.
Every floating-point step is a separate rounding in the storage dtype; the weights of the matching are fp64."""
import numpy as np

from _cheb_mirror import mirror as cheb_mirror
from _mg_mirror import bits, csr_tensor, same_bits  # noqa: F401  (re-exported for the tests)

MASK = 0x7FFFFFFF


def edge_hash(u, v):
    k = (u * 73856093 + v * 19349663) & MASK
    k = ((k ^ (k >> 15)) * 0x2C1B3C6D) & MASK
    k = ((k ^ (k >> 12)) * 0x297A2D39) & MASK
    return k ^ (k >> 15)


def galerkin_agg(crow, col, val, agg, nc):
    """(crow, col, val) of P^T A P: entry (I, J) = the stored entries with agg[row] = I, agg[col] = J added in storage order; rows
    sorted by column, stored zeros kept."""
    n = len(crow) - 1
    acc = {}
    for i in range(n):
        for k in range(int(crow[i]), int(crow[i + 1])):
            key = (int(agg[i]), int(agg[col[k]]))
            acc[key] = acc[key] + val[k] if key in acc else val[k]
    keys = sorted(acc)
    out_val = np.array([acc[k] for k in keys], dtype=val.dtype)
    out_col = np.array([k[1] for k in keys], dtype=np.int64)
    out_crow = np.concatenate([[0], np.cumsum(np.bincount(np.array([k[0] for k in keys], dtype=np.int64), minlength=nc))]).astype(np.int64)
    return out_crow, out_col, out_val


def matching_pass(crow, col, val, theta):
    """(agg, nc) of one pass on a COALESCED matrix: the greedy matching over the strong edges in rank order."""
    n = len(crow) - 1
    w = {}
    for i in range(n):
        for k in range(int(crow[i]), int(crow[i + 1])):
            j = int(col[k])
            if j != i:
                e = (min(i, j), max(i, j))
                w[e] = max(w.get(e, 0.0), abs(float(val[k])))
    m = [0.0] * n
    for (u, v), we in w.items():
        m[u], m[v] = max(m[u], we), max(m[v], we)
    strong = [(edge_hash(u, v), u * n + v, u, v) for (u, v), we in w.items() if we > 0.0 and we >= theta * min(m[u], m[v])]
    partner = list(range(n))
    for _, _, u, v in sorted(strong):
        if partner[u] == u and partner[v] == v:
            partner[u], partner[v] = v, u
    agg, nc = np.empty(n, dtype=np.int64), 0
    for i in range(n):                       # ascending: an aggregate is numbered when its smallest member is met
        if partner[i] < i:
            agg[i] = agg[partner[i]]
        else:
            agg[i], nc = nc, nc + 1
    return agg, nc


def pairwise_aggregates(crow, col, val, passes=2, theta=0.25):
    n = len(crow) - 1
    agg, nc = np.arange(n, dtype=np.int64), n
    for _ in range(passes):
        step, nc_next = matching_pass(*galerkin_agg(crow, col, val, agg, nc), theta)
        if nc_next == nc:
            break
        agg, nc = step[agg], nc_next
    return agg, nc


def hierarchy(crow, col, val, passes=2, theta=0.25):
    """[(crow, col, val, agg or None)] per level; the last level is the first one whose aggregates are all single rows."""
    out = []
    while True:
        n = len(crow) - 1
        agg, nc = pairwise_aggregates(crow, col, val, passes, theta)
        if nc == n:
            out.append((crow, col, val, None))
            return out
        out.append((crow, col, val, agg))
        crow, col, val = galerkin_agg(crow, col, val, agg, nc)


def member_lists(agg, nc):
    mem = [[] for _ in range(nc)]
    for i, a in enumerate(agg):
        mem[int(a)].append(i)                # ascending fine index
    return mem


def csr_members(agg, nc):
    """(aptr, amem) int32 of the kernels' interface."""
    mem = member_lists(agg, nc)
    aptr = np.concatenate([[0], np.cumsum([len(m) for m in mem])]).astype(np.int32)
    return aptr, np.array([i for m in mem for i in m], dtype=np.int32)


def restrict(t, mem):
    """rc[I] = t[first member], then + t[member] over the others, left to right."""
    rc = np.empty(len(mem), dtype=t.dtype)
    for I, m in enumerate(mem):
        s = t[m[0]]
        for i in m[1:]:
            s = s + t[i]
        rc[I] = s
    return rc


def prolong_add(z, e, omega, agg):
    """z + (omega * e[agg[i]]), omega rounded to the storage dtype once."""
    f = z.dtype.type
    out = np.empty_like(z)
    w = f(omega)
    for i in range(len(z)):
        out[i] = z[i] + (w * e[agg[i]])
    return out


def restrict_np(t, aptr, amem):
    """restrict() for vectors too long for a Python loop: the k-th member of every aggregate that has one is added in pass k, one
    numpy addition per element, so the same left-to-right sums (checked against restrict() on the small cases)."""
    aptr, amem = np.asarray(aptr, dtype=np.int64), np.asarray(amem, dtype=np.int64)
    start, sizes = aptr[:-1], np.diff(aptr)
    rc = t[amem[start]]
    for k in range(1, int(sizes.max())):
        has = np.flatnonzero(sizes > k)
        rc[has] = rc[has] + t[amem[start[has] + k]]
    assert rc.dtype == t.dtype
    return rc


def prolong_add_np(z, e, omega, agg):
    out = z + (z.dtype.type(omega) * e[np.asarray(agg, dtype=np.int64)])
    assert out.dtype == z.dtype
    return out


def synthetic_aggregates(n, nc, spread, seed=0):
    """(agg, aptr, amem) int32 for n rows in nc aggregates of 1 .. 9 members, sizes mixed by a seeded draw (n <= 9 nc).  `spread`
    False: an aggregate's members are adjacent rows; True: member k of every aggregate lies behind member k - 1 of ALL aggregates,
    so the members of one aggregate are about nc rows apart."""
    assert nc <= n <= 9 * nc
    rng = np.random.default_rng([seed, n, nc])
    sizes = 1 + rng.binomial(8, (n / nc - 1.0) / 8.0, nc).astype(np.int64)
    fixed = 9 if nc >= 100 else 0                                 # every size 1 .. 9 occurs
    sizes[:fixed] = rng.permutation(9)[:fixed] + 1
    while sizes.sum() != n:                                       # the draw misses n by a few: single steps on seeded aggregates
        d = n - int(sizes.sum())
        room = fixed + np.flatnonzero(sizes[fixed:] < 9 if d > 0 else sizes[fixed:] > 1)
        sizes[rng.choice(room, min(abs(d), len(room)), replace=False)] += 1 if d > 0 else -1
    aptr = np.concatenate([[0], np.cumsum(sizes)])
    owner = np.repeat(np.arange(nc), sizes)                       # the aggregate of every slot of amem
    if spread:
        rank = np.arange(n) - aptr[:-1][owner]                    # which member of its aggregate a slot is
        amem = np.empty(n, dtype=np.int64)
        amem[np.lexsort((owner, rank))] = np.arange(n)
    else:
        amem = np.arange(n)
    agg = np.empty(n, dtype=np.int64)
    agg[amem] = owner
    return agg.astype(np.int32), aptr.astype(np.int32), amem.astype(np.int32)


def _csr_np(lev):
    c = lev.csr.cpu()
    return c.crow_indices().numpy(), c.col_indices().numpy(), c.values().numpy()


def vcycle(oracle, M, l, r):
    lev = M.levels[l]
    f = r.dtype.type
    if l == len(M.levels) - 1:
        return lev.dinv.cpu().numpy().astype(r.dtype) * r
    crow, col, val = _csr_np(lev)
    agg = lev.agg.cpu().numpy()
    spmv = oracle.spmv if r.dtype == np.float64 else oracle.spmv32
    S = lambda v: cheb_mirror(oracle, crow, col, val, lev.smoother, v, dtype=f)
    z = S(r)
    t = spmv(crow, col, val, z, bsub=r)
    e = vcycle(oracle, M, l + 1, restrict(t, member_lists(agg, M.levels[l + 1].n)))
    z = prolong_add(z, e, M.omega, agg)
    t = spmv(crow, col, val, z, bsub=r)
    z = z + S(t)
    assert z.dtype == r.dtype
    return z


def apply(oracle, M, r, scale=None):
    """M(r): scale * V(0, r) when scale != 1 (scale: the object's unless given)."""
    r = np.ascontiguousarray(r)
    z = vcycle(oracle, M, 0, r)
    s = M.scale if scale is None else scale
    return r.dtype.type(s) * z if s != 1.0 else z


# --------------------------------------------------------------------------------------------------------------------- matrices
def stencil5(nx, ny, west=-1.0, east=-1.0, south=-1.0, north=-1.0, diag=None, dtype=np.float64):
    """5-point matrix on an nx x ny grid, row i ny + j, Dirichlet truncation; (i, j-1) is west, (i-1, j) south.  A coefficient of
    None is NOT STORED (a one-sided entry); `diag` defaults to minus the sum of the four."""
    d = -sum(c for c in (west, east, south, north) if c is not None) if diag is None else diag
    crow, col, val = [0], [], []
    for i in range(nx):
        for j in range(ny):
            for c, (a, b) in ((south, (i - 1, j)), (west, (i, j - 1)), (d, (i, j)), (east, (i, j + 1)), (north, (i + 1, j))):
                if c is not None and 0 <= a < nx and 0 <= b < ny:
                    col.append(a * ny + b)
                    val.append(c)
            crow.append(len(col))
    return np.array(crow, dtype=np.int64), np.array(col, dtype=np.int64), np.array(val, dtype=dtype)


def anisotropic(nx, ny, eps, dtype=np.float64):
    """The 5-point Laplacian with the coupling along the fast index (j, the y of row i ny + j) scaled by eps."""
    return stencil5(nx, ny, west=-eps, east=-eps, dtype=dtype)


def one_sided(nx, ny, dtype=np.float64):
    """Convection-diffusion: diffusion 1 along i in both directions, pure upwind convection along j -- the upstream entry -2 is
    stored, the downstream one is not, so the edges along j have one direction only.  Diagonal 4.1: strictly dominant."""
    return stencil5(nx, ny, west=-2.0, east=None, diag=4.1, dtype=dtype)


def shuffled(crow, col, val, seed=1):
    """P A P^T for a seeded permutation: rows and columns renumbered alike, every row's entries kept in their stored order."""
    n = len(crow) - 1
    new_of = np.random.default_rng(seed).permutation(n)          # old row i becomes row new_of[i]
    old_of = np.argsort(new_of)
    lens = np.diff(crow)[old_of]
    out_crow = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    idx = np.concatenate([np.arange(crow[i], crow[i + 1]) for i in old_of]) if n else np.zeros(0, dtype=np.int64)
    return out_crow, new_of[col[idx]].astype(np.int64), np.ascontiguousarray(val[idx])


def block_diagonal(*mats):
    crow, col, val, off = [np.zeros(1, dtype=np.int64)], [], [], 0
    for c, j, v in mats:
        crow.append(c[1:] + crow[-1][-1])
        col.append(j + off)
        val.append(v)
        off += len(c) - 1
    return np.concatenate(crow), np.concatenate(col), np.concatenate(val)


def star(leaves, dtype=np.float64):
    """A centre (row 0) coupled to `leaves` leaves by -1: pairwise matching removes one pair per pass."""
    n = leaves + 1
    crow = np.concatenate([[0, n], n + 2 * np.arange(1, n)]).astype(np.int64)
    col = np.concatenate([np.arange(n), np.stack([np.zeros(leaves, dtype=np.int64), np.arange(1, n)], 1).reshape(-1)])
    val = np.concatenate([[float(leaves) + 1.0], -np.ones(leaves), np.tile([-1.0, 2.0], leaves)])
    return crow, col.astype(np.int64), val.astype(dtype)
