"""Aggregation multigrid on a structured grid, as a preconditioner for the `M` argument of cg / bicgstab / gmres.

`AggregationMultigridPreconditioner(A, grid)` is one V-cycle of plain (unsmoothed) aggregation: 2 x 2 (x 2) boxes of grid points
are the aggregates, the coarse matrices are the Galerkin products with the piecewise-constant prolongation, the smoother of every
level is the Chebyshev polynomial of `ChebyshevPreconditioner`, and the coarse correction is over-weighted by `omega`.  Its
iteration count grows only slowly with the grid, where the polynomial and Jacobi preconditioners follow sqrt(cond(A)).

`AggregationMultigridPreconditioner.from_graph(A)` is the same object for a matrix without a known grid: the aggregates are
`pairwise_aggregates` of the matrix graph (pairwise matching on strong couplings), everything else is unchanged.

Like `ChebyshevPreconditioner` the apply consists of SpMVs and element-wise steps only -- no dot product, no atomics -- so it is
deterministic, independent of launch shapes and bitwise equal to a CPU mirror of the steps (tests/_mg_mirror.py).
"""
import math
import numbers

import torch

from .preconditioners import ChebyshevPreconditioner, _diagonal

__all__ = ["AggregationMultigridPreconditioner", "MG_TAIL_MAX_ROWS", "MG_GRAPH_MAX_LEVELS", "MG_DENSE_MAX_ROWS", "MG_DENSE_TAIL_ROWS",
           "MG_W_MAX_LEVELS", "pairwise_aggregates"]

# The default of `tail_rows`: levels of at most this many unknowns run inside the one-launch tail kernel (0: none do).
# Measured (tools/mg_probe.py, profiles/mg_probe.txt, MI355X, fp64, 5-point Poisson 2000 x 2000, degree 1, device time per apply):
# tail_rows 0: 877.3 us (100 launches), 256: 563.1 us (64), 1024: 532.0 us (55), 4096: 620.3 us (46).  One workgroup walks the
# levels of up to 1024 rows faster than their launches do, but not the 3969-row one: 1024 had the least time, as it had in the two
# earlier runs of the probe (656.1 and 774.8 us, before the transfer kernels took the chunk form).  Variable diffusion 2000 x 2000
# and 7-point 128^3 agree; at 1000 x 1000 4096 is ahead (364.4 against 398.9 us), at 4000 x 4000 256 and 1024 tie.
# Graph hierarchies (`from_graph`) take the same default: their sweep at 2000 x 2000 decides nothing (profiles/mg_graph_probe.txt: a
# small level has a row of 38 entries, so no tail runs at any value, 2852 - 2889 us); at 1000 x 1000 256 / 1024 / 4096 gave 807.0 /
# 802.2 / 860.3 us, on an anisotropic 2000 x 2000 operator 960.1 / 995.7 / 1063.2 us.
MG_TAIL_MAX_ROWS = 1024

# `from_graph`: a hierarchy of more levels than this is refused as a stalled coarsening (pairwise matching shrinks a level by a
# factor of about 3.2 with two passes: 48 levels are far beyond any matrix that fits a device)
MG_GRAPH_MAX_LEVELS = 48

# `from_graph(coarse_rows=K)`: the largest dense coarsest level (`hipk_mg_dense_apply`'s envelope; its fp64 inverse is 32 MB), and
# the largest one the one-launch tail takes as its last level (`hipk_mg_gtail_dense_apply`'s: one workgroup streams the inverse)
MG_DENSE_MAX_ROWS = 2048
MG_DENSE_TAIL_ROWS = 512
DENSE_SEGMENT = 64        # the columns of one partial sum of the dense step

# `cycle="W"`: a hierarchy of more levels than this is refused.  Level l is visited 2^l times, as launches wherever the one-launch
# tail does not take the level (`_hipk.MG_TAIL_W_MAX_LEVELS`, 12): at 16 levels the last one is visited 2^14 times per apply, and
# `from_graph` without `coarse_rows` builds 33 - 39 levels on 1000^2 ... 4000^2 grids, where an apply would never end
MG_W_MAX_LEVELS = 16


def _grid3(dims):
    d = tuple(int(v) for v in dims)
    return (1,) * (3 - len(d)) + d


def _coarse_dims(dims):
    return tuple((int(v) + 1) // 2 for v in dims)


def _aggregate_of(idx: torch.Tensor, dims) -> torch.Tensor:
    """Coarse row of the fine rows `idx` (int64) of a grid `dims`: (i0 // 2, i1 // 2, i2 // 2) of (i0, i1, i2)."""
    n0, n1, n2 = _grid3(dims)
    m0, m1, m2 = _grid3(_coarse_dims(dims))
    i2 = idx % n2
    q = torch.div(idx, n2, rounding_mode="floor")
    i1 = q % n1
    i0 = torch.div(q, n1, rounding_mode="floor")
    h = lambda v: torch.div(v, 2, rounding_mode="floor")
    return (h(i0) * m1 + h(i1)) * m2 + h(i2)


def _rows_of(crow: torch.Tensor) -> torch.Tensor:
    n = crow.numel() - 1
    return torch.repeat_interleave(torch.arange(n, device=crow.device), crow[1:] - crow[:-1])


def _galerkin(crow: torch.Tensor, col: torch.Tensor, val: torch.Tensor, dims):
    """CSR arrays of P^T A P for the piecewise-constant P of the grid's aggregates.  Entry (I, J) is the sum of the stored entries of
    A with agg(row) = I and agg(col) = J in the order they are stored in A (s = first; s = s + next, in the storage dtype); rows
    sorted by column, stored zeros kept.  Torch ops without repeated scatter targets: the same bits on CPU and device, run to run."""
    crow, col = crow.to(torch.int64), col.to(torch.int64)
    nc = math.prod(_coarse_dims(dims))
    return _galerkin_keys(_aggregate_of(_rows_of(crow), dims) * nc + _aggregate_of(col, dims), val, nc)


def _galerkin_agg(crow: torch.Tensor, col: torch.Tensor, val: torch.Tensor, agg: torch.Tensor, nc: int):
    """`_galerkin` for aggregates given as an index array: `agg` (int64, one entry per row) maps a row to its aggregate in
    [0, nc).  The same rule and the same bits: entry (I, J) is s = first, s = s + next over A's storage order."""
    crow, col = crow.to(torch.int64), col.to(torch.int64)
    return _galerkin_keys(agg[_rows_of(crow)] * nc + agg[col], val, int(nc))


def _galerkin_keys(key: torch.Tensor, val: torch.Tensor, nc: int):
    """The sum of `_galerkin` over the stored entries keyed I * nc + J."""
    order, start, counts, ukey = _galerkin_order(key)
    s = _segment_sums(val[order], start, counts, int(counts.max()) if counts.numel() else 0)
    I = torch.div(ukey, nc, rounding_mode="floor")
    crow_c = torch.zeros(nc + 1, dtype=torch.int64, device=val.device)
    crow_c[1:] = torch.cumsum(torch.bincount(I, minlength=nc), 0)
    return crow_c, ukey % nc, s


def _galerkin_order(key: torch.Tensor):
    """What the sum over keyed entries needs beside the values: (`order`, the stable sort of the keys -- a segment keeps A's
    storage order --, the start and the length of every segment of equal keys in it, the segments' keys ascending)."""
    skey, order = torch.sort(key, stable=True)
    ukey, counts = torch.unique_consecutive(skey, return_counts=True)
    return order, torch.cumsum(counts, 0) - counts, counts, ukey


def _segment_sums(v: torch.Tensor, start: torch.Tensor, counts: torch.Tensor, longest: int) -> torch.Tensor:
    """s = v[start], s = s + v[start + k] for k = 1 .. counts - 1: one pass per rank within a segment, `longest` = max(counts)."""
    s = v[start]
    for k in range(1, longest):
        has = counts > k
        s = torch.where(has, s + v[torch.where(has, start + k, start)], s)
    return s


def _abs_row_sums(crow: torch.Tensor, val: torch.Tensor) -> torch.Tensor:
    """sum_j |a_ij| with each row summed left to right in stored order, whatever the device (the bits of the sequential CPU sum
    `ChebyshevPreconditioner` takes its Gershgorin bound from)."""
    crow = crow.to(torch.int64)
    n = crow.numel() - 1
    lens = crow[1:] - crow[:-1]
    K = int(lens.max()) if n and val.numel() else 0
    if K > 64:        # long rows (a dense matrix as CSR): the sequential CPU sum
        rows = _rows_of(crow.cpu())
        return torch.zeros(n, dtype=val.dtype).index_add_(0, rows, val.abs().cpu()).to(val.device)
    s = torch.zeros(n, dtype=val.dtype, device=val.device)
    av = val.abs()
    for k in range(K):
        has = lens > k
        s = torch.where(has, s + av[torch.where(has, crow[:-1] + k, 0)], s)
    return s


def _edge_hash(u: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """h(u, v) of `pairwise_aggregates`: non-negative int64 throughout, no product overflows for u, v < 2^31."""
    k = (u * 73856093 + v * 19349663) & 0x7FFFFFFF
    k = ((k ^ (k >> 15)) * 0x2C1B3C6D) & 0x7FFFFFFF
    k = ((k ^ (k >> 12)) * 0x297A2D39) & 0x7FFFFFFF
    return k ^ (k >> 15)


def _matching_pass(crow: torch.Tensor, col: torch.Tensor, val: torch.Tensor, theta: float):
    """One pass of `pairwise_aggregates` on the coalesced matrix (crow, col, val) -- unique (row, col), rows sorted --: (the aggregate
    of every vertex, the number of aggregates, the handshake rounds)."""
    n = crow.numel() - 1
    dev = val.device
    ids = torch.arange(n, device=dev)
    rows = _rows_of(crow)
    off = rows != col
    u, v = torch.minimum(rows[off], col[off]), torch.maximum(rows[off], col[off])
    key, order = torch.sort(u * n + v, stable=True)           # an undirected edge is stored once or twice
    a = val[off].abs().to(torch.float64)[order]
    key, counts = torch.unique_consecutive(key, return_counts=True)
    start = torch.cumsum(counts, 0) - counts
    w = a[start]
    two = counts > 1
    w = torch.where(two, torch.maximum(w, a[torch.where(two, start + 1, start)]), w)
    u, v = torch.div(key, n, rounding_mode="floor"), key % n
    m = torch.zeros(n, dtype=torch.float64, device=dev)       # the largest incident weight: a maximum, independent of order
    m.scatter_reduce_(0, u, w, "amax").scatter_reduce_(0, v, w, "amax")
    strong = (w > 0) & (w >= theta * torch.minimum(m[u], m[v]))
    u, v, key = u[strong], v[strong], key[strong]
    by_hash = torch.sort(_edge_hash(u, v), stable=True)[1]    # `key` ascends: ties of the hash go to the smaller u n + v
    rank = torch.empty_like(by_hash)
    rank[by_hash] = torch.arange(by_hash.numel(), device=dev)
    partner = ids.clone()
    free = torch.ones(n, dtype=torch.bool, device=dev)
    rounds = 0
    while True:
        live = free[u] & free[v]
        if not bool(live.any()):
            break
        u, v, rank = u[live], v[live], rank[live]
        best = torch.full((n,), torch.iinfo(torch.int64).max, dtype=torch.int64, device=dev)
        best.scatter_reduce_(0, u, rank, "amin").scatter_reduce_(0, v, rank, "amin")
        hit = (best[u] == rank) & (best[v] == rank)           # the smallest live rank at both ends: no two hits share a vertex
        mu, mv = u[hit], v[hit]
        partner[mu], partner[mv] = mv, mu
        free[mu] = False
        free[mv] = False
        rounds += 1
    first = torch.minimum(ids, partner)                       # the smallest member names the aggregate
    number = torch.cumsum((first == ids).to(torch.int64), 0) - 1
    return number[first], int(number[-1]) + 1, rounds


def pairwise_aggregates(A_csr: torch.Tensor, passes: int = 2, theta: float = 0.25):
    """(agg, nc): aggregates of the matrix graph of the CSR tensor `A_csr` by `passes` (1 .. 4) passes of pairwise matching on
    strong couplings.  `agg` (int64, n entries) maps a row to its aggregate in [0, nc); aggregates have 1 .. 2^passes members and
    are numbered in ascending order of their smallest member.  Torch ops whose results do not depend on the order of execution:
    the same `agg` on CPU and device.

    A pass, on a matrix with n vertices:
      coalesce   entries stored with the same (row, col) are summed in stored order (`_galerkin_agg` with identity aggregates);
      edges      e = (u, v), u < v, of weight w_e = max(|a_uv|, |a_vu|) in fp64, a direction that is not stored counting as 0;
                 m_u = the largest weight at u;
      strong     w_e > 0 and w_e >= theta * min(m_u, m_v) (the product one fp64 rounding);
      rank       strong edges by the hash h(u, v) (`_edge_hash`), the smaller first, ties to the smaller u n + v.  The weight
                 does not enter: a rank monotone in a smooth coefficient makes the handshake take O(n) rounds, a random one O(log n);
      matching   the greedy matching in rank order, by handshake rounds: an edge is live while both ends are free, every free
                 vertex takes the smallest rank among its live edges, an edge that is the smallest at both ends is matched;
      result     a matched pair or an unmatched vertex.
    Pass p + 1 runs on the Galerkin matrix of A with the composite aggregates of passes 1 .. p (one `_galerkin_agg` sum from A,
    used for the weights only) and pairs those aggregates; it is skipped once a pass has formed no pair.  nc == n exactly when the
    coalesced matrix has no non-zero off-diagonal entry."""
    if not (isinstance(A_csr, torch.Tensor) and A_csr.layout == torch.sparse_csr and A_csr.ndim == 2 and A_csr.shape[0] == A_csr.shape[1]):
        raise ValueError("pairwise_aggregates needs a square CSR tensor")
    if isinstance(passes, bool) or int(passes) != passes or not 1 <= int(passes) <= 4:
        raise ValueError(f"passes must be 1, 2, 3 or 4, got {passes}")
    theta = float(theta)
    if not 0.0 <= theta <= 1.0:
        raise ValueError(f"theta must be in [0, 1], got {theta}")
    return _pairwise_aggregates(A_csr, int(passes), theta)[:2]


def _pairwise_aggregates(A_csr, passes: int, theta: float):
    """(agg, nc, the handshake rounds of every pass run)."""
    crow, col, val = A_csr.crow_indices().to(torch.int64), A_csr.col_indices().to(torch.int64), A_csr.values()
    n = int(A_csr.shape[0])
    if n >= 2 ** 31:
        raise ValueError("pairwise_aggregates takes fewer than 2^31 rows")
    agg, nc, rounds = torch.arange(n, device=val.device), n, []
    for _ in range(passes):
        step, nc_next, r = _matching_pass(*_galerkin_agg(crow, col, val, agg, nc), theta)
        rounds.append(r)
        if nc_next == nc:
            break
        agg, nc = step[agg], nc_next
    return agg, nc, rounds


class _Level:
    """One level: `csr` (the matrix, a CSR tensor), `dims`, `n`, `dinv` (the reciprocal diagonal) and, except on the last level,
    the smoother's coefficients `c0`, `c1`, `c2` (`ChebyshevPreconditioner`'s, `smoother` is that object).  `agg`: on a level of a
    graph hierarchy that has a next one, the int64 map from its rows to the next level's; None otherwise.  A dense last level
    (`from_graph(coarse_rows=K)`) has no `dinv` and no smoother but `cinv`, the inverse of its matrix in the storage dtype as a
    contiguous (n, ld) tensor, `ld = (n + 3) & ~3`: `cinv[j, i]` is element (i, j) of the inverse -- column j of the inverse is row
    j of the tensor, so element (i, j) sits at `j * ld + i` of the memory -- and `cinv[:, n:]` is zero padding."""

    def __init__(self, csr, dims):
        self.csr, self.dims, self.n = csr, tuple(dims), int(csr.shape[0])
        self.agg = None
        crow = csr.crow_indices()
        self.max_row = int((crow[1:] - crow[:-1]).max())
        self.smoother = None
        self.dinv = None
        self.c0 = self.c1 = self.c2 = None
        self.cinv = self.ld = None


class AggregationMultigridPreconditioner:
    """M(r) = one V-cycle of aggregation multigrid for a matrix `A` whose unknowns are the points of a structured grid.

    `grid = (n0, n1)` or `(n0, n1, n2)`, slowest dimension first: row (i0 n1 + i1) n2 + i2, prod(grid) == n
    (`create_poisson_2d_csr(nx, ny)` is `grid=(nx, ny)`; the transposed grid still converges but costs several times the
    iterations).  `A` is fp64 or fp32 in any layout, on CPU or device; unsorted rows, a column stored twice and stored zeros are
    accepted.  The supported use is an SPD `A` with `cg`: M is then a fixed SPD operator.  With `bicgstab` / `gmres` it is left
    preconditioning, deterministic, and promises nothing about convergence.

    Levels.  dims_{l+1} = ceil(dims_l / 2) per dimension, down to the level L with one unknown; the aggregate of fine point
    (i0, i1, i2) is coarse point (i0 // 2, i1 // 2, i2 // 2).  A_{l+1} = P^T A_l P with the piecewise-constant P: entry (I, J) is
    the sum of the stored entries of A_l with agg(row) = I, agg(col) = J in A_l's storage order, s = first, s = s + next in the
    storage dtype; rows sorted by column, stored zeros kept -- the same bits on CPU and device.

    Smoother.  S_l is the recurrence of `ChebyshevPreconditioner(A_l, degree=degree, ratio=ratio, normalize=False)` (lmax the
    Gershgorin bound, rows summed in stored order); level L is z = dinv_L r, dinv_L = 1 / a.

    The apply V(l, r), every step a separate rounding, no fma, `omega` rounded to the storage dtype once:
        1. z = S_l(r)
        2. t = r - A_l z                          (the SpMV's residual form and its one summation order)
        3. rc[I] = the sum of t over the members of aggregate I in ascending fine index, left to right from the first member
        4. e = V(l + 1, rc)
        5. z = z + (omega * e[agg(i)])
        6. t = r - A_l z;  d = S_l(t);  z = z + d
    and M(r) = scale * V(0, r) when scale != 1.

    `cycle` ("V", the default, or "W"; the attribute `cycle`).  "W" changes step 4 where level l + 1 is a smoothed level -- not
    the last one, which is exact or diagonal and is visited once --:
        4.  e   = V(l + 1, rc)
        4a. rc2 = rc - A_{l+1} e                  (the SpMV's residual form, as step 2)
        4b. e2  = V(l + 1, rc2)
        4c. e   = e + e2                          (one rounding)
    so level l is visited 2^l times.  The V-cycle's iteration count grows with the grid over unsmoothed aggregates; the W-cycle's
    is nearly independent of it.  `omega`, `scale`, `normalize` (the estimate uses the selected cycle), `applies` and `update`
    (which keeps the cycle) are unchanged, and `cycle="V"` is the object without the keyword bit for bit.  A W hierarchy of more
    than `MG_W_MAX_LEVELS` (16) levels is a ValueError: `from_graph` without `coarse_rows` coarsens by two unknowns per level near
    the bottom and builds dozens of levels on large matrices, so `cycle="W"` there needs `coarse_rows`.

    `normalize`.  The reference decides `info` from ||M (b - A x)|| <= tol ||b|| (TSL:1007-1014) and this M approximates A^-1, norm
    about 1 / lambda_min(A): unscaled, a converged solve mostly returns info = -1.  `normalize=True` estimates the norm of the
    unscaled cycle by eight steps of the power iteration from v = ones / sqrt(n) (w = M_1 v, lambda = ||w||, v = w / lambda; the
    constant vector is close to the top eigenvector) and sets scale = 1 / lambda, a host double.  Scaling M changes neither the
    iterates nor the counts.

    Device vectors run hand-written kernels on the current stream without synchronisation: `hipk_cheb_apply` for S_l, the SpMV's
    residual form, `hipk_mg_restrict`, `hipk_mg_prolong_add`, `hipk_mg_correct` (step 6's sum and the scale) and `hipk_mg_diag`
    (level L).  `tail_rows`: the levels from the first one with at most that many unknowns on (capped at 4096; 0: none; None: the
    module constant `MG_TAIL_MAX_ROWS`) run in ONE launch of one workgroup instead, `hipk_mg_tail_apply`, bit for bit the same
    result; when one of them has a row of more than 32 stored entries the kernel's envelope is left and they all stay launches.
    `tail_from` is the first level the tail kernel runs, or None.  Level 0 uses `_hipk.handle_for(A)`, the handle a solve of `A` holds; the object owns a `CsrHandle` per coarse level
    (the handle cache holds eight entries, a deep hierarchy would flush it) and all work vectors.  CPU vectors run torch ops in
    exactly the order above, with `_SpecSpmv` for the row sums.  With `cycle="W"` step 4a is the SpMV's residual form on level
    l + 1's handle and 4c `hipk_mg_add`; the tail is `hipk_mg_tail_apply_w` (or its `gtail` / `gtail_dense` twin), which runs the
    whole W walk over its levels in its one launch and takes at most `_hipk.MG_TAIL_W_MAX_LEVELS` (12) levels, else they stay launches.
    The tail is launched once per visit of its first level: twice per visit of level `tail_from - 1` when that first level is
    smoothed, with 4a and 4c between and behind the two launches.

    `from_graph(A, ...)` builds the same object without a grid, from aggregates of the matrix graph (see there).
    `update(A_new)` refreshes an object from either constructor for new values on the same sparsity pattern: the aggregates and
    index arrays stay, the numbers are recomputed (see there; `normalize`, `updates`, `refresh_plan_bytes`).

    Attributes: `levels` (per level `csr`, `dims`, `n`, `dinv`, `c0`, `c1`, `c2`, `agg`, `cinv`), `graph` (True for `from_graph`),
    `coarse_rows` and `dense` (`from_graph(coarse_rows=K)`: K, and whether the last level is solved with `levels[-1].cinv`),
    `handshake_rounds` (graph: per level the rounds of each matching pass), `scale`, `applies`, `tail_rows`, `tail_from`,
    `launches_per_apply` (the launches of one device apply, a Chebyshev step counted as the one launch it is where the SpMV has
    the Chebyshev epilogue: 2 degree + 7 per level above the tail -- above L without one --, then one).

    `launches_per_apply` with `cycle="W"`.  k = 2 degree + 7, L the last level, T = `tail_from`, or L without a tail.  Level
    l < T is visited 2^l times at k launches; each second visit (2^(l-1) of them on level l >= 1) adds 4a and 4c; the end -- the
    tail or the last level -- is one launch per visit of level T:
        (2^T - 1) k + max(2^T - 2, 0) + E,    E = 1 if T == 0;  2^(T-1) if T == L;  2^T + 2^T otherwise
    (T == L: the last level, once per visit of level L - 1; otherwise the tail's first level is smoothed: 2^T launches of the
    tail and 2^(T-1) times 4a and 4c around them)."""

    def __init__(self, A: torch.Tensor, grid, degree: int = 1, ratio: float = 4.0, omega: float = 1.8, normalize: bool = True,
                 tail_rows=None, cycle="V"):
        self._check_matrix(A)
        try:
            dims = tuple(int(v) for v in grid)
        except TypeError:
            raise ValueError("grid must be (n0, n1) or (n0, n1, n2)") from None
        if len(dims) not in (2, 3):
            raise ValueError(f"grid must have 2 or 3 dimensions, got {len(dims)}")
        if min(dims) < 1 or math.prod(dims) != A.shape[0]:
            raise ValueError(f"grid {dims} does not have the matrix's {A.shape[0]} points")
        self._set_up(A, dims, degree, ratio, omega, normalize, tail_rows, None, None, cycle)

    @classmethod
    def from_graph(cls, A: torch.Tensor, degree: int = 1, ratio: float = 4.0, omega: float = 1.8, normalize: bool = True,
                   tail_rows=None, passes: int = 2, theta: float = 0.25, coarse_rows=None, cycle="V"):
        """The same preconditioner for ANY square `A`: the aggregates come from the matrix graph, not from a grid.

        Level l's aggregates are `pairwise_aggregates(A_l, passes, theta)` (pairwise matching on strong couplings, aggregates of
        1 .. 2^passes rows; `passes` 1 .. 4, `theta` in [0, 1]), A_{l+1} is the one-step Galerkin sum from A_l with them under the
        rule above, and steps 3 and 5 read index arrays: the members of an aggregate in ascending fine index, and agg(i).
        Coarsening ends at the first level whose graph has no pair left, which is the level without a non-zero off-diagonal entry
        -- one unknown for a connected graph, one per component otherwise --; that level is z = dinv r.  More than
        `MG_GRAPH_MAX_LEVELS` (48) levels is a ValueError: the coarsening has stalled (a star graph loses one pair per pass).
        Smoother, cycle (`cycle`), `normalize`, `tail_rows`, `applies` and `launches_per_apply` are the grid object's; every level has
        `dims == (n,)` and, except the last, `agg` (int64, the map to the next level).  The device transfers are
        `hipk_mg_restrict_agg` / `hipk_mg_prolong_add_agg`, the tail `hipk_mg_gtail_apply` (at most 32 levels, else launches).

        `coarse_rows=K` (an integer in [1, `MG_DENSE_MAX_ROWS`] = 2048; None: the hierarchy above, unchanged) ends the coarsening
        at the first level, level 0 included, of at most K unknowns -- or where the rule above ends it, whichever comes first --
        and solves that level with the inverse of its matrix.  The matching shrinks a level by 3.2 only down to a few thousand
        unknowns and by two unknowns per level below that; the cut removes those levels.  The levels above the cut are the
        default hierarchy's, bit for bit.  The dense level (`dense` is True, `levels[-1].cinv`): its coalesced matrix (entries
        stored with the same (row, col) summed in stored order) is written out densely, converted to fp64 on the CPU, inverted
        there with `torch.linalg.inv` and rounded once to the storage dtype -- the same bits from a CPU and a device matrix; a
        singular matrix or a non-finite inverse is a ValueError.  V(L, r) = cinv r in segments of 64 columns:
            p_q = 0;  p_q = p_q + (cinv[i, j] * r[j])   for j = 64 q .. min(64 q + 64, n) - 1 ascending
            s   = 0;  s   = s + p_q                     for q ascending;   z[i] = s
        one rounding per operation, no fma, in the storage dtype.  On the device it is the last level of the tail
        (`hipk_mg_gtail_dense_apply`) when `tail_rows` selects a tail, every sparse level below it fits the tail's envelope and
        the dense level has at most `MG_DENSE_TAIL_ROWS` (512) unknowns; otherwise the levels run as launches and end in one
        `hipk_mg_dense_apply`.  `launches_per_apply` keeps its formula."""
        self = cls.__new__(cls)
        cls._check_matrix(A)
        if coarse_rows is not None:
            if isinstance(coarse_rows, bool) or not isinstance(coarse_rows, numbers.Integral) or not 1 <= coarse_rows <= MG_DENSE_MAX_ROWS:
                raise ValueError(f"coarse_rows must be None or an integer in [1, {MG_DENSE_MAX_ROWS}], got {coarse_rows!r}")
            coarse_rows = int(coarse_rows)
        if isinstance(passes, bool) or int(passes) != passes or not 1 <= int(passes) <= 4:
            raise ValueError(f"passes must be 1, 2, 3 or 4, got {passes}")
        if not 0.0 <= float(theta) <= 1.0:
            raise ValueError(f"theta must be in [0, 1], got {theta}")
        self._set_up(A, (int(A.shape[0]),), degree, ratio, omega, normalize, tail_rows, (int(passes), float(theta)), coarse_rows, cycle)
        return self

    @staticmethod
    def _check_matrix(A) -> None:
        if getattr(A, "_hipk_row_block", False) is True:
            raise ValueError("AggregationMultigridPreconditioner is not available on a RowBlockCSR")
        if not (isinstance(A, torch.Tensor) and A.ndim == 2 and A.shape[0] == A.shape[1]):
            raise ValueError("AggregationMultigridPreconditioner needs a square matrix tensor")
        if A.dtype not in (torch.float64, torch.float32):
            raise ValueError(f"AggregationMultigridPreconditioner needs a float64 or float32 matrix, not {A.dtype}")

    def _set_up(self, A, dims, degree, ratio, omega, normalize, tail_rows, graph, coarse_rows, cycle) -> None:
        """Everything after the argument checks of the two constructors.  `graph`: None on a grid, else (passes, theta);
        `coarse_rows`: None, or on a graph the largest dense last level."""
        if not (isinstance(cycle, str) and cycle in ("V", "W")):
            raise ValueError(f'cycle must be "V" or "W", got {cycle!r}')
        self.cycle = cycle
        if not 1 <= int(degree) <= 32:
            raise ValueError("degree must be in [1, 32]")
        if not float(omega) > 0.0:
            raise ValueError("omega must be positive")
        self.degree, self.ratio, self.omega = int(degree), float(ratio), float(omega)
        self.shape = tuple(A.shape)
        self.dtype, self.device = A.dtype, A.device
        self._A = A.detach()
        csr = self._A if A.layout == torch.sparse_csr else \
            (self._A.coalesce() if A.layout == torch.sparse_coo else self._A).to_sparse_csr()
        self.levels = []
        self.graph = graph is not None
        self.handshake_rounds = [] if self.graph else None      # per level with a next one: the rounds of each matching pass
        self.coarse_rows, self.dense = coarse_rows, False
        while True:
            lev = _Level(csr, dims)
            if coarse_rows is not None and lev.n <= coarse_rows:      # the cut: this level is solved, not coarsened
                self._set_up_dense(lev, len(self.levels))
                self.levels.append(lev)
                self.dense = True
                break
            below = self._coarsen(csr, dims, graph)
            self._set_up_smoother(lev, len(self.levels), below is None)
            self.levels.append(lev)
            if below is None:
                break
            if self.graph and len(self.levels) == MG_GRAPH_MAX_LEVELS:
                raise ValueError(f"AggregationMultigridPreconditioner.from_graph: the coarsening has stalled, level "
                                 f"{len(self.levels) - 1} still has {lev.n} unknowns and more than {MG_GRAPH_MAX_LEVELS} "
                                 f"levels would be needed (sizes {[v.n for v in self.levels[:4]]} ...)")
            lev.agg, rounds, csr, dims = below
            if rounds is not None:
                self.handshake_rounds.append(rounds)
        L = len(self.levels) - 1
        if cycle == "W" and len(self.levels) > MG_W_MAX_LEVELS:
            raise ValueError(f'AggregationMultigridPreconditioner: cycle="W" takes at most {MG_W_MAX_LEVELS} levels (level l is visited '
                             f"2^l times), this hierarchy has {len(self.levels)} (sizes {[v.n for v in self.levels[:4]]} ...); "
                             "from_graph(coarse_rows=K) cuts the small levels off")
        from .. import _hipk          # constants only: the library is not loaded
        # the tail: the levels from the first one of at most `tail_rows` unknowns on, when they all fit the kernel's envelope
        tail_rows = MG_TAIL_MAX_ROWS if tail_rows is None else int(tail_rows)
        if tail_rows < 0:
            raise ValueError("tail_rows must be 0 (no tail kernel) or positive")
        self.tail_rows = min(tail_rows, 4096)
        first = next((l for l, lev in enumerate(self.levels) if lev.n <= self.tail_rows), None)
        fits = first is not None and all(lev.max_row <= 32 for lev in self.levels[first:len(self.levels) - self.dense]) and \
            (not self.graph or len(self.levels) - first <= 32) and (not self.dense or self.levels[-1].n <= MG_DENSE_TAIL_ROWS) and \
            (cycle == "V" or len(self.levels) - first <= _hipk.MG_TAIL_W_MAX_LEVELS)
        self.tail_from = first if fits else None
        T, k = L if self.tail_from is None else self.tail_from, 2 * self.degree + 7
        if cycle == "V":
            self.launches_per_apply = T * k + 1
        else:
            end = 1 if T == 0 else (2 ** (T - 1) if T == L else 2 ** T + 2 ** T)
            self.launches_per_apply = (2 ** T - 1) * k + max(2 ** T - 2, 0) + end
        self._cpu = None      # per level: (spec SpMV, the aggregate of every row, step 3's gather indices)
        self._dev = None      # per level: handle and work vectors of the device apply
        self._keep = {}       # what an `update` reuses: the device index arrays and work vectors, by (level, name)
        self._plan = None     # the refresh plan, built by the first `update`
        self.normalize, self.updates = bool(normalize), 0
        self.scale = 1.0
        self.applies = 0
        if normalize:
            self._estimate_scale()

    def _estimate_scale(self) -> None:
        """`scale` of `normalize=True`: eight steps of the power iteration on the unscaled cycle.  The norm is taken in fp64 on the
        host whatever the device and v = w / lambda is an element-wise quotient (a device divides by a Python number through its
        reciprocal): the applies have the same bits on CPU and device, so the two objects get the same `scale`."""
        self.scale = 1.0
        v = torch.full((self.shape[0],), 1.0 / math.sqrt(self.shape[0]), dtype=self.dtype, device=self.device)
        lam = 1.0
        for _ in range(8):
            w = self(v)
            lam = float(torch.linalg.vector_norm(w.cpu().to(torch.float64)))
            if not (lam > 0.0 and math.isfinite(lam)):
                raise ValueError("AggregationMultigridPreconditioner: the norm estimate of the V-cycle broke down "
                                 f"(||M v|| = {lam}); is the matrix symmetric positive definite?")
            v = w / torch.tensor(lam, dtype=w.dtype, device=w.device)      # a tensor: an element-wise quotient on every device
        self.scale = 1.0 / lam
        self.applies = 0

    @staticmethod
    def _coarsen(csr, dims, graph):
        """One coarsening step from the level (`csr`, `dims`): None when it is the last level, else (`agg`, the handshake rounds,
        the next level's csr, its dims).  On a grid (`graph` None) the boxes follow from `dims` and the first two are None; on
        a graph (`graph` = (passes, theta)) `agg` is the int64 map from the rows to the next level's."""
        crow, col, val = csr.crow_indices(), csr.col_indices(), csr.values()
        if graph is None:
            if csr.shape[0] == 1:
                return None
            agg = rounds = None
            crow, col, val = _galerkin(crow, col, val, dims)
            dims = _coarse_dims(dims)
        else:
            agg, n, rounds = _pairwise_aggregates(csr, *graph)
            if n == csr.shape[0]:
                return None
            crow, col, val = _galerkin_agg(crow, col, val, agg, n)
            dims = (n,)
        n = math.prod(dims)
        return agg, rounds, torch.sparse_csr_tensor(crow, col, val, size=(n, n)), dims

    def _set_up_smoother(self, lev: _Level, l: int, last: bool) -> None:
        csr = lev.csr
        try:
            if last and self.graph:          # no non-zero off-diagonal entry is left: any number of unknowns
                d = _diagonal(csr)
                if bool((d <= 0).any()):
                    raise ValueError("zero or negative entry on the diagonal")
                lev.dinv = torch.reciprocal(d)
                return
            if last:
                a = csr.values().sum() if csr.values().numel() else torch.zeros((), dtype=csr.dtype)
                if not float(a) > 0.0:
                    raise ValueError("zero or negative entry on the diagonal")
                lev.dinv = torch.reciprocal(a).reshape(1)
                return
            sm = ChebyshevPreconditioner(csr, degree=self.degree, lmax=self._gershgorin(csr), ratio=self.ratio, normalize=False)
        except ValueError as e:
            raise ValueError(f"AggregationMultigridPreconditioner, level {l} ({'x'.join(map(str, lev.dims))}): {e}") from None
        lev.smoother, lev.dinv, lev.c0, lev.c1, lev.c2 = sm, sm.dinv, sm.c0, sm.c1, sm.c2

    def _set_up_dense(self, lev: _Level, l: int) -> None:
        """`lev.cinv` of a dense last level: the inverse of its coalesced matrix, taken in fp64 on the CPU and rounded once."""
        csr, n = lev.csr, lev.n
        crow, col, val = _galerkin_agg(csr.crow_indices(), csr.col_indices(), csr.values(), torch.arange(n, device=csr.device), n)
        dense = torch.zeros((n, n), dtype=val.dtype, device=val.device)
        dense[_rows_of(crow), col] = val                          # coalesced: every (row, col) once
        self._invert_dense(lev, l, dense)

    def _invert_dense(self, lev: _Level, l: int, dense: torch.Tensor) -> None:
        """`lev.cinv` and `lev.ld` from the level's matrix written out densely, in the storage dtype on the matrix's device."""
        n = lev.n
        where = f"AggregationMultigridPreconditioner.from_graph, dense level {l} ({n})"
        try:
            inv = torch.linalg.inv(dense.to(device="cpu", dtype=torch.float64))
        except RuntimeError as e:
            raise ValueError(f"{where}: the matrix is singular ({e})") from None
        inv = inv.to(dense.dtype)
        if not bool(torch.isfinite(inv).all()):
            raise ValueError(f"{where}: the inverse is not finite; is the matrix singular?")
        lev.ld = (n + 3) & ~3
        cinv = torch.zeros((n, lev.ld), dtype=dense.dtype)
        cinv[:, :n] = inv.T                                       # row j of the tensor is column j of the inverse
        lev.cinv = cinv.to(self.device)

    @staticmethod
    def _gershgorin(csr) -> float:
        d = _diagonal(csr)
        if bool((d <= 0).any()):
            raise ValueError("zero or negative entry on the diagonal")
        return float((_abs_row_sums(csr.crow_indices(), csr.values()).to(torch.float64) / d.to(torch.float64)).max())

    # ------------------------------------------------------------------ CPU: torch ops in the documented order
    def _cpu_state(self):
        if self._cpu is None:
            st = []
            for lev in self.levels[:-1]:
                if lev.agg is not None:          # index arrays: member k of every aggregate that has one, ascending fine index
                    agg = lev.agg.cpu()
                    amem = torch.sort(agg, stable=True)[1]
                    counts = torch.bincount(agg)
                    start = torch.cumsum(counts, 0) - counts
                    members = [(counts > k, amem[torch.where(counts > k, start + k, start)]) for k in range(int(counts.max()))]
                    st.append((agg, members))
                    continue
                n0, n1, n2 = _grid3(lev.dims)
                m0, m1, m2 = _grid3(_coarse_dims(lev.dims))
                I = torch.arange(m0 * m1 * m2)
                I2, q = I % m2, torch.div(I, m2, rounding_mode="floor")
                I1, I0 = q % m1, torch.div(q, m1, rounding_mode="floor")
                members = []          # ascending fine index: d2 fastest
                for d0 in (0, 1):
                    for d1 in (0, 1):
                        for d2 in (0, 1):
                            i0, i1, i2 = 2 * I0 + d0, 2 * I1 + d1, 2 * I2 + d2
                            has = (i0 < n0) & (i1 < n1) & (i2 < n2)
                            members.append((has, torch.where(has, (i0 * n1 + i1) * n2 + i2, 0)))
                st.append((_aggregate_of(torch.arange(lev.n), lev.dims), members))
            self._cpu = st
        return self._cpu

    def _v_torch(self, l: int, r: torch.Tensor) -> torch.Tensor:
        lev = self.levels[l]
        if l == len(self.levels) - 1:
            return self._dense_torch(lev, r) if self.dense else lev.dinv.cpu() * r
        agg, members = self._cpu_state()[l]
        S = lev.smoother._apply_torch
        z = S(r)
        spmv = lev.smoother._cpu[0]         # the smoother's `_SpecSpmv` of A_l, built by its first apply
        t = r - spmv(z)
        rc = t[members[0][1]]
        for has, idx in members[1:]:
            rc = torch.where(has, rc + t[idx], rc)
        e = self._v_torch(l + 1, rc)
        if self.cycle == "W" and l + 1 < len(self.levels) - 1:      # steps 4a - 4c: the smoothed level l + 1 a second time
            rc2 = rc - self.levels[l + 1].smoother._cpu[0](e)
            e = e + self._v_torch(l + 1, rc2)
        z = z + (torch.tensor(self.omega, dtype=r.dtype) * e[agg])
        t = r - spmv(z)
        return z + S(t)

    @staticmethod
    def _dense_torch(lev: _Level, r: torch.Tensor) -> torch.Tensor:
        """z = cinv r by the dense step's rounding spec: pass k adds column 64 q + k to the partial of every segment q that has
        one (a product, then a sum, each one torch op and one rounding), then the partials are added in ascending q."""
        n = lev.n
        C = lev.cinv.cpu()[:, :n]                                 # C[j] is column j of the inverse
        first = torch.arange(0, n, DENSE_SEGMENT)
        P = torch.zeros((first.numel(), n), dtype=r.dtype)
        for k in range(min(DENSE_SEGMENT, n)):
            q = torch.nonzero(first + k < n).flatten()
            j = first[q] + k
            P[q] = P[q] + (C[j] * r[j, None])
        s = torch.zeros(n, dtype=r.dtype)
        for q in range(first.numel()):
            s = s + P[q]
        return s

    # ------------------------------------------------------------------ device: one launch per step
    def _dev_state(self):
        """Per level: the work vectors and, above the tail, the handle and the two transfers of the launch sequence as callables
        `restrict(t, rc)` and `prolong_add(omega, e, z)`; `self._end(omega, scale, r, z)` is the launch the sequence ends in.  The
        callables look the `_hipk` wrappers up at every call and hold no reference to the object."""
        if self._dev is None:
            from .. import _hipk
            dev, dt = self.device, self.dtype
            st = []
            tf = len(self.levels) if self.tail_from is None else self.tail_from
            for l, lev in enumerate(self.levels):
                # work vectors and index arrays depend on the pattern alone: an `update` finds them in `_keep`
                vec = lambda name: self._kept(l, name, lambda: torch.empty(lev.n, dtype=dt, device=dev))
                if lev.cinv is not None:         # the dense last level: nothing but its inverse
                    s = {"n": lev.n, "cinv": _hipk.aligned(lev.cinv.to(device=dev, dtype=dt)).reshape(-1), "ld": lev.ld}
                else:
                    s = {"dinv": _hipk.aligned(lev.dinv.to(device=dev, dtype=dt))}
                if l and l <= tf:
                    s["r"], s["z"] = vec("r"), vec("z")
                    if self.cycle == "W" and l < len(self.levels) - 1:      # a smoothed level: rc2 and e2 of its second visit
                        s["r2"], s["z2"] = vec("r2"), vec("z2")
                if lev.agg is not None:          # the transfers' index arrays: agg, and the members aggregate by aggregate
                    if (l, "agg") not in self._keep:
                        agg = lev.agg.to(dev)
                        counts = torch.bincount(agg, minlength=self.levels[l + 1].n)
                        self._keep[l, "agg"] = _hipk.aligned(agg.to(torch.int32))
                        self._keep[l, "amem"] = _hipk.aligned(torch.sort(agg, stable=True)[1].to(torch.int32))
                        self._keep[l, "aptr"] = _hipk.aligned(torch.cat([counts.new_zeros(1), torch.cumsum(counts, 0)]).to(torch.int32))
                    s.update({name: self._keep[l, name] for name in ("agg", "amem", "aptr")})
                c = lev.csr
                if l >= tf and lev.cinv is None:          # a level of the tail kernel: int32 CSR arrays for its descriptor
                    crow, col = self._int32_pattern(l)
                    s.update(crow=crow, col=col,
                             val=_hipk.aligned(c.values()), dims=lev.dims, max_row=lev.max_row, c0=lev.c0, c1=lev.c1, c2=lev.c2)
                    if "r2" in s:                         # the W-cycle's step 4a on the tail's first level is a launch
                        s["h"] = self._level_handle(l)
                elif l < min(tf, len(self.levels) - 1):   # a level of the launch sequence that has a next one
                    s["h"] = _hipk.handle_for(self._A) if l == 0 else self._level_handle(l)
                    s["t"], s["d"] = vec("t"), vec("d")
                    s["work"] = self._kept(l, "work", lambda: torch.empty(2 * ((lev.n + 3) & ~3) * c.values().element_size(),
                                                                          dtype=torch.uint8, device=dev))
                    if lev.agg is None:
                        s["restrict"] = lambda t, rc, dims=lev.dims: _hipk.mg_restrict(dims, t, rc)
                        s["prolong_add"] = lambda omega, e, z, dims=lev.dims: _hipk.mg_prolong_add(dims, omega, e, z)
                    else:
                        s["restrict"] = lambda t, rc, aptr=s["aptr"], amem=s["amem"]: _hipk.mg_restrict_agg(aptr, amem, t, rc)
                        s["prolong_add"] = lambda omega, e, z, agg=s["agg"]: _hipk.mg_prolong_add_agg(agg, omega, e, z)
                st.append(s)
            last = st[-1]
            if tf < len(self.levels):
                w = "_w" if self.cycle == "W" else ""      # the W tails: the same descriptors, a larger workspace
                if self.dense:
                    tail = _hipk.MgGTail(st[tf:], self.degree, cinv=last["cinv"], ld=last["ld"], cycle=self.cycle)
                    self._end = lambda omega, scale, r, z: getattr(_hipk, "mg_gtail_dense_apply" + w)(tail, omega, scale, r, z, work=work)
                elif self.graph:
                    tail = _hipk.MgGTail(st[tf:], self.degree, cycle=self.cycle)
                    self._end = lambda omega, scale, r, z: getattr(_hipk, "mg_gtail_apply" + w)(tail, omega, scale, r, z, work=work)
                else:
                    tail = _hipk.MgTail(st[tf:], self.degree, cycle=self.cycle)
                    self._end = lambda omega, scale, r, z: getattr(_hipk, "mg_tail_apply" + w)(tail, omega, scale, r, z, work=work)
                self._tail = tail
                work = self._kept(tf, "tail work" + w, lambda: torch.empty(tail.work_bytes, dtype=torch.uint8, device=dev))
            elif self.dense:
                self._end = lambda omega, scale, r, z: _hipk.mg_dense_apply(last["cinv"], last["ld"], scale, r, z)
            else:
                self._end = lambda omega, scale, r, z: _hipk.mg_diag(scale, last["dinv"], r, z)
            self._dev = st
        return self._dev

    def _apply_device(self, v: torch.Tensor) -> torch.Tensor:
        from .. import _hipk
        st, levels = self._dev_state(), self.levels
        L = len(levels) - 1 if self.tail_from is None else self.tail_from      # the last level the launches reach
        v = _hipk.aligned(v)
        out = torch.empty_like(v)
        smooth = lambda l, src, dst: _hipk.cheb_apply(st[l]["h"], self.degree, st[l]["dinv"], levels[l].smoother._coef, src,
                                                      work=st[l]["work"], out=dst)

        def visit(l, r, z):          # z = V(l, r), scaled on level 0
            if l == L:               # level L, or the tail from it on
                self._end(self.omega, self.scale if L == 0 else 1.0, r, z)
                return
            s, c = st[l], st[l + 1]
            smooth(l, r, z)                                                     # steps 1 - 3
            _hipk.spmv_residual(s["h"], z, r, s["t"])
            s["restrict"](s["t"], c["r"])
            visit(l + 1, c["r"], c["z"])                                        # step 4
            if "r2" in c:                                                       # steps 4a - 4c of the W-cycle
                _hipk.spmv_residual(c["h"], c["z"], c["r"], c["r2"])
                visit(l + 1, c["r2"], c["z2"])
                _hipk.mg_add(c["z2"], c["z"])
            s["prolong_add"](self.omega, c["z"], z)                             # steps 5 - 6
            _hipk.spmv_residual(s["h"], z, r, s["t"])
            smooth(l, s["t"], s["d"])
            _hipk.mg_correct(self.scale if l == 0 else 1.0, s["d"], z)

        visit(0, v, out)
        return out

    def __call__(self, v):
        n = self.shape[0]
        if not isinstance(v, torch.Tensor) or v.shape != (n,):
            raise ValueError(f"AggregationMultigridPreconditioner for {n} unknowns applied to a vector of shape "
                             f"{tuple(getattr(v, 'shape', ()))}")
        if v.dtype != self.dtype or v.device != self.device:
            raise ValueError(f"AggregationMultigridPreconditioner of a {self.dtype} matrix on {self.device} applied to a {v.dtype} "
                             f"vector on {v.device}")
        if v.is_cuda:
            z = self._apply_device(v.detach())
        else:
            z = self._v_torch(0, v.detach())
            if self.scale != 1.0:
                z = torch.tensor(self.scale, dtype=v.dtype) * z
        self.applies += 1
        return z

    # ------------------------------------------------------------------ update: new values on the same pattern
    def _kept(self, l: int, name: str, make):
        """The device tensor (`l`, `name`) of `_keep`, made on first use: index arrays and work vectors, which follow from the
        sparsity patterns alone and so outlive every `update`."""
        if (l, name) not in self._keep:
            self._keep[l, name] = make()
        return self._keep[l, name]

    def _int32_pattern(self, l: int):
        """Level l's row pointers and columns as aligned int32 device arrays (the tail's descriptors and the level scan read them)."""
        from .. import _hipk
        c = self.levels[l].csr
        return (self._kept(l, "crow", lambda: _hipk.aligned(c.crow_indices().to(torch.int32))),
                self._kept(l, "col", lambda: _hipk.aligned(c.col_indices().to(torch.int32))))

    def _level_handle(self, l: int):
        """The `CsrHandle` of coarse level l: constructed once and kept in `_keep` -- its pattern-dependent half outlives every
        `update` --, and given the level's values (`CsrHandle.update_values`) when it holds others."""
        from .. import _hipk
        c = self.levels[l].csr
        h = self._keep.get((l, "h"))
        if h is None:
            h = self._keep[l, "h"] = _hipk.CsrHandle(c.crow_indices(), c.col_indices(), c.values(), c.shape)
        else:
            val = _hipk.aligned(c.values())
            if h.val.data_ptr() != val.data_ptr():        # (h.val keeps its tensor alive: an equal address is the same tensor)
                h.update_values(val)
        return h

    def _handles_back(self, A_new) -> None:
        """After an `update` that raised: the kept handles that already took the new values (the norm estimate applies the new
        hierarchy before the swap) are updated back to this object's values, and level 0's cached handle, if `A_new` took it over,
        goes back to `_A`.  An updated handle is the fresh handle of its values, so the object is bit for bit what it was."""
        if self.device.type != "cuda":
            return
        from .. import _hipk
        for (l, name) in [k for k in self._keep if k[1] == "h"]:
            self._level_handle(l)
        if A_new.layout == torch.sparse_csr and self._A.layout == torch.sparse_csr:
            try:
                _hipk.refresh_matrix(self._A, like=A_new)
            except ValueError:                            # index tensors of its own: the handle never moved
                pass

    def update(self, A_new: torch.Tensor) -> "AggregationMultigridPreconditioner":
        """Refresh the hierarchy for a matrix with the SAME sparsity pattern and new values, and return self: what AMG packages
        call a re-setup.  The aggregates of every level (the boxes of a grid, `agg` of a graph hierarchy) and every index array
        stay; the numbers are recomputed under the constructors' rounding rules, so the object is the one the constructor would
        have produced for `A_new` with every level's aggregates held fixed:
          values    `levels[l + 1].csr` holds the Galerkin sum of `levels[l].csr`, s = first, s = s + next over the fine storage
                    order, on the unchanged pattern;
          smoother  every level's `dinv`, the Gershgorin bound (rows summed in stored order) and `c0`, `c1`, `c2` with the
                    constructor's `degree` and `ratio`; the last level of a graph hierarchy stays z = dinv r from its diagonal;
          dense     `cinv` of a dense last level from the fp64 inversion on the CPU, rounded once, in the same layout;
          scale     re-estimated by the same eight power-iteration steps when the object was built with `normalize=True`;
          counters  `applies` goes back to 0, `updates` counts the successful calls.
        `agg`, `dims`, `max_row`, `tail_rows`, `tail_from`, `launches_per_apply`, `handshake_rounds`, `dense` and `coarse_rows` do
        not change.  A CPU object and a device object refreshed with the same values hold the same bits.

        `A_new` has the shape, dtype and device of the matrix the object was built from and goes through the same conversion to
        CSR (CSR taken as it is, COO coalesced); its `crow_indices` / `col_indices` must equal level 0's, stored zeros counting
        as pattern.  Anything else is a ValueError that names what differs.

        All or nothing: the new state is built beside the old one and swapped in at the end.  When the call raises -- a
        non-positive diagonal on some level, 0 < lmin < lmax violated, a singular dense level or a broken-down norm estimate,
        each with the constructor's message --, the object is exactly what it was.

        The first call builds the refresh plan (`refresh_plan_bytes`): per level with a next one the stable sort order of the
        Galerkin keys, `gsrc`, and the segment starts `gptr` (int32 on a device object, which needs nnz < 2^31; int64 on a CPU
        object), and for a dense level the slot of each stored entry.  Later calls sort nothing.  On the device the Galerkin sums
        are `hipk_mg_restrict_agg` over (gptr, gsrc), every level's dinv / bound / diagonal check is one `hipk_mg_level_scan`,
        and the bounds of all levels come back in one copy; the coarse levels' `CsrHandle`s are kept and given the new values
        (`CsrHandle.update_values`: nothing that follows from a level's pattern is rebuilt), level 0's cached handle moves to
        `A_new` (`refresh_matrix(A_new, like=` the old matrix`)`) when `A_new` is a CSR tensor on the old matrix's index tensors and
        is `_hipk.handle_for(A_new)` otherwise; the tail's descriptors are rebuilt, index arrays and work vectors are reused.  When
        the call raises after handles took the new values, they are updated back."""
        what = "AggregationMultigridPreconditioner.update"
        self._check_matrix(A_new)
        if tuple(A_new.shape) != self.shape:
            raise ValueError(f"{what}: the matrix has shape {tuple(A_new.shape)}, the object was built from one of shape {self.shape}")
        if A_new.dtype != self.dtype:
            raise ValueError(f"{what}: the matrix is {A_new.dtype}, the object was built from a {self.dtype} matrix")
        if A_new.device != self.device:
            raise ValueError(f"{what}: the matrix is on {A_new.device}, the object was built from a matrix on {self.device}")
        A = A_new.detach()
        csr = A if A.layout == torch.sparse_csr else (A.coalesce() if A.layout == torch.sparse_coo else A).to_sparse_csr()
        old = self.levels[0].csr
        if csr.values().numel() != old.values().numel():
            raise ValueError(f"{what}: the sparsity pattern differs, the matrix stores {csr.values().numel()} entries and the one "
                             f"the object was built from {old.values().numel()}")
        for name in ("crow_indices", "col_indices"):
            if not torch.equal(getattr(csr, name)().to(torch.int64), getattr(old, name)().to(torch.int64)):
                raise ValueError(f"{what}: the sparsity pattern differs, {name} are not those of the matrix the object was built from")
        try:
            state = self._refreshed(A, csr, self._refresh_plan()).__dict__
        except BaseException:
            self._handles_back(A)
            raise
        self.__dict__.clear()
        self.__dict__.update(state)
        return self

    @property
    def refresh_plan_bytes(self) -> int:
        """The memory of the refresh plan on the matrix's device: `gsrc`, `gptr`, the dense level's slots and, on a device, the
        scan's results and workspace and the int32 patterns it reads (which the tail's levels share).  0 before the first `update`."""
        if self._plan is None:
            return 0
        held = list(self._plan["tensors"]) + [t for (_, name), t in self._keep.items() if name in ("crow", "col")]
        return sum(t.numel() * t.element_size() for t in held)

    def _refresh_plan(self):
        """The plan of `update`, built once: {"steps": per level with a next one {"gsrc", "gptr", "longest"} -- the stable sort
        order of the keys agg(row) nc + agg(col), the segment starts (nnz_{l+1} + 1 entries) and the longest segment --, "dense":
        None or {"slots", "gsrc", "gptr", "longest"} -- the index of each entry in the flattened dense matrix, and the order /
        segments of its coalescing where an entry is stored more than once (None otherwise) --, "res" / "work": the level
        scans' results and workspace on a device, "tensors": everything above that holds memory}."""
        if self._plan is not None:
            return self._plan
        on_dev = self.device.type == "cuda"
        if on_dev:
            from .. import _hipk
        index = lambda t: _hipk.aligned(t.to(torch.int32)) if on_dev else t
        tensors = []

        def ordered(key):
            if on_dev and key.numel() >= 2 ** 31:
                raise ValueError("AggregationMultigridPreconditioner.update: the device refresh plan needs nnz < 2^31 on every level, "
                                 f"got {key.numel()}")
            order, start, counts, ukey = _galerkin_order(key)
            step = {"gsrc": index(order), "gptr": index(torch.cat([start, start.new_full((1,), key.numel())])),
                    "longest": int(counts.max()) if counts.numel() else 0}
            tensors.extend([step["gsrc"], step["gptr"]])
            return step, ukey

        steps = []
        for lev, nxt in zip(self.levels[:-1], self.levels[1:]):
            crow, col = lev.csr.crow_indices().to(torch.int64), lev.csr.col_indices().to(torch.int64)
            if lev.agg is None:
                key = _aggregate_of(_rows_of(crow), lev.dims) * nxt.n + _aggregate_of(col, lev.dims)
            else:
                key = lev.agg[_rows_of(crow)] * nxt.n + lev.agg[col]
            steps.append(ordered(key)[0])
        dense = None
        if self.dense:
            lev = self.levels[-1]
            crow, col = lev.csr.crow_indices().to(torch.int64), lev.csr.col_indices().to(torch.int64)
            key = _rows_of(crow) * lev.n + col
            dense = {"slots": key, "gsrc": None}
            if len(self.levels) == 1:          # the caller's matrix: an entry may be stored more than once
                step, ukey = ordered(key)
                if step["longest"] > 1:
                    dense = dict(step, slots=ukey)
            tensors.append(dense["slots"])
        plan = {"steps": steps, "dense": dense, "tensors": tensors}
        if on_dev:
            plan["res"] = torch.zeros((len(self.levels), 2), dtype=torch.float64, device=self.device)
            plan["work"] = torch.empty(max(_hipk.mg_level_scan_work_bytes(lev.n) for lev in self.levels), dtype=torch.uint8,
                                       device=self.device)
            tensors.extend([plan["res"], plan["work"]])
        self._plan = plan
        return plan

    def _segment_sum(self, step, v: torch.Tensor) -> torch.Tensor:
        """The sums of `v` over the segments of a plan step, each s = first, s = s + next in the stored sort order."""
        if v.is_cuda:
            from .. import _hipk
            out = torch.empty(step["gptr"].numel() - 1, dtype=v.dtype, device=v.device)
            return _hipk.mg_restrict_agg(step["gptr"], step["gsrc"], _hipk.aligned(v), out)
        start = step["gptr"][:-1]
        return _segment_sums(v[step["gsrc"]], start, step["gptr"][1:] - start, step["longest"])

    def _refreshed(self, A, csr, plan):
        """The object `update` swaps in: a shallow copy of this one with new levels, `_A` and device state, built without touching
        this one.  The plan, the kept index arrays and work vectors and the CPU gather indices are shared and hold no value.  The
        `CsrHandle`s of `_keep` are shared too and DO hold values: the new object's first apply (the norm estimate below, when
        there is one) gives them the new levels' values while this object still refers to them, which is why `update` calls
        `_handles_back` when this function raises.  `_level_handle` takes a handle for current when it borrows the level's own
        values tensor (equal `data_ptr`); that holds because every level of the new object gets a values tensor of its own
        below (`A_new`'s for level 0, a fresh Galerkin sum for each coarse level) while the old levels keep theirs alive, so two
        levels' values never share an address."""
        new = object.__new__(type(self))
        new.__dict__.update(self.__dict__)
        new._A, new._dev, new.scale, new.applies, new.updates = A, None, 1.0, 0, self.updates + 1
        new.__dict__.pop("_tail", None)
        new.__dict__.pop("_end", None)
        L = len(self.levels) - 1
        new.levels = []
        val = csr.values()
        for l, old in enumerate(self.levels):
            lev = _Level.__new__(_Level)
            lev.__dict__.update(old.__dict__)
            c = old.csr
            lev.csr = csr if l == 0 else torch.sparse_csr_tensor(c.crow_indices(), c.col_indices(), val, size=c.shape)
            lev.smoother = lev.dinv = lev.c0 = lev.c1 = lev.c2 = lev.cinv = None
            new.levels.append(lev)
            if l < L:
                val = self._segment_sum(plan["steps"][l], val)
        if self.device.type == "cuda" and L > 0:
            new._scan_levels(plan)
        else:      # torch ops through the plan (a one-level device object has nothing to enqueue: the constructor's path)
            for l, lev in enumerate(new.levels):
                if self.dense and l == L:
                    new._refresh_dense(lev, l, plan)
                else:
                    new._set_up_smoother(lev, l, l == L)
        if self.device.type == "cuda" and A.layout == torch.sparse_csr and self._A.layout == torch.sparse_csr and A is not self._A:
            from .. import _hipk
            try:                                          # level 0: the handle the solves of the old matrix hold goes to the new one
                _hipk.refresh_matrix(A, like=self._A)
            except ValueError:                            # index tensors of its own: `handle_for` builds A's handle as it always did
                pass
        if self.normalize:
            new._estimate_scale()
        return new

    def _refresh_dense(self, lev: _Level, l: int, plan) -> None:
        """`_set_up_dense` through the plan's slots: an indexed store instead of the coalescing sort."""
        d, val = plan["dense"], lev.csr.values()
        if d["gsrc"] is not None:
            val = self._segment_sum(d, val)
        dense = torch.zeros(lev.n * lev.n, dtype=val.dtype, device=val.device)
        dense[d["slots"]] = val
        self._invert_dense(lev, l, dense.view(lev.n, lev.n))

    def _scan_levels(self, plan) -> None:
        """The device form of the per-level set-up: one `hipk_mg_level_scan` per sparse level, all enqueued before the one copy
        that brings every level's (bound, non-positive diagonal entries) back; the coefficients are formed on the host."""
        from .. import _hipk
        L = len(self.levels) - 1
        res = plan["res"]
        for l, lev in enumerate(self.levels):
            if self.dense and l == L:
                continue
            crow, col = self._int32_pattern(l)
            lev.dinv = torch.empty(lev.n, dtype=self.dtype, device=self.device)
            # the bound is needed where there is a smoother; the one unknown of a grid's last level takes it as its NaN check
            _hipk.mg_level_scan(crow, col, _hipk.aligned(lev.csr.values()), l < L or not self.graph, lev.dinv, res[l], plan["work"])
        host = res.cpu()
        for l, lev in enumerate(self.levels):
            if self.dense and l == L:
                self._refresh_dense(lev, l, plan)
                continue
            where = f"AggregationMultigridPreconditioner, level {l} ({'x'.join(map(str, lev.dims))})"
            lmax, bad = float(host[l, 0]), float(host[l, 1])
            if bad > 0 or (l == L and math.isnan(lmax)):
                raise ValueError(f"{where}: zero or negative entry on the diagonal")
            if l == L:
                continue
            sm = ChebyshevPreconditioner.__new__(ChebyshevPreconditioner)
            sm.degree, sm.shape, sm._A, sm.dinv, sm._cpu, sm._dev = self.degree, tuple(lev.csr.shape), lev.csr, lev.dinv, None, None
            try:
                sm._set_coefficients(lmax, None, self.ratio, False, 0.0)
            except ValueError as e:
                raise ValueError(f"{where}: {e}") from None
            lev.smoother, lev.c0, lev.c1, lev.c2 = sm, sm.c0, sm.c1, sm.c2
