"""AggregationMultigridPreconditioner.update on CPU tensors (no GPU): the refreshed object against freshly built ones and against the
mirrors, every comparison of numbers bitwise.

"The same object" below: the level values, `dinv`, the coefficients, `cinv` and `scale` of two objects compare equal.
  1. refreshing with the same matrix gives back the same object; on the grid class the refreshed object IS the freshly built one
     (its boxes do not depend on the values); on a graph hierarchy refreshing with 4 A gives the object from_graph(4 A) builds (a
     power-of-two scaling leaves every strength test and the hash ranking unchanged);
  2. for a genuinely different matrix of the same pattern every level's values are the mirror's Galerkin sum with the object's own
     aggregates, dinv and the coefficients are ChebyshevPreconditioner's for the Gershgorin bound of tests/_mg_refresh_mirror.py,
     cinv is tests/_mg_dense_mirror.py's stored inverse, M(r) is the mirror V-cycle on the refreshed levels, and a second update
     with the first matrix returns to the first object's bits;
  3. no sort runs after the first update (torch.sort is patched);
  4. the errors, each leaving M(r) bitwise unchanged;
  5. cg iteration counts on the t-family (k = exp((4 - 6 t) x + 3 sin(6 y + 5 t)) at the cell faces of a 64 x 64 grid, hierarchy
     built at t = 0, fp64, b = ones, tol 1e-6).  Measured with this generator, for coarse_rows None / 256, at
     t = 0.05, 0.1, 0.2, 0.4, 0.7, 1.0:   built afresh 17 17 18 17 18 17 / 16 16 16 17 16 15,   refreshed 19 18 18 18 18 17 /
     17 17 17 16 16 16,   stale 32 68 318 4081 .. / 31 67 314 4092 ..; plain cg at t = 0 needs 5622."""
import numpy as np
import pytest
import torch

import _mg_dense_mirror as DM
import _mg_graph_mirror as GM
import _mg_mirror as MM
import _mg_refresh_mirror as RM
from _order_cases import TRANSFORMS
from pytorch_sparse_solver.module_a import AggregationMultigridPreconditioner, ChebyshevPreconditioner, cg, get_last_stats
from pytorch_sparse_solver.utils.matrix_utils import create_poisson_2d_csr, create_variable_diffusion_2d_csr

P = AggregationMultigridPreconditioner
DTYPES = [np.float64, np.float32]


def _np(A):
    return A.crow_indices().numpy(), A.col_indices().numpy(), A.values().numpy()


# name -> (grid, the matrix the object is built from, a genuinely different matrix of the same pattern)
SYSTEMS = {
    "poisson17x13": ((17, 13), lambda: _np(create_poisson_2d_csr(17, 13)), lambda: _np(create_variable_diffusion_2d_csr(17, 13, contrast=3.0, seed=7))),
    "poisson32x32": ((32, 32), lambda: _np(create_poisson_2d_csr(32, 32)), lambda: _np(create_variable_diffusion_2d_csr(32, 32, contrast=3.0, seed=7))),
    "seven_point9x7x5": ((9, 7, 5), lambda: MM.grid_matrix((9, 7, 5)), lambda: MM.grid_matrix((9, 7, 5), seed=3)),
    "vardiff32x32": ((32, 32), lambda: _np(create_variable_diffusion_2d_csr(32, 32)), lambda: _np(create_variable_diffusion_2d_csr(32, 32, contrast=3.0, seed=7))),
}
# the stored order of the entries: as built, shuffled, split-entry, stored-zero, reversed-row
ORDERS = {"sorted": None, "shuffled": "shuf", "split": "dup", "zero": "zero", "reversed": "rev"}
KINDS = {"grid": lambda A, grid, **kw: P(A, grid, **kw), "graph": lambda A, grid, **kw: P.from_graph(A, **kw),
         "dense64": lambda A, grid, **kw: P.from_graph(A, coarse_rows=64, **kw)}
_arrays = {}


def _pair(system, order, dtype):
    """(grid, the arrays of the first matrix, those of the other one): one pattern, shared by the tests."""
    key = (system, order, np.dtype(dtype).name)
    if key not in _arrays:
        grid, first, other = SYSTEMS[system]
        out = []
        for arrs in (first(), other()):
            crow, col, val = (np.asarray(arrs[0], dtype=np.int64), np.asarray(arrs[1], dtype=np.int64), np.asarray(arrs[2], dtype=np.float64))
            if ORDERS[order] is not None:
                crow, col, val = TRANSFORMS[ORDERS[order]](crow, col, val, seed=5)
            out.append((crow, col, val.astype(dtype)))
        assert RM.same_pattern(*out) and not np.array_equal(out[0][2], out[1][2])
        _arrays[key] = (grid, out[0], out[1])
    return _arrays[key]


def _state(M):
    """Everything `update` recomputes, as bytes."""
    out = {"scale": M.scale}
    for l, lev in enumerate(M.levels):
        out[l] = (lev.csr.values().numpy().tobytes(), None if lev.dinv is None else lev.dinv.numpy().tobytes(), lev.c0,
                  None if lev.c1 is None else tuple(lev.c1), None if lev.c2 is None else tuple(lev.c2),
                  None if lev.cinv is None else lev.cinv.numpy().tobytes())
    return out


def _kept(M):
    return ([None if lev.agg is None else lev.agg.clone() for lev in M.levels], [lev.dims for lev in M.levels], [lev.max_row for lev in M.levels],
            M.tail_rows, M.tail_from, M.launches_per_apply, M.handshake_rounds, M.dense, M.coarse_rows,
            [(lev.csr.crow_indices().clone(), lev.csr.col_indices().clone()) for lev in M.levels])


def _same_kept(a, b):
    for x, y in zip(a[0], b[0]):
        assert (x is None) == (y is None) and (x is None or torch.equal(x, y))
    assert a[1:9] == b[1:9]
    for (c0, j0), (c1, j1) in zip(a[9], b[9]):
        assert torch.equal(c0, c1) and torch.equal(j0, j1)


CASES = [(s, o, k) for s in SYSTEMS for o in ORDERS for k in KINDS]


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
@pytest.mark.parametrize("system, order, kind", CASES, ids=["-".join(c) for c in CASES])
def test_the_three_equalities(system, order, kind, dtype):
    grid, first, other = _pair(system, order, dtype)
    build = KINDS[kind]
    A = MM.csr_tensor(*first)
    M0, M = build(A, grid), build(A, grid)
    kept = _kept(M)
    assert M.updates == 0 and M.refresh_plan_bytes == 0 and M.normalize is True
    M(torch.ones(A.shape[0], dtype=A.dtype))
    assert M.update(A) is M and M.updates == 1 and M.applies == 0 and M.refresh_plan_bytes > 0
    assert _state(M) == _state(M0), "refreshing with the same matrix changed the object"
    _same_kept(_kept(M), kept)
    if kind == "grid":
        B = MM.csr_tensor(*other)
    else:
        B = MM.csr_tensor(first[0], first[1], first[2] * dtype(4))
    M.update(B)
    assert M.updates == 2 and _state(M) == _state(build(B, grid)), "the refreshed object is not the freshly built one"
    _same_kept(_kept(M), kept)


def _galerkin_mirror(M, l, arrs):
    lev = M.levels[l]
    if lev.agg is None:
        return MM.galerkin(*arrs, lev.dims)
    return GM.galerkin_agg(*arrs, lev.agg.numpy(), M.levels[l + 1].n)


def _check_against_mirrors(oracle, M, arrs, degree, ratio):
    """The refreshed object `M` of the matrix `arrs`: values, numerics and apply."""
    dtype = arrs[2].dtype.type
    L = len(M.levels) - 1
    for l, lev in enumerate(M.levels):
        got = _np(lev.csr)
        assert RM.same_pattern(got, arrs) and DM.same_bits(got[2], arrs[2]), f"level {l}: not the mirror's Galerkin sum"
        if M.dense and l == L:
            assert lev.dinv is None and lev.smoother is None
            assert DM.same_bits(lev.cinv.reshape(-1).numpy(), DM.stored_inverse(DM.dense_matrix(*arrs)))
            break
        dinv, lmax, bad = RM.level_scan(*arrs, want_lmax=l < L)
        assert bad == 0 and DM.same_bits(lev.dinv.numpy(), dinv), f"level {l}: dinv"
        if l == L:
            assert lev.smoother is None and lev.c0 is None
            break
        ref = ChebyshevPreconditioner(lev.csr, degree=degree, lmax=lmax, ratio=ratio, normalize=False)
        assert (lev.c0, lev.c1, lev.c2) == (ref.c0, ref.c1, ref.c2) and DM.same_bits(lev.dinv.numpy(), ref.dinv.numpy())
        assert lev.smoother.lmax == lmax
        arrs = _galerkin_mirror(M, l, arrs)
    r = np.random.default_rng(3).standard_normal(M.shape[0]).astype(dtype)
    z = M(torch.from_numpy(r)).numpy()
    ref = DM.apply(oracle, M, r) if M.graph else MM.apply(oracle, M, r)
    assert DM.same_bits(z, ref), f"{np.count_nonzero(DM.bits(z) != DM.bits(ref))} of {len(z)} entries of M(r) differ from the mirror"
    return z


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
@pytest.mark.parametrize("system, order, kind", CASES, ids=["-".join(c) for c in CASES])
def test_a_different_matrix_gives_the_mirrors_numbers_and_the_way_back(oracle, monkeypatch, system, order, kind, dtype):
    grid, first, other = _pair(system, order, dtype)
    A, B = MM.csr_tensor(*first), MM.csr_tensor(*other)
    M = KINDS[kind](A, grid, degree=2, ratio=5.0)
    before = _state(M)
    M.update(B)
    assert M.scale != 1.0 and M.scale != before["scale"]
    _check_against_mirrors(oracle, M, other, 2, 5.0)

    def no_sort(*a, **kw):
        raise AssertionError("torch.sort after the first update")
    with monkeypatch.context() as mp:
        mp.setattr(torch, "sort", no_sort)
        mp.setattr(torch.Tensor, "sort", no_sort)
        mp.setattr(torch, "argsort", no_sort)
        mp.setattr(torch.Tensor, "argsort", no_sort)
        M.update(A)
        assert _state(M) == before, "the second update did not return to the first object's bits"
        assert M.updates == 2 and M.applies == 0
        M.update(B.to_sparse_coo() if order == "sorted" else B)
        M(torch.ones(A.shape[0], dtype=A.dtype))
    assert M.updates == 3 and M.applies == 1


def test_normalize_false_is_kept_and_counters_move():
    grid, first, other = _pair("poisson17x13", "sorted", np.float64)
    M = P.from_graph(MM.csr_tensor(*first), normalize=False)
    assert M.normalize is False and M.scale == 1.0
    M(torch.ones(221, dtype=torch.float64))
    M.update(MM.csr_tensor(*other))
    assert M.scale == 1.0 and M.applies == 0 and M.updates == 1


def test_a_dense_level_0_with_entries_stored_twice(oracle):
    """coarse_rows above the matrix: level 0 is the dense level, and the caller's matrix may store an entry twice."""
    grid, first, other = _pair("poisson17x13", "split", np.float64)
    M = P.from_graph(MM.csr_tensor(*first), coarse_rows=221)
    assert len(M.levels) == 1 and M.dense
    M.update(MM.csr_tensor(*other))
    _check_against_mirrors(oracle, M, other, 1, 4.0)
    assert _state(M) == _state(P.from_graph(MM.csr_tensor(*other), coarse_rows=221))


# ------------------------------------------------------------------------------------------------------------------------ errors
def _path(ends, n=8):
    rows = [[(i, ends if i in (0, n - 1) else 2.0)] + [(j, -1.0) for j in (i - 1, i + 1) if 0 <= j < n] for i in range(n)]
    crow = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    return crow, np.array([c for r in rows for c, _ in r]), np.array([v for r in rows for _, v in r])


@pytest.mark.parametrize("kind", list(KINDS))
def test_errors_leave_the_object_as_it_was(kind):
    grid, first, other = _pair("poisson17x13", "zero", np.float64)
    crow, col, val = first
    A = MM.csr_tensor(crow, col, val)
    M = KINDS[kind](A, grid)
    M.update(MM.csr_tensor(*other))
    M.update(A)
    r = torch.from_numpy(np.random.default_rng(2).standard_normal(221))
    z0, state, updates = M(r).clone(), _state(M), M.updates

    def refused(A_new, match):
        with pytest.raises(ValueError, match=match):
            M.update(A_new)
        assert M.updates == updates and _state(M) == state
        assert torch.equal(M(r), z0), f"M(r) changed after the refused update ({match})"

    moved = col.copy()                                            # another pattern: one column moved, and one entry fewer
    k = int(np.flatnonzero(col[crow[5]:crow[6]] != 5)[0]) + int(crow[5])
    moved[k] = 200
    refused(MM.csr_tensor(crow, moved, val), "col_indices")
    fewer = np.concatenate([crow[:1], crow[1:] - 1])
    refused(MM.csr_tensor(fewer, col[1:], val[1:]), "pattern")
    shifted = crow.copy()
    shifted[1] -= 1                                                # the same entries, one of them in the next row
    refused(MM.csr_tensor(shifted, col, val), "crow_indices")
    dense = MM.csr_tensor(crow, col, val).to_dense()              # a strided matrix drops the stored zeros: the pattern moved
    refused(dense, "pattern")
    refused(create_poisson_2d_csr(13, 13), "shape")
    refused(MM.csr_tensor(crow, col, val.astype(np.float32)), "float32")
    refused(MM.csr_tensor(crow, col, val).to("meta"), "meta")
    negated = val.copy()
    negated[int(np.flatnonzero(col[crow[7]:crow[8]] == 7)[0]) + int(crow[7])] *= -1.0
    refused(MM.csr_tensor(crow, col, negated), r"level 0 \(.*\): zero or negative entry on the diagonal")

    class FakeRowBlock:
        _hipk_row_block = True
    refused(FakeRowBlock(), "RowBlockCSR")
    refused(val, "square matrix")


def test_a_singular_dense_level_is_refused():
    """The Dirichlet path's hierarchy refreshed with the Neumann path: row sums exactly 0 on every level."""
    D, N = _path(2.0), _path(1.0)
    sizes = [len(lev[0]) - 1 for lev in GM.hierarchy(*D)]
    M = P.from_graph(MM.csr_tensor(*D), coarse_rows=sizes[1])
    assert M.dense and [lev.n for lev in M.levels] == sizes[:2]
    r = torch.from_numpy(np.random.default_rng(2).standard_normal(8))
    z0, state = M(r).clone(), _state(M)
    with pytest.raises(ValueError, match=rf"dense level 1 \({sizes[1]}\).*singular"):
        M.update(MM.csr_tensor(*N))
    assert M.updates == 0 and _state(M) == state and torch.equal(M(r), z0)
    M.update(MM.csr_tensor(D[0], D[1], 2.0 * D[2]))
    assert M.updates == 1 and torch.equal(M.levels[-1].csr.values(), 2.0 * torch.from_numpy(np.frombuffer(state[1][0]).copy()))


# -------------------------------------------------------------------------------------------------------------------- iterations
T_LIST = (0.05, 0.1, 0.2, 0.4, 0.7, 1.0)


def _iterations(A, M, maxiter=None):
    b = torch.ones(A.shape[0], dtype=torch.float64)
    x, info = cg(A, b, tol=1e-6, M=M, maxiter=maxiter)
    return get_last_stats().iterations, info


@pytest.mark.parametrize("K", [None, 256], ids=["coarse_rows_none", "coarse_rows_256"])
def test_a_refreshed_hierarchy_costs_at_most_three_iterations_and_a_stale_one_is_ruinous(K):
    A0 = MM.csr_tensor(*RM.t_family(64, 0.0))
    M, stale = P.from_graph(A0, coarse_rows=K), P.from_graph(A0, coarse_rows=K)
    for t in T_LIST:
        A = MM.csr_tensor(*RM.t_family(64, t))
        fresh, info_f = _iterations(A, P.from_graph(A, coarse_rows=K))
        refreshed, info_r = _iterations(A, M.update(A))
        print(f"coarse_rows {K}, t = {t}: built afresh {fresh}, refreshed {refreshed} iterations")
        assert info_f == 0 and info_r == 0
        assert refreshed <= fresh + 3, (t, fresh, refreshed)
        if t == 0.4:       # more than ten times the refreshed count: not converged after exactly ten times as many
            its, info = _iterations(A, stale, maxiter=10 * refreshed)
            print(f"coarse_rows {K}, t = {t}: the t = 0 object has not converged after {its} iterations (info {info})")
            assert its == 10 * refreshed and info != 0
    assert M.updates == len(T_LIST) and stale.updates == 0
