"""`AggregationMultigridPreconditioner(cycle="W")` on the CPU (module_a/multigrid.py), against tests/_mg_w_mirror.py:

1. cycle="V" is the object built without the keyword, bit for bit;
2. the CPU apply of cycle="W" is the mirror's recursion bitwise on a grid, a graph and a dense-cut hierarchy, both dtypes, degree 1
   and 2, scaled and unscaled; on a shuffled and a split-entry matrix; on a two-level hierarchy (W is V bit for bit: the only coarse
   level is the last) and on a one-level one;
3. M is symmetric and positive definite at omega = 1.8 (assembled from unit vectors);
4. iteration counts of cg on Poisson 48^2 and 96^2: W at most 11 and 12 from `from_graph(coarse_rows=64)` and fewer than V, at
   most 8 from the grid class;
5. `update` on a W object is a freshly built W object; the errors of the keyword; `launches_per_apply` is the docstring's closed
   form and the count of a walk."""
import numpy as np
import pytest
import torch

import _mg_graph_mirror as GM
import _mg_mirror as MM
import _mg_w_mirror as WM
from _order_cases import TRANSFORMS
from pytorch_sparse_solver.module_a import AggregationMultigridPreconditioner as P
from pytorch_sparse_solver.module_a import cg, get_last_stats
from pytorch_sparse_solver.utils.matrix_utils import create_poisson_2d_csr, create_variable_diffusion_2d_csr

DTYPES = [np.float64, np.float32]


def _np(A):
    return A.crow_indices().numpy(), A.col_indices().numpy(), A.values().numpy()


# kind -> (the matrix in fp64, the constructor)
KINDS = {
    "grid": (lambda: _np(create_poisson_2d_csr(17, 13)), lambda A, **kw: P(A, (17, 13), **kw)),
    "graph": (lambda: _np(create_variable_diffusion_2d_csr(32, 32)), lambda A, **kw: P.from_graph(A, **kw)),
    "dense": (lambda: _np(create_poisson_2d_csr(48, 48)), lambda A, **kw: P.from_graph(A, coarse_rows=64, **kw)),
}
_arrays = {}


def _matrix(kind, dtype, transform=None):
    key = (kind, np.dtype(dtype).name, transform)
    if key not in _arrays:
        crow, col, val = KINDS[kind][0]()
        if transform is not None:
            crow, col, val = TRANSFORMS[transform](np.asarray(crow, dtype=np.int64), np.asarray(col, dtype=np.int64), val, seed=5)
        _arrays[key] = MM.csr_tensor(crow, col, np.asarray(val).astype(dtype))
    return _arrays[key]


def _state(M):
    out = {"scale": M.scale, "tail": (M.tail_rows, M.tail_from, M.launches_per_apply), "n": [lev.n for lev in M.levels]}
    for l, lev in enumerate(M.levels):
        out[l] = (lev.csr.values().numpy().tobytes(), None if lev.dinv is None else lev.dinv.numpy().tobytes(), lev.c0,
                  None if lev.c1 is None else tuple(lev.c1), None if lev.c2 is None else tuple(lev.c2),
                  None if lev.cinv is None else lev.cinv.numpy().tobytes(), None if lev.agg is None else lev.agg.numpy().tobytes())
    return out


def _rhs(n, dtype, seed=5):
    return np.random.default_rng([seed, n]).standard_normal(n).astype(dtype)


# ------------------------------------------------------------------------------------------------------------ 1. cycle="V"
@pytest.mark.parametrize("kind", list(KINDS))
def test_cycle_v_is_the_object_without_the_keyword(kind):
    A = _matrix(kind, np.float64)
    M0, M1 = KINDS[kind][1](A), KINDS[kind][1](A, cycle="V")
    assert M0.cycle == M1.cycle == "V" and _state(M0) == _state(M1)
    r = torch.from_numpy(_rhs(A.shape[0], np.float64))
    assert MM.same_bits(M0(r).numpy(), M1(r).numpy())


# ------------------------------------------------------------------------------------------------------------ 2. the W apply
@pytest.mark.parametrize("normalize", [True, False], ids=["scaled", "unscaled"])
@pytest.mark.parametrize("degree", [1, 2])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_w_apply_is_the_mirror(oracle, kind, dtype, degree, normalize):
    A = _matrix(kind, dtype)
    M = KINDS[kind][1](A, degree=degree, normalize=normalize, cycle="W")
    assert M.cycle == "W" and len(M.levels) >= 4 and (M.scale != 1.0) == normalize
    r = _rhs(A.shape[0], dtype)
    mirror = WM.Mirror(oracle, M)
    ref = mirror(r)
    last = len(M.levels) - 1
    assert mirror.visits == [2 ** min(l, last - 1) for l in range(last + 1)]
    z = M(torch.from_numpy(r)).numpy()
    assert MM.same_bits(z, ref), f"{np.count_nonzero(MM.bits(z) != MM.bits(ref))} of {r.size} entries differ from the mirror"
    assert not MM.same_bits(ref, WM.apply(oracle, M, r, cycle="V")), "the W-cycle of the mirror is its V-cycle"


@pytest.mark.parametrize("transform", ["shuf", "dup"], ids=["shuffled", "split"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_w_apply_is_the_mirror_on_unsorted_and_split_rows(oracle, kind, transform):
    A = _matrix(kind, np.float64, transform)
    M = KINDS[kind][1](A, degree=2, cycle="W")
    r = _rhs(A.shape[0], np.float64, seed=6)
    assert MM.same_bits(M(torch.from_numpy(r)).numpy(), WM.apply(oracle, M, r))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
def test_two_levels_and_one_level_are_the_v_cycle(oracle, dtype):
    cases = [(lambda A, **kw: P(A, (2, 1), **kw), MM.grid_matrix((2, 1), dtype=dtype), 2),
             (lambda A, **kw: P.from_graph(A, coarse_rows=64, **kw), GM.stencil5(12, 12, dtype=dtype), 2),
             (lambda A, **kw: P(A, (1, 1), **kw), MM.grid_matrix((1, 1), dtype=dtype), 1),
             (lambda A, **kw: P.from_graph(A, coarse_rows=64, **kw), GM.stencil5(6, 6, dtype=dtype), 1)]
    for build, arrs, nlev in cases:
        A = MM.csr_tensor(*arrs)
        V, W = build(A, cycle="V"), build(A, cycle="W")
        assert len(W.levels) == nlev and W.scale == V.scale and W.launches_per_apply == V.launches_per_apply
        r = _rhs(A.shape[0], dtype)
        z = W(torch.from_numpy(r)).numpy()
        assert MM.same_bits(z, V(torch.from_numpy(r)).numpy()) and MM.same_bits(z, WM.apply(oracle, W, r))


# ------------------------------------------------------------------------------------------------------------ 3. M is SPD
@pytest.mark.parametrize("kind", ["grid", "graph"])
def test_w_operator_is_symmetric_positive_definite_at_omega_1_8(kind):
    A = create_poisson_2d_csr(12, 12)
    M = P(A, (12, 12), omega=1.8, cycle="W") if kind == "grid" else P.from_graph(A, omega=1.8, cycle="W")
    assert M.omega == 1.8 and len(M.levels) >= 3
    n = A.shape[0]
    eye = torch.eye(n, dtype=torch.float64)
    Mm = torch.stack([M(eye[i]) for i in range(n)], dim=1).numpy()
    asym = np.abs(Mm - Mm.T).max() / np.abs(Mm).max()
    low = np.linalg.eigvalsh((Mm + Mm.T) / 2).min()
    print(f"{kind}: asymmetry {asym:.3e} relative, smallest eigenvalue {low:.6e}")
    assert asym <= 1e-12
    assert low > 0.0


# ------------------------------------------------------------------------------------------------------------ 4. iteration counts
def _iterations(A, M):
    b = torch.ones(A.shape[0], dtype=torch.float64)
    x, info = cg(A, b, tol=1e-6, M=M)
    assert info == 0
    return get_last_stats().iterations


@pytest.mark.parametrize("n, most", [(48, 11), (96, 12)])      # 192^2 (at most 13) takes 12 s on a CPU: left out
def test_w_iteration_counts_on_poisson(n, most):
    A = create_poisson_2d_csr(n, n)
    w = _iterations(A, P.from_graph(A, coarse_rows=64, cycle="W"))
    v = _iterations(A, P.from_graph(A, coarse_rows=64))
    g = _iterations(A, P(A, (n, n), cycle="W"))
    print(f"Poisson {n}^2: from_graph(coarse_rows=64) W {w}, V {v}; grid W {g}")
    assert w <= most and w < v and g <= 8


# ------------------------------------------------------------------------------------------------------------ 5. update, errors, launches
@pytest.mark.parametrize("kind", ["grid", "graph", "dense"])
def test_update_keeps_the_cycle_and_equals_a_fresh_w_object(kind):
    grid = (9, 7, 5)
    first, other = MM.grid_matrix(grid), MM.grid_matrix(grid, seed=3)
    build = {"grid": lambda A: P(A, grid, cycle="W"), "graph": lambda A: P.from_graph(A, cycle="W"),
             "dense": lambda A: P.from_graph(A, coarse_rows=64, cycle="W")}[kind]
    A = MM.csr_tensor(*first)
    # the aggregates held fixed: a grid's are its boxes whatever the values; a graph's are those of a multiple of the matrix
    B = MM.csr_tensor(*other) if kind == "grid" else MM.csr_tensor(first[0], first[1], first[2] * 4.0)
    M = build(A)
    r = torch.from_numpy(_rhs(A.shape[0], np.float64))
    M(r)
    assert M.update(B) is M and M.cycle == "W" and M.updates == 1 and M.applies == 0
    fresh = build(B)
    assert _state(M) == _state(fresh)
    assert MM.same_bits(M(r).numpy(), fresh(r).numpy())
    if kind == "grid":                # (a multiple by a power of two gives the normalised operator of the first matrix again)
        assert not MM.same_bits(M(r).numpy(), build(A)(r).numpy())


@pytest.mark.parametrize("bad", ["X", None, "w", 2, ["W"]], ids=repr)
def test_cycle_errors(bad):
    A = create_poisson_2d_csr(8, 8)
    with pytest.raises(ValueError, match="cycle must be") as e:
        P(A, (8, 8), cycle=bad)
    assert repr(bad) in str(e.value)
    with pytest.raises(ValueError, match="cycle must be") as e:
        P.from_graph(A, cycle=bad)
    assert repr(bad) in str(e.value)


def _closed_form(M):
    k, L = 2 * M.degree + 7, len(M.levels) - 1
    T = L if M.tail_from is None else M.tail_from
    end = 1 if T == 0 else (2 ** (T - 1) if T == L else 2 ** T + 2 ** T)
    return (2 ** T - 1) * k + max(2 ** T - 2, 0) + end


@pytest.mark.parametrize("name", ["grid_tail0", "grid_tail64", "graph_tail256", "dense_no_tail", "one_launch"])
def test_launches_per_apply_is_the_closed_form_and_the_walks_count(name):
    A = create_poisson_2d_csr(48, 48)
    M = {"grid_tail0": lambda: P(A, (48, 48), degree=2, tail_rows=0, normalize=False, cycle="W"),
         "grid_tail64": lambda: P(A, (48, 48), tail_rows=64, normalize=False, cycle="W"),
         "graph_tail256": lambda: P.from_graph(A, tail_rows=256, normalize=False, cycle="W"),
         "dense_no_tail": lambda: P.from_graph(A, coarse_rows=64, tail_rows=0, degree=3, normalize=False, cycle="W"),
         "one_launch": lambda: P.from_graph(A, coarse_rows=64, tail_rows=4096, normalize=False, cycle="W")}[name]()
    print(name, [lev.n for lev in M.levels], M.tail_from, M.launches_per_apply)
    assert M.launches_per_apply == _closed_form(M) == WM.launches(M)
    if name == "grid_tail0":          # 48, 24, 12, 6, 3, 2, 1 points per side: levels 0 .. 6, k = 11
        assert M.tail_from is None and M.launches_per_apply == 63 * 11 + 62 + 32
    if name == "grid_tail64":         # the tail from level 3 (36 unknowns) on, k = 9
        assert M.tail_from == 3 and M.launches_per_apply == 7 * 9 + 6 + 16
    if name == "one_launch":
        assert M.tail_from == 0 and M.launches_per_apply == 1


def test_more_than_twelve_small_levels_stay_launches_and_more_than_sixteen_are_refused(oracle):
    """The W tails take at most 12 levels: a deeper run of small levels is left to the launch sequence, where V takes the tail.  A
    star loses one pair per matching pass: 13 levels from 13 rows, 29 from 29 -- where level 27 would be visited 2^27 times, so a W
    hierarchy of more than 16 levels is a ValueError."""
    A = MM.csr_tensor(*GM.star(12))
    V = P.from_graph(A, passes=1, tail_rows=4096, normalize=False)
    W = P.from_graph(A, passes=1, tail_rows=4096, normalize=False, cycle="W")
    assert len(V.levels) == len(W.levels) == 13 and V.tail_from == 0 and W.tail_from is None
    assert W.launches_per_apply == _closed_form(W) == WM.launches(W) == 4095 * 9 + 4094 + 2048
    r = _rhs(13, np.float64)
    assert MM.same_bits(W(torch.from_numpy(r)).numpy(), WM.apply(oracle, W, r))
    B = MM.csr_tensor(*GM.star(28))
    assert len(P.from_graph(B, passes=1, normalize=False).levels) == 29
    with pytest.raises(ValueError, match='cycle="W" takes at most 16 levels.*coarse_rows'):
        P.from_graph(B, passes=1, normalize=False, cycle="W")
    C = create_variable_diffusion_2d_csr(64, 64)
    W = P.from_graph(C, tail_rows=4096, normalize=False, cycle="W")
    assert len(W.levels) == 12 and W.tail_from == 0 and W.launches_per_apply == 1
