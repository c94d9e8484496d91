"""AggregationMultigridPreconditioner.from_graph and pairwise_aggregates on CPU tensors (no GPU): the aggregates, the level sizes and
the Galerkin coarse matrices bit for bit against tests/_mg_graph_mirror.py (whose matching is the sequential greedy walk), the apply
bit for bit against the mirror's V-cycle, symmetry and definiteness of the operator, the errors, and what it does to cg's
iteration count -- on a shuffled matrix, where the grid class cannot be built, and on an anisotropic one, where it degrades."""
import numpy as np
import pytest
import torch

import _mg_graph_mirror as GM
import _mg_mirror as MM
from _order_cases import TRANSFORMS
from pytorch_sparse_solver.module_a import AggregationMultigridPreconditioner, ChebyshevPreconditioner, cg, get_last_stats, pairwise_aggregates
from pytorch_sparse_solver.module_a import multigrid as MG
from pytorch_sparse_solver.utils.matrix_utils import create_poisson_2d_csr, create_variable_diffusion_2d_csr

P = AggregationMultigridPreconditioner


def _np(A):
    return A.crow_indices().numpy(), A.col_indices().numpy(), A.values().numpy()


def _matrices():
    p = _np(create_poisson_2d_csr(17, 13))
    yield "poisson17x13", p
    yield "poisson37x29", _np(create_poisson_2d_csr(37, 29))
    yield "vardiff30x26", _np(create_variable_diffusion_2d_csr(30, 26))
    yield "seven_point9x7x5", MM.grid_matrix((9, 7, 5))
    yield "poisson24x24_shuffled", GM.shuffled(*_np(create_poisson_2d_csr(24, 24)), seed=1)
    yield "poisson17x13_split", TRANSFORMS["dup"](*p, seed=5)
    yield "poisson17x13_zero", TRANSFORMS["zero"](*p, seed=5)
    yield "poisson17x13_rev", TRANSFORMS["rev"](*p, seed=5)
    yield "one_sided14x11", GM.one_sided(14, 11)
    yield "diagonal9", (np.arange(10, dtype=np.int64), np.arange(9, dtype=np.int64), np.linspace(1.0, 3.0, 9))
    yield "two_blocks", GM.block_diagonal(_np(create_poisson_2d_csr(7, 5)), MM.grid_matrix((1, 6), seed=2))
    yield "one_row", (np.array([0, 1]), np.array([0]), np.array([2.5]))


MATRICES = dict(_matrices())
LAST_LEVEL = {"diagonal9": 9, "two_blocks": 2}
_mirror_levels = {}


def _mirror_hierarchy(name, dtype):
    """The mirror's levels of a matrix, computed once per (matrix, dtype) and shared."""
    if (name, dtype) not in _mirror_levels:
        crow, col, val = MATRICES[name]
        _mirror_levels[name, dtype] = GM.hierarchy(crow, col, val.astype(dtype))
    return _mirror_levels[name, dtype]


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("name", sorted(MATRICES))
def test_hierarchy_has_the_mirrors_bits(name, dtype):
    crow, col, val = MATRICES[name]
    M = P.from_graph(MM.csr_tensor(crow, col, val.astype(dtype)), normalize=False)
    ref = _mirror_hierarchy(name, dtype)
    assert [lev.n for lev in M.levels] == [len(r[0]) - 1 for r in ref]
    assert M.levels[-1].n == LAST_LEVEL.get(name, 1) and M.levels[-1].agg is None and M.levels[-1].c0 is None
    assert (len(M.levels) == 1) == (name in ("diagonal9", "one_row"))
    for l, (lev, (rc, cc, vc, agg)) in enumerate(zip(M.levels, ref)):
        got = _np(lev.csr)
        assert lev.dims == (lev.n,) and lev.csr.values().dtype == torch.from_numpy(val.astype(dtype)).dtype
        assert np.array_equal(got[0], rc) and np.array_equal(got[1], cc), (name, l)
        assert GM.same_bits(got[2], vc), (name, l)
        if agg is None:
            assert l == len(M.levels) - 1
            diag = np.array([vc[k] for i in range(lev.n) for k in range(rc[i], rc[i + 1]) if cc[k] == i])   # stored once: coalesced
            assert len(diag) == lev.n and GM.same_bits(lev.dinv.numpy(), dtype(1.0) / diag)
            continue
        assert lev.agg.dtype == torch.int64 and np.array_equal(lev.agg.numpy(), agg), (name, l)
        sizes = np.bincount(agg)
        assert sizes.min() >= 1 and sizes.max() <= 4 and len(sizes) == M.levels[l + 1].n
        first = np.array([m[0] for m in GM.member_lists(agg, len(sizes))])
        assert np.all(np.diff(first) > 0), "aggregates are not numbered by their smallest member"
        if l:
            rows = np.repeat(np.arange(lev.n), np.diff(rc))
            assert np.all(np.diff(cc)[np.diff(rows) == 0] > 0), "a coarse row is not strictly ascending"
        ref_s = ChebyshevPreconditioner(lev.csr, degree=1, ratio=4.0, normalize=False)
        assert (lev.c0, lev.c1, lev.c2) == (ref_s.c0, ref_s.c1, ref_s.c2) and torch.equal(lev.dinv, ref_s.dinv)


@pytest.mark.parametrize("passes", [1, 2, 3])
@pytest.mark.parametrize("name", ["poisson17x13", "vardiff30x26", "poisson24x24_shuffled", "one_sided14x11", "poisson17x13_split"])
def test_pairwise_aggregates_is_the_greedy_matching_with_at_most_2_to_the_passes_members(name, passes):
    crow, col, val = MATRICES[name]
    for theta in (0.25, 0.0, 1.0):
        agg, nc = pairwise_aggregates(MM.csr_tensor(crow, col, val), passes=passes, theta=theta)
        ref, ref_nc = GM.pairwise_aggregates(crow, col, val, passes, theta)
        assert agg.dtype == torch.int64 and nc == ref_nc and np.array_equal(agg.numpy(), ref), (name, passes, theta)
        sizes = np.bincount(ref, minlength=nc)
        assert sizes.min() >= 1 and sizes.max() <= 2 ** passes
        assert nc < len(ref)


def test_a_pass_pairs_only_strong_neighbours_and_weights_take_the_larger_direction():
    """Path 0 - 1 - 2 - 3 with couplings 1, 0.1, 1: at theta = 0.25 the middle edge is weak, so {0, 1}, {2, 3} whatever the hash says;
    with the strong couplings stored in ONE direction only the result is the same."""
    for one_sided in (False, True):
        rows = [[(0, 2.0), (1, -1.0)], [(0, -1.0), (1, 2.0), (2, -0.1)], [(1, -0.1), (2, 2.0), (3, -1.0)], [(2, -1.0), (3, 2.0)]]
        if one_sided:
            rows[0] = [(0, 2.0)]
            rows[3] = [(3, 2.0)]
        crow = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
        col, val = np.array([c for r in rows for c, _ in r]), np.array([v for r in rows for _, v in r])
        agg, nc = pairwise_aggregates(MM.csr_tensor(crow, col, val), passes=1)
        assert agg.tolist() == [0, 0, 1, 1] and nc == 2
        agg, nc = pairwise_aggregates(MM.csr_tensor(crow, col, val), passes=1, theta=0.0)     # every edge strong: the hash decides
        assert np.array_equal(agg.numpy(), GM.pairwise_aggregates(crow, col, val, 1, 0.0)[0])


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("degree", [1, 2, 3])
@pytest.mark.parametrize("normalize", [True, False], ids=["normalized", "unscaled"])
@pytest.mark.parametrize("name", ["vardiff30x26", "seven_point9x7x5", "poisson24x24_shuffled", "two_blocks"])
def test_cpu_apply_has_the_mirrors_bits(oracle, name, normalize, degree, dtype):
    crow, col, val = MATRICES[name]
    A = MM.csr_tensor(crow, col, val.astype(dtype))
    M = P.from_graph(A, degree=degree, normalize=normalize)
    assert (M.scale != 1.0) == normalize and M.applies == 0
    r = np.random.default_rng(11).standard_normal(A.shape[0]).astype(dtype)
    z = M(torch.from_numpy(r)).numpy()
    ref = GM.apply(oracle, M, r)
    assert M.applies == 1
    assert GM.same_bits(z, ref), f"{np.count_nonzero(GM.bits(z) != GM.bits(ref))} entries differ"


def test_single_level_hierarchies_apply_the_reciprocal_diagonal(oracle):
    for name in ("diagonal9", "one_row"):
        crow, col, val = MATRICES[name]
        M = P.from_graph(MM.csr_tensor(crow, col, val), normalize=False)
        r = np.random.default_rng(3).standard_normal(len(val))
        assert GM.same_bits(M(torch.from_numpy(r)).numpy(), (1.0 / val) * r) and M.launches_per_apply == 1 and M.tail_from == 0


def test_operator_is_symmetric_positive_definite():
    crow, col, val = MATRICES["poisson17x13"]
    M = P.from_graph(MM.csr_tensor(crow, col, val))
    D = torch.stack([M(e) for e in torch.eye(17 * 13, dtype=torch.float64)], 1)
    asym = float((D - D.T).abs().max() / D.abs().max())
    print(f"relative asymmetry {asym:.3e}")
    assert asym < 1e-12
    assert float(torch.linalg.eigvalsh((D + D.T) / 2).min()) > 0.0


def test_errors():
    A = create_poisson_2d_csr(6, 5)
    for passes in (0, 5):
        with pytest.raises(ValueError, match="passes"):
            P.from_graph(A, passes=passes)
        with pytest.raises(ValueError, match="passes"):
            pairwise_aggregates(A, passes=passes)
    for theta in (-0.01, 1.01, float("nan")):
        with pytest.raises(ValueError, match="theta"):
            P.from_graph(A, theta=theta)
        with pytest.raises(ValueError, match="theta"):
            pairwise_aggregates(A, theta=theta)
    with pytest.raises(ValueError, match="degree"):
        P.from_graph(A, degree=0)
    with pytest.raises(ValueError, match="omega"):
        P.from_graph(A, omega=0.0)
    with pytest.raises(ValueError, match="tail_rows"):
        P.from_graph(A, tail_rows=-1)
    with pytest.raises(ValueError, match="square"):
        P.from_graph(torch.zeros(30, 29, dtype=torch.float64))
    with pytest.raises(ValueError, match="float"):
        P.from_graph(torch.eye(30, dtype=torch.int64))

    class FakeRowBlock:
        _hipk_row_block = True
    with pytest.raises(ValueError, match="RowBlockCSR"):
        P.from_graph(FakeRowBlock())
    M = P.from_graph(A)
    for v in (torch.ones(29, dtype=torch.float64), torch.ones(30, 1, dtype=torch.float64), torch.ones(30, dtype=torch.float32),
              torch.ones(30, dtype=torch.float64, device="meta"), np.ones(30)):
        with pytest.raises(ValueError, match="applied to"):
            M(v)
    assert M.applies == 0


def test_a_star_graph_stalls_and_is_refused():
    crow, col, val = GM.star(200)
    agg, nc = pairwise_aggregates(MM.csr_tensor(crow, col, val))
    assert nc == 199 and np.bincount(agg.numpy()).max() == 3          # the centre and one leaf per pass
    with pytest.raises(ValueError, match=r"stalled.*48"):
        P.from_graph(MM.csr_tensor(crow, col, val))
    assert MG.MG_GRAPH_MAX_LEVELS == 48
    assert len(P.from_graph(MM.csr_tensor(*GM.star(60)), normalize=False).levels) == 31


def test_non_positive_diagonal_names_the_level():
    crow, col, val = (a.copy() for a in MATRICES["poisson17x13"])
    val[(col == 5) & (np.repeat(np.arange(221), np.diff(crow)) == 5)] = -4.0
    with pytest.raises(ValueError, match=r"level 0 \(221\).*diagonal"):
        P.from_graph(MM.csr_tensor(crow, col, val))
    # the Neumann Laplacian of a path (row sums exactly 0): every Galerkin level keeps the row sums, the last level is the stored 0
    n = 8
    rows = [[(i, 1.0 if i in (0, n - 1) else 2.0)] + [(j, -1.0) for j in (i - 1, i + 1) if 0 <= j < n] for i in range(n)]
    crow = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    col, val = np.array([c for r in rows for c, _ in r]), np.array([v for r in rows for _, v in r])
    levels = len(GM.hierarchy(crow, col, val))
    with pytest.raises(ValueError, match=rf"level {levels - 1} \(1\).*diagonal"):
        P.from_graph(MM.csr_tensor(crow, col, val))


def test_tail_from_and_launch_count_follow_the_level_list():
    A = create_poisson_2d_csr(64, 64)
    sizes = [lev.n for lev in P.from_graph(A, normalize=False).levels]
    assert sizes[:4] == [4096, 1241, 394, 137]
    for tail_rows in (0, 1, 256, 1024, 4096, 100000):
        M = P.from_graph(A, degree=2, normalize=False, tail_rows=tail_rows)
        tail_from = next((l for l, n in enumerate(sizes) if n <= min(tail_rows, 4096)), None)
        assert M.tail_from == tail_from and M.tail_rows == min(tail_rows, 4096)
        assert M.launches_per_apply == (len(sizes) - 1 if tail_from is None else tail_from) * (2 * 2 + 7) + 1
    assert P.from_graph(A, normalize=False).tail_rows == MG.MG_TAIL_MAX_ROWS
    G = P(A, (64, 64), normalize=False)                                # the grid constructor is what it was
    assert all(lev.agg is None for lev in G.levels) and G.levels[0].dims == (64, 64) and not G.graph


def _iterations(A, M=None):
    b = torch.ones(A.shape[0], dtype=torch.float64)
    x, info = cg(A, b, tol=1e-6, M=M)
    relres = float(torch.linalg.vector_norm(b - A @ x) / torch.linalg.vector_norm(b))
    return get_last_stats().iterations, info, relres


@pytest.mark.parametrize("name, make, divisor", [
    ("poisson64", lambda: create_poisson_2d_csr(64, 64), 4),
    ("poisson128", lambda: create_poisson_2d_csr(128, 128), 6),
    ("poisson64_shuffled", lambda: MM.csr_tensor(*GM.shuffled(*_np(create_poisson_2d_csr(64, 64)), seed=1)), 4),
])
def test_cg_takes_a_fraction_of_the_iterations(name, make, divisor):
    """The conditions of the issue: a quarter of plain cg's iterations at 64 x 64 (a prototype had 17 against 101; 18 on the shuffled
    matrix), a sixth at 128 x 128 (23 against 204)."""
    A = make()
    plain, info0, _ = _iterations(A)
    its, info, relres = _iterations(A, P.from_graph(A))
    print(f"{name}: plain {plain}, graph multigrid {its}, relative residual {relres:.3e}")
    assert info0 == 0 and info == 0 and relres <= 1e-6
    assert divisor * its <= plain


def test_anisotropic_matrix_needs_fewer_iterations_than_the_grid_class():
    """y-coupling x 0.01 at 64 x 64: the 2 x 2 boxes aggregate across the weak direction, the matching does not (a prototype had 22
    against 39, plain cg 281)."""
    A = MM.csr_tensor(*GM.anisotropic(64, 64, 0.01))
    plain, _, _ = _iterations(A)
    grid, info_g, _ = _iterations(A, P(A, (64, 64)))
    graph, info, relres = _iterations(A, P.from_graph(A))
    print(f"anisotropic 64 x 64: plain {plain}, grid {grid}, graph {graph}, relative residual {relres:.3e}")
    assert info == 0 and info_g == 0 and relres <= 1e-6
    assert graph < grid
