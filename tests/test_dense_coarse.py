"""AggregationMultigridPreconditioner.from_graph(coarse_rows=K) on CPU tensors (no GPU): the hierarchy above the cut is the default
one bit for bit, the dense last level holds the fp64 inverse rounded once in the column layout, the apply is tests/_mg_dense_mirror.py's
bit for bit (dense levels of 1, 2, 63, 64, 65 and 130 unknowns: below, at and above one segment of 64 columns, and three segments
with a ragged last one), the operator stays symmetric positive definite, the errors, and what the cut does to a stalled hierarchy
and to cg's count."""
import numpy as np
import pytest
import torch

import _mg_dense_mirror as DM
import _mg_graph_mirror as GM
import _mg_mirror as MM
from _order_cases import TRANSFORMS
from pytorch_sparse_solver.module_a import AggregationMultigridPreconditioner, cg, get_last_stats
from pytorch_sparse_solver.module_a import multigrid as MG
from pytorch_sparse_solver.utils.matrix_utils import create_poisson_2d_csr, create_variable_diffusion_2d_csr

P = AggregationMultigridPreconditioner


def _np(A):
    return A.crow_indices().numpy(), A.col_indices().numpy(), A.values().numpy()


def _matrices():
    yield "poisson9x7", _np(create_poisson_2d_csr(9, 7))                                        # 63
    yield "vardiff8x8", _np(create_variable_diffusion_2d_csr(8, 8))                             # 64
    yield "seven_point5x13x2", MM.grid_matrix((5, 13, 2))                                       # 130
    yield "poisson13x5_shuffled", GM.shuffled(*_np(create_poisson_2d_csr(13, 5)), seed=1)       # 65
    yield "poisson13x10_split", TRANSFORMS["dup"](*_np(create_poisson_2d_csr(13, 10)), seed=5)  # 130, a column stored twice
    yield "poisson8x8_zero", TRANSFORMS["zero"](*_np(create_poisson_2d_csr(8, 8)), seed=5)      # 64, stored zeros
    yield "two_blocks", GM.block_diagonal(_np(create_poisson_2d_csr(6, 5)), MM.grid_matrix((5, 7), seed=2))   # 65, ends at 2 unknowns
    yield "poisson37x29", _np(create_poisson_2d_csr(37, 29))
    yield "one_sided14x11", GM.one_sided(14, 11)


MATRICES = dict(_matrices())
# (matrix, coarse_rows, the unknowns of the dense level -- None: those of the first level of at most K, 0: no dense level, the
# default rule ends the hierarchy first)
APPLY_CASES = [("poisson9x7", 63, 63), ("poisson9x7", 1, 1), ("poisson9x7", 30, None),
               ("vardiff8x8", 64, 64), ("vardiff8x8", 20, None),
               ("seven_point5x13x2", 130, 130), ("seven_point5x13x2", 50, None),
               ("poisson13x5_shuffled", 65, 65), ("poisson13x5_shuffled", 1, 1),
               ("poisson13x10_split", 130, 130), ("poisson13x10_split", 40, None),
               ("poisson8x8_zero", 64, 64), ("poisson8x8_zero", 10, None),
               ("two_blocks", 65, 65), ("two_blocks", 2, 2), ("two_blocks", 1, 0)]
_default = {}


def _default_hierarchy(name, dtype=np.float64):
    """The default object of a matrix (no apply changes it), built once per (matrix, dtype) and shared."""
    key = (name, np.dtype(dtype).name)
    if key not in _default:
        crow, col, val = MATRICES[name]
        _default[key] = P.from_graph(MM.csr_tensor(crow, col, val.astype(dtype)), normalize=False)
    return _default[key]


def _same_level(a, b):
    assert a.n == b.n and a.dims == b.dims and a.max_row == b.max_row
    assert torch.equal(a.csr.crow_indices(), b.csr.crow_indices()) and torch.equal(a.csr.col_indices(), b.csr.col_indices())
    assert DM.same_bits(a.csr.values().numpy(), b.csr.values().numpy())
    assert (a.agg is None) == (b.agg is None) and (a.agg is None or torch.equal(a.agg, b.agg))


def _same_smoother(a, b):
    assert (a.c0, a.c1, a.c2) == (b.c0, b.c1, b.c2) and DM.same_bits(a.dinv.numpy(), b.dinv.numpy())


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("name", ["poisson37x29", "two_blocks", "one_sided14x11", "poisson13x10_split"])
def test_coarse_rows_none_is_the_default_object(name, dtype):
    crow, col, val = MATRICES[name]
    A = MM.csr_tensor(crow, col, val.astype(dtype))
    M0, M = P.from_graph(A, degree=2), P.from_graph(A, degree=2, coarse_rows=None)
    assert M.coarse_rows is None and M.dense is False and M0.dense is False and M.levels[-1].cinv is None
    assert len(M.levels) == len(M0.levels) and M.handshake_rounds == M0.handshake_rounds
    for a, b in zip(M.levels, M0.levels):
        _same_level(a, b)
        _same_smoother(a, b)
    assert (M.scale, M.tail_rows, M.tail_from, M.launches_per_apply) == (M0.scale, M0.tail_rows, M0.tail_from, M0.launches_per_apply)
    r = torch.from_numpy(np.random.default_rng(4).standard_normal(A.shape[0]).astype(dtype))
    assert DM.same_bits(M(r).numpy(), M0(r).numpy())
    G = P(MM.csr_tensor(*_np(create_poisson_2d_csr(8, 8))), (8, 8), normalize=False)          # the grid constructor has no cut
    assert G.coarse_rows is None and G.dense is False


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("name, K", [("poisson37x29", 1073), ("poisson37x29", 1072), ("poisson37x29", 100), ("poisson37x29", 7),
                                     ("poisson37x29", 1), ("one_sided14x11", 40), ("poisson13x10_split", 130), ("two_blocks", 2)])
def test_levels_above_the_cut_are_a_prefix_of_the_default_hierarchy(name, K, dtype):
    crow, col, val = MATRICES[name]
    M0 = _default_hierarchy(name, dtype)
    M = P.from_graph(MM.csr_tensor(crow, col, val.astype(dtype)), normalize=False, coarse_rows=K)
    L = len(M.levels) - 1
    assert M.coarse_rows == K and M.dense is True and L == next(l for l, lev in enumerate(M0.levels) if lev.n <= K)
    assert M.levels[L].n <= K and (L == 0 or M.levels[L - 1].n > K)
    assert M.handshake_rounds == M0.handshake_rounds[:L]
    for a, b in zip(M.levels[:L], M0.levels[:L]):
        _same_level(a, b)
        _same_smoother(a, b)
    last, ref = M.levels[L], M0.levels[L]
    assert last.agg is None and last.smoother is None and last.dinv is None and last.c0 is None and last.cinv is not None
    assert last.n == ref.n and torch.equal(last.csr.crow_indices(), ref.csr.crow_indices()) and \
        torch.equal(last.csr.col_indices(), ref.csr.col_indices()) and DM.same_bits(last.csr.values().numpy(), ref.csr.values().numpy())


def test_the_default_rule_still_ends_a_hierarchy_above_the_cut():
    """Two blocks end at two unknowns without a pair: with K = 1 that level is today's z = dinv r and nothing is dense."""
    crow, col, val = MATRICES["two_blocks"]
    M0 = _default_hierarchy("two_blocks")
    M = P.from_graph(MM.csr_tensor(crow, col, val), normalize=False, coarse_rows=1)
    assert M.coarse_rows == 1 and M.dense is False and M.levels[-1].cinv is None and M.levels[-1].n == 2
    assert len(M.levels) == len(M0.levels) and DM.same_bits(M.levels[-1].dinv.numpy(), M0.levels[-1].dinv.numpy())


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("name, K", [("poisson9x7", 63), ("poisson13x10_split", 130), ("poisson8x8_zero", 64), ("poisson37x29", 100),
                                     ("one_sided14x11", 154), ("poisson9x7", 1)])
def test_cinv_is_the_fp64_inverse_rounded_once_in_the_column_layout(name, K, dtype):
    crow, col, val = MATRICES[name]
    M = P.from_graph(MM.csr_tensor(crow, col, val.astype(dtype)), normalize=False, coarse_rows=K)
    lev = M.levels[-1]
    n, ld = lev.n, (lev.n + 3) & ~3
    c = lev.csr
    D = DM.dense_matrix(*_np(c))
    if len(M.levels) == 1 and name.endswith(("_split", "_zero")):
        assert c.values().numel() > np.count_nonzero(D)          # the split halves were added, the stored zero kept out of nothing
    ref = DM.stored_inverse(D)
    assert lev.ld == ld and lev.cinv.dtype == c.values().dtype and lev.cinv.is_contiguous() and tuple(lev.cinv.shape) == (n, ld)
    flat = lev.cinv.reshape(-1).numpy()
    assert DM.same_bits(flat, ref), f"{np.count_nonzero(DM.bits(flat) != DM.bits(ref))} of {n * ld} stored elements differ"
    assert not flat.reshape(n, ld)[:, n:].any(), "the padding is not zero"
    inv = torch.linalg.inv(torch.from_numpy(D.astype(np.float64))).to(lev.cinv.dtype).numpy()
    i, j = (n - 1, 0)
    assert DM.bits(flat[j * ld + i:j * ld + i + 1]) == DM.bits(inv[i:i + 1, j]) and DM.same_bits(DM.inverse_of(lev), inv)


def test_cinv_of_a_nonsymmetric_matrix_is_not_stored_transposed():
    crow, col, val = MATRICES["one_sided14x11"]
    n = 154
    M = P.from_graph(MM.csr_tensor(crow, col, val), normalize=False, coarse_rows=n)
    D = DM.dense_matrix(crow, col, val)
    assert len(M.levels) == 1 and not np.array_equal(D, D.T)
    ref = np.linalg.inv(D)
    cond = np.linalg.cond(D, 2)
    bound = 16 * n * np.finfo(np.float64).eps * cond
    C = DM.inverse_of(M.levels[-1])
    err = np.linalg.norm(C - ref, 2) / np.linalg.norm(ref, 2)
    err_t = np.linalg.norm(C.T - ref, 2) / np.linalg.norm(ref, 2)
    print(f"cond_2 {cond:.3e}, bound {bound:.3e}, relative error {err:.3e}, of the transpose {err_t:.3e}")
    assert err <= bound < err_t


def test_apply_cases_put_the_dense_level_at_every_size_of_interest():
    sizes = set()
    for name, K, n_dense in APPLY_CASES:
        crow, col, val = MATRICES[name]
        M = P.from_graph(MM.csr_tensor(crow, col, val), normalize=False, coarse_rows=K)
        assert M.dense == bool(n_dense != 0)
        if n_dense is not None and M.dense:
            assert M.levels[-1].n == n_dense
        if M.dense:
            assert M.levels[-1].n <= K and (len(M.levels) == 1 or M.levels[-2].n > K)
            sizes.add(M.levels[-1].n)
    assert {1, 2, 63, 64, 65, 130} <= sizes and any(2 < n < 63 for n in sizes), sorted(sizes)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("degree", [1, 3])
@pytest.mark.parametrize("name, K", [(c[0], c[1]) for c in APPLY_CASES])
def test_cpu_apply_has_the_mirrors_bits(oracle, name, K, degree, dtype):
    crow, col, val = MATRICES[name]
    A = MM.csr_tensor(crow, col, val.astype(dtype))
    M = P.from_graph(A, degree=degree, coarse_rows=K)
    assert M.scale != 1.0 and M.applies == 0
    r = np.random.default_rng([11, K]).standard_normal(A.shape[0]).astype(dtype)
    z = M(torch.from_numpy(r)).numpy()
    ref = DM.apply(oracle, M, r)
    assert M.applies == 1 and z.dtype == ref.dtype
    assert DM.same_bits(z, ref), f"{np.count_nonzero(DM.bits(z) != DM.bits(ref))} of {len(z)} entries differ"
    if M.dense:                                               # the dense step alone, unscaled
        C = DM.inverse_of(M.levels[-1])
        v = np.random.default_rng(12).standard_normal(C.shape[0]).astype(dtype)
        assert DM.same_bits(M._dense_torch(M.levels[-1], torch.from_numpy(v)).numpy(), DM.segmented(C, v))


def test_segmented_sum_is_the_spec_written_as_scalar_loops():
    """The mirror's numpy form against the spec's three loops element by element, -0 included (0 + -0 is +0)."""
    rng = np.random.default_rng(6)
    for n in (1, 63, 64, 65, 130):
        for dtype in (np.float64, np.float32):
            C, r = rng.standard_normal((n, n)).astype(dtype), rng.standard_normal(n).astype(dtype)
            C[0, :] = 0.0
            r[0] = -1.0                                       # row 0: every product is -0 or +0
            ref = np.empty(n, dtype=dtype)
            for i in range(n):
                s = dtype(0)
                for j0 in range(0, n, 64):
                    p = dtype(0)
                    for j in range(j0, min(j0 + 64, n)):
                        p = dtype(p + dtype(C[i, j] * r[j]))
                    s = dtype(s + p)
                ref[i] = s
            assert DM.same_bits(DM.segmented(C, r), ref) and not np.signbit(ref[0])


@pytest.mark.parametrize("K", [221, 64, 1])
def test_operator_is_symmetric_positive_definite(K):
    A = create_poisson_2d_csr(17, 13)
    M = P.from_graph(A, coarse_rows=K)
    assert M.dense
    D = torch.stack([M(e) for e in torch.eye(17 * 13, dtype=torch.float64)], 1)
    asym = float((D - D.T).abs().max() / D.abs().max())
    print(f"coarse_rows {K}: levels {[lev.n for lev in M.levels]}, relative asymmetry {asym:.3e}")
    assert asym < 1e-12
    assert float(torch.linalg.eigvalsh((D + D.T) / 2).min()) > 0.0


def test_one_dense_level_solves_in_at_most_two_iterations():
    A = create_poisson_2d_csr(24, 20)
    b = torch.ones(480, dtype=torch.float64)
    for K in (480, 2048):
        M = P.from_graph(A, coarse_rows=K)
        assert len(M.levels) == 1 and M.dense and M.tail_from == 0 and M.launches_per_apply == 1
        x, info = cg(A, b, tol=1e-6, M=M)
        its = get_last_stats().iterations
        relres = float(torch.linalg.vector_norm(b - A @ x) / torch.linalg.vector_norm(b))
        print(f"coarse_rows {K}: {its} iterations, relative residual {relres:.3e}")
        assert info == 0 and relres <= 1e-6 and its <= 2


def test_errors():
    A = create_poisson_2d_csr(6, 5)
    for K in (0, -1, 2049, True, False, 16.0, 2.5, "16", np.float64(16.0), np.bool_(True)):
        with pytest.raises(ValueError, match="coarse_rows"):
            P.from_graph(A, coarse_rows=K)
    assert MG.MG_DENSE_MAX_ROWS == 2048 and MG.MG_DENSE_TAIL_ROWS == 512
    assert P.from_graph(A, coarse_rows=np.int64(30)).coarse_rows == 30 and P.from_graph(A, coarse_rows=2048).dense
    with pytest.raises(TypeError):
        P(A, (6, 5), coarse_rows=16)                             # the grid constructor has no such argument
    # a singular coarse matrix: the Neumann Laplacian of a path (row sums exactly 0), and a level that is singular outright
    n = 8
    rows = [[(i, 1.0 if i in (0, n - 1) else 2.0)] + [(j, -1.0) for j in (i - 1, i + 1) if 0 <= j < n] for i in range(n)]
    crow = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    col, val = np.array([c for r in rows for c, _ in r]), np.array([v for r in rows for _, v in r])
    sizes = [len(lev[0]) - 1 for lev in GM.hierarchy(crow, col, val)]
    with pytest.raises(ValueError, match=rf"dense level 1 \({sizes[1]}\).*singular"):
        P.from_graph(MM.csr_tensor(crow, col, val), coarse_rows=sizes[1])
    with pytest.raises(ValueError, match=r"dense level 0 \(2\).*singular"):
        P.from_graph(MM.csr_tensor(np.array([0, 2, 4]), np.array([0, 1, 0, 1]), np.array([1.0, 1.0, 1.0, 1.0])), coarse_rows=2)


def test_a_star_graph_that_stalls_builds_with_a_cut():
    crow, col, val = GM.star(100)
    A = MM.csr_tensor(crow, col, val)
    with pytest.raises(ValueError, match=r"stalled.*48"):
        P.from_graph(A)
    with pytest.raises(ValueError, match=r"stalled.*48"):
        P.from_graph(A, coarse_rows=None)
    M = P.from_graph(A, coarse_rows=16)
    sizes = [lev.n for lev in M.levels]
    assert M.dense and sizes[0] == 101 and sizes[-1] <= 16 < sizes[-2] and len(sizes) <= MG.MG_GRAPH_MAX_LEVELS
    b = torch.ones(101, dtype=torch.float64)
    x, info = cg(A, b, tol=1e-8, M=M)
    assert info == 0 and float(torch.linalg.vector_norm(b - A @ x) / torch.linalg.vector_norm(b)) <= 1e-8
    with pytest.raises(ValueError, match=r"stalled.*48"):          # a cut too low to be reached within 48 levels changes nothing
        P.from_graph(MM.csr_tensor(*GM.star(200)), coarse_rows=16)


def test_tail_from_and_launch_count_with_a_dense_level():
    """The tail takes the dense level when tail_rows selects one and the level has at most 512 rows; the formula is unchanged."""
    A = create_poisson_2d_csr(64, 64)
    sizes = [lev.n for lev in P.from_graph(A, normalize=False).levels]
    assert sizes[:4] == [4096, 1241, 394, 137]
    for K, tail_rows, levels, tail_from in [(137, 1024, 4, 2), (394, 1024, 3, 2), (394, 256, 3, None), (394, 0, 3, None),
                                            (1241, 4096, 2, None), (1241, 1024, 2, None), (2048, 4096, 2, None), (137, 4096, 4, 0),
                                            (137, 137, 4, 3), (137, 100, 4, None)]:
        M = P.from_graph(A, degree=2, normalize=False, tail_rows=tail_rows, coarse_rows=K)
        assert [lev.n for lev in M.levels] == sizes[:levels] and M.dense
        assert M.tail_from == tail_from, (K, tail_rows, M.tail_from)
        assert M.launches_per_apply == (levels - 1 if tail_from is None else tail_from) * (2 * 2 + 7) + 1


def test_cg_on_poisson_128_needs_no_more_applies_with_a_dense_level():
    """A prototype had 21 applies with coarse_rows=1024 against the default's 25."""
    A = create_poisson_2d_csr(128, 128)
    b = torch.ones(128 * 128, dtype=torch.float64)
    counts = {}
    for K in (None, 1024):
        M = P.from_graph(A, coarse_rows=K)
        x, info = cg(A, b, tol=1e-6, M=M)
        relres = float(torch.linalg.vector_norm(b - A @ x) / torch.linalg.vector_norm(b))
        counts[K] = M.applies
        print(f"coarse_rows {K}: {len(M.levels)} levels, {M.applies} applies, relative residual {relres:.3e}")
        assert info == 0 and relres <= 1e-6
    assert counts[1024] <= counts[None]
