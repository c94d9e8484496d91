"""AggregationMultigridPreconditioner on CPU tensors (no GPU): the level dimensions, the Galerkin coarse matrices and the apply bit for
bit against tests/_mg_mirror.py, symmetry and definiteness of the operator, the errors, and what it does to cg's iteration count."""
import numpy as np
import pytest
import torch

import _mg_mirror as MM
from _order_cases import TRANSFORMS
from pytorch_sparse_solver.module_a import AggregationMultigridPreconditioner, ChebyshevPreconditioner, cg, get_last_stats
from pytorch_sparse_solver.module_a import multigrid as MG
from pytorch_sparse_solver.utils.matrix_utils import (create_ldc_pressure_csr, create_poisson_2d_csr,
                                                      create_variable_diffusion_2d_csr)


def _np(A):
    return A.crow_indices().numpy(), A.col_indices().numpy(), A.values().numpy()


@pytest.mark.parametrize("grid, dims", [
    ((17, 13), [(17, 13), (9, 7), (5, 4), (3, 2), (2, 1), (1, 1)]),
    ((1, 7), [(1, 7), (1, 4), (1, 2), (1, 1)]),
    ((64, 64), [(64, 64), (32, 32), (16, 16), (8, 8), (4, 4), (2, 2), (1, 1)]),
    ((5, 1, 3), [(5, 1, 3), (3, 1, 2), (2, 1, 1), (1, 1, 1)]),
    ((2, 2, 2), [(2, 2, 2), (1, 1, 1)]),
    ((1, 1), [(1, 1)]),
])
def test_level_dimensions(grid, dims):
    M = AggregationMultigridPreconditioner(MM.csr_tensor(*MM.grid_matrix(grid)), grid)
    assert [lev.dims for lev in M.levels] == dims == MM.level_dims(grid)
    assert [lev.n for lev in M.levels] == [int(np.prod(d)) for d in dims]
    assert all(tuple(lev.csr.shape) == (lev.n, lev.n) and lev.dinv.numel() == lev.n for lev in M.levels)
    assert M.levels[-1].c0 is None and all(len(lev.c1) == len(lev.c2) == 1 for lev in M.levels[:-1])


def _matrices():
    p = _np(create_poisson_2d_csr(17, 13))
    yield "poisson17x13", (17, 13), p
    yield "vardiff33x65", (33, 65), _np(create_variable_diffusion_2d_csr(33, 65))
    yield "seven_point9x8x7", (9, 8, 7), MM.grid_matrix((9, 8, 7))
    for tr in ("shuf", "dup", "zero", "dup_shuf"):
        yield f"poisson17x13_{tr}", (17, 13), TRANSFORMS[tr](*p, seed=5)
    yield "vardiff33x65_fp32", (33, 65), tuple(a if i < 2 else a.astype(np.float32) for i, a in enumerate(_np(create_variable_diffusion_2d_csr(33, 65))))
    yield "seven_point9x8x7_fp32_shuf", (9, 8, 7), TRANSFORMS["shuf"](*MM.grid_matrix((9, 8, 7), seed=3, dtype=np.float32), seed=2)


MATRICES = {name: (grid, arrs) for name, grid, arrs in _matrices()}


@pytest.mark.parametrize("name", sorted(MATRICES))
def test_coarse_matrices_have_the_mirrors_bits(name):
    grid, (crow, col, val) = MATRICES[name]
    M = AggregationMultigridPreconditioner(MM.csr_tensor(crow, col, val), grid, normalize=False)
    assert M.levels[0].csr.values().dtype == torch.from_numpy(val).dtype
    for lev, nxt in zip(M.levels[:-1], M.levels[1:]):
        rc, cc, vc = MM.galerkin(crow, col, val, lev.dims)
        got = _np(nxt.csr)
        assert np.array_equal(got[0], rc) and np.array_equal(got[1], cc), (name, nxt.dims)
        assert MM.same_bits(got[2], vc), (name, nxt.dims)
        rows = np.repeat(np.arange(nxt.n), np.diff(rc))
        assert np.all(np.diff(cc)[np.diff(rows) == 0] > 0), "a coarse row is not strictly ascending"
        crow, col, val = rc, cc, vc
        # the smoother is ChebyshevPreconditioner's on that level matrix
        ref = ChebyshevPreconditioner(nxt.csr, degree=1, ratio=4.0, normalize=False) if nxt.n > 1 else None
        if ref is not None:
            assert (nxt.c0, nxt.c1, nxt.c2) == (ref.c0, ref.c1, ref.c2) and torch.equal(nxt.dinv, ref.dinv)


def test_galerkin_keeps_a_stored_zero_and_the_row_sums():
    """Grid (1, 4), aggregates {0, 1} and {2, 3}: the coarse off-diagonal entries are 1 + (-1) = 0 and stay stored."""
    crow, col = np.array([0, 2, 4, 6, 8]), np.array([0, 3, 1, 2, 1, 2, 0, 3])
    val = np.array([2.0, 1.0, 2.0, -1.0, -1.0, 2.0, 1.0, 2.0])
    M = AggregationMultigridPreconditioner(MM.csr_tensor(crow, col, val), (1, 4), normalize=False)
    c = M.levels[1].csr
    assert c.crow_indices().tolist() == [0, 2, 4] and c.col_indices().tolist() == [0, 1, 0, 1] and c.values().tolist() == [4.0, 0.0, 0.0, 4.0]
    A = create_variable_diffusion_2d_csr(8, 6)
    M = AggregationMultigridPreconditioner(A, (8, 6), normalize=False)
    fine, coarse = M.levels[0].csr.to_dense(), M.levels[1].csr.to_dense()
    P = torch.zeros(48, 12, dtype=torch.float64)
    P[torch.arange(48), torch.from_numpy(MM.aggregate(np.arange(48), (8, 6)))] = 1.0
    assert torch.allclose(coarse, P.T @ fine @ P, rtol=1e-13, atol=0.0)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("degree", [1, 2, 3])
@pytest.mark.parametrize("normalize", [True, False], ids=["normalized", "unscaled"])
@pytest.mark.parametrize("name", ["vardiff33x65", "seven_point9x8x7", "poisson17x13_dup_shuf"])
def test_cpu_apply_has_the_mirrors_bits(oracle, name, normalize, degree, dtype):
    grid, (crow, col, val) = MATRICES[name]
    A = MM.csr_tensor(crow, col, val.astype(dtype))
    M = AggregationMultigridPreconditioner(A, grid, degree=degree, normalize=normalize)
    assert (M.scale != 1.0) == normalize and M.applies == 0
    r = np.random.default_rng(11).standard_normal(A.shape[0]).astype(dtype)
    z = M(torch.from_numpy(r)).numpy()
    assert M.applies == 1
    assert MM.same_bits(z, MM.apply(oracle, M, r)), f"{np.count_nonzero(MM.bits(z) != MM.bits(MM.apply(oracle, M, r)))} entries differ"


def test_normalize_is_the_power_iteration_of_the_unscaled_cycle(oracle):
    grid, (crow, col, val) = MATRICES["poisson17x13"]
    A = MM.csr_tensor(crow, col, val)
    M1 = AggregationMultigridPreconditioner(A, grid, normalize=False)
    v = np.full(A.shape[0], 1.0 / np.sqrt(A.shape[0]))
    for _ in range(8):
        w = MM.apply(oracle, M1, v)
        lam = float(np.linalg.norm(w))
        v = w / lam
    M = AggregationMultigridPreconditioner(A, grid)
    assert M.scale == pytest.approx(1.0 / lam, rel=1e-13)
    dense = torch.stack([M(e) for e in torch.eye(A.shape[0], dtype=torch.float64)], 1)
    assert 0.95 < float(torch.linalg.eigvalsh((dense + dense.T) / 2).max()) < 1.0 + 1e-3     # the estimate is the operator's norm


def test_operator_is_symmetric_positive_definite():
    grid, (crow, col, val) = MATRICES["poisson17x13"]
    M = AggregationMultigridPreconditioner(MM.csr_tensor(crow, col, val), grid)
    D = torch.stack([M(e) for e in torch.eye(17 * 13, dtype=torch.float64)], 1)
    asym = float((D - D.T).abs().max() / D.abs().max())
    print(f"relative asymmetry {asym:.3e}")
    assert asym < 1e-12
    assert float(torch.linalg.eigvalsh((D + D.T) / 2).min()) > 0.0


def test_errors():
    A = create_poisson_2d_csr(6, 5)
    P = AggregationMultigridPreconditioner
    for bad in ((6, 6), (5, 5), (30,), (1, 2, 3, 5), (0, 30), (-6, -5)):
        with pytest.raises(ValueError, match="grid"):
            P(A, bad)
    for degree in (0, 33):
        with pytest.raises(ValueError, match="degree"):
            P(A, (6, 5), degree=degree)
    for omega in (0.0, -1.0):
        with pytest.raises(ValueError, match="omega"):
            P(A, (6, 5), omega=omega)
    with pytest.raises(ValueError, match="square"):
        P(torch.zeros(30, 29, dtype=torch.float64), (6, 5))
    with pytest.raises(ValueError, match="float"):
        P(torch.eye(30, dtype=torch.int64), (6, 5))
    with pytest.raises(ValueError, match="tail_rows"):
        P(A, (6, 5), tail_rows=-1)

    class FakeRowBlock:
        _hipk_row_block = True
    with pytest.raises(ValueError, match="RowBlockCSR"):
        P(FakeRowBlock(), (6, 5))
    M = P(A, (6, 5))
    for v in (torch.ones(29, dtype=torch.float64), torch.ones(30, 1, dtype=torch.float64), torch.ones(30, dtype=torch.float32),
              torch.ones(30, dtype=torch.float64, device="meta"), np.ones(30)):
        with pytest.raises(ValueError, match="applied to"):
            M(v)
    assert M.applies == 0


def test_non_positive_diagonal_names_the_level():
    N = create_ldc_pressure_csr(8)                      # the Neumann Laplacian with a NEGATIVE diagonal: level 0 refuses
    with pytest.raises(ValueError, match=r"level 0 \(8x8\).*diagonal"):
        AggregationMultigridPreconditioner(N, (8, 8))
    # its negative is positive semi-definite with row sums 0 (exact: multiples of 64): every Galerkin level keeps that, so the
    # level with one unknown is the stored zero
    crow, col, val = _np(N)
    with pytest.raises(ValueError, match=r"level 3 \(1x1\).*diagonal"):
        AggregationMultigridPreconditioner(MM.csr_tensor(crow, col, -val), (8, 8))


def test_dense_and_coo_layouts_give_the_csr_hierarchy():
    A = create_variable_diffusion_2d_csr(9, 6)
    ref = AggregationMultigridPreconditioner(A, (9, 6))
    for B in (A.to_dense(), A.to_sparse_coo()):
        M = AggregationMultigridPreconditioner(B, (9, 6))
        assert M.scale == ref.scale
        for a, b in zip(M.levels, ref.levels):
            assert torch.equal(a.csr.values(), b.csr.values()) and torch.equal(a.csr.col_indices(), b.csr.col_indices())


def test_tail_from_and_launch_count_follow_the_level_list():
    A = create_poisson_2d_csr(130, 70)                  # 9100, 2275, 594, 153, 45, 15, 6, 2, 1
    assert [lev.n for lev in AggregationMultigridPreconditioner(A, (130, 70), normalize=False).levels] == [9100, 2275, 594, 153, 45, 15, 6, 2, 1]
    for tail_rows, tail_from in ((0, None), (1, 8), (256, 3), (1024, 2), (4096, 1), (100000, 1)):
        M = AggregationMultigridPreconditioner(A, (130, 70), degree=2, normalize=False, tail_rows=tail_rows)
        assert M.tail_from == tail_from and M.tail_rows == min(tail_rows, 4096), (tail_rows, M.tail_from)
        assert M.launches_per_apply == (8 if tail_from is None else tail_from) * (2 * 2 + 7) + 1
    assert MG.MG_TAIL_MAX_ROWS in (0, 256, 1024, 4096)
    assert AggregationMultigridPreconditioner(A, (130, 70), normalize=False).tail_rows == MG.MG_TAIL_MAX_ROWS
    crow, col, val = MM.grid_matrix((12, 12), radius=3, full_box=True)        # rows of 49 entries: outside the tail's envelope
    M = AggregationMultigridPreconditioner(MM.csr_tensor(crow, col, val), (12, 12), normalize=False, tail_rows=4096)
    assert max(np.diff(crow)) == 49 and M.tail_from is None and M.launches_per_apply == 4 * 9 + 1


@pytest.mark.parametrize("name, A, grid", [("poisson200", lambda: create_poisson_2d_csr(200, 200), (200, 200)),
                                           ("vardiff128", lambda: create_variable_diffusion_2d_csr(128, 128), (128, 128))])
def test_cg_takes_a_tenth_of_the_iterations(name, A, grid):
    """The condition of the issue: at most one tenth of plain cg's iterations (a prototype had 14 against 320 and 28 against 2656)."""
    A = A()
    b = torch.ones(A.shape[0], dtype=torch.float64)
    x0, info0 = cg(A, b, tol=1e-6)
    plain = get_last_stats().iterations
    M = AggregationMultigridPreconditioner(A, grid)
    x, info = cg(A, b, tol=1e-6, M=M)
    its = get_last_stats().iterations
    relres = float(torch.linalg.vector_norm(b - A @ x) / torch.linalg.vector_norm(b))
    print(f"{name}: plain {plain}, multigrid {its}, relative residual {relres:.3e}, scale {M.scale:.6e}")
    assert info0 == 0 and info == 0
    assert relres <= 1e-6
    assert 10 * its <= plain
