"""cg_multi / bicgstab_multi without a GPU: the generic route (a loop over the columns through cg / bicgstab), the shape, dtype
and error contract, the workspace query of the block solves and the exports."""
import os

import pytest
import torch


def _poisson(nx, dtype=torch.float64):
    from pytorch_sparse_solver.utils.matrix_utils import create_poisson_2d_csr
    return create_poisson_2d_csr(nx, nx, dtype=dtype)


def _convdiff(nx):
    from pytorch_sparse_solver.utils.matrix_utils import create_convdiff_2d_csr
    return create_convdiff_2d_csr(nx, nx)


def _rhs(n, k, seed):
    return torch.randn(n, k, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def test_exports():
    import pytorch_sparse_solver.module_a as ma
    from pytorch_sparse_solver import _hipk
    assert callable(ma.cg_multi) and callable(ma.bicgstab_multi)
    assert {"cg_multi", "bicgstab_multi"} <= set(ma.__all__)
    assert {"hipk_multi_work_bytes", "hipk_cg_solve_multi", "hipk_bicgstab_solve_multi"} <= set(_hipk.SYMBOLS)


@pytest.mark.parametrize("kind", ["cg", "bicgstab"])
def test_cpu_columns_equal_single_solves(kind):
    from pytorch_sparse_solver import _hipk
    from pytorch_sparse_solver.module_a import bicgstab, bicgstab_multi, cg, cg_multi, get_last_stats
    multi, single = (cg_multi, cg) if kind == "cg" else (bicgstab_multi, bicgstab)
    A = _poisson(12) if kind == "cg" else _convdiff(12)
    n = 144
    B = _rhs(n, 4, 1)
    B[:, 2] = 0.0
    X0 = _rhs(n, 4, 2) * 0.1
    X0[:, 2] = 0.0
    X, info = multi(A, B, X0, tol=1e-7, maxiter=60)
    st = get_last_stats()
    assert X.shape == (n, 4) and X.dtype == torch.float64
    assert info.dtype == torch.int64 and info.shape == (4,) and info.device.type == "cpu"
    assert isinstance(st, _hipk.MultiSolveStats) and st.block_spmvs == 0 and len(st.columns) == 4
    for j in range(4):
        xs, inf = single(A, B[:, j], X0[:, j], tol=1e-7, maxiter=60)
        ss = get_last_stats()
        assert torch.equal(X[:, j], xs) and int(info[j]) == inf
        assert (st.columns[j].iterations, st.columns[j].matvecs) == (ss.iterations, ss.matvecs)
    assert torch.equal(X[:, 2], torch.zeros(n, dtype=torch.float64)) and int(info[2]) == 0


def test_cpu_fp32_matrix_behaves_like_cg():
    """The generic route keeps cg's behaviour exactly: an fp32 CPU matrix meets fp64-promoted vectors and raises there too."""
    from pytorch_sparse_solver.module_a import cg, cg_multi
    A = _poisson(6, dtype=torch.float32)
    B = _rhs(36, 2, 3).to(torch.float32)
    with pytest.raises(RuntimeError) as e1:
        cg(A, B[:, 0])
    with pytest.raises(RuntimeError) as e2:
        cg_multi(A, B)
    assert str(e1.value) == str(e2.value)


def test_callable_operator_and_pytree_route():
    from pytorch_sparse_solver.module_a import cg, cg_multi
    A = _poisson(5).to_dense()
    B = _rhs(25, 3, 4)
    X, info = cg_multi(lambda v: A @ v, B, tol=1e-8)
    for j in range(3):
        assert torch.equal(X[:, j], cg(lambda v: A @ v, B[:, j], tol=1e-8)[0])
    Bt = {"u": B[:10], "v": B[10:]}
    Xt, info_t = cg_multi(lambda t: {"u": (A @ torch.cat([t["u"], t["v"]]))[:10], "v": (A @ torch.cat([t["u"], t["v"]]))[10:]},
                          Bt, tol=1e-8)
    assert set(Xt) == {"u", "v"} and Xt["u"].shape == (10, 3) and Xt["v"].shape == (15, 3)
    assert torch.allclose(torch.cat([Xt["u"], Xt["v"]]), X, atol=1e-12)


def test_errors():
    from pytorch_sparse_solver.module_a import bicgstab_multi, cg_multi
    A = _poisson(4)
    B = _rhs(16, 2, 5)
    with pytest.raises(ValueError, match=r"must have shape \(n, k\)"):
        cg_multi(A, B[:, 0])
    with pytest.raises(ValueError, match=r"must have shape \(n, k\)"):
        bicgstab_multi(A, B.reshape(16, 2, 1))
    with pytest.raises(ValueError, match=r"must have shape \(n, k\)"):
        cg_multi(A, torch.zeros(16, 0, dtype=torch.float64))
    with pytest.raises(ValueError, match="matching shapes"):
        cg_multi(A, B, torch.zeros(16, 3, dtype=torch.float64))
    with pytest.raises(ValueError, match="square matrix"):
        cg_multi(torch.zeros(16, 15, dtype=torch.float64), B)
    with pytest.raises(ValueError, match="cg_differentiable"):
        cg_multi(A, B.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="bicgstab_differentiable"):
        bicgstab_multi(A, B, torch.zeros_like(B).requires_grad_(True))
    with pytest.raises(ValueError, match="cg_differentiable"):
        cg_multi(A.to_dense().requires_grad_(True), B)


def _lib():
    import torch  # noqa: F401  (HIP runtime first)
    from pytorch_sparse_solver import _hipk
    if not os.path.exists(_hipk.LIB_PATH):
        _hipk.build()
    return _hipk.lib()


@pytest.mark.parametrize("solver,precond,nvec", [(0, 0, 3), (0, 1, 3), (1, 0, 6), (1, 1, 8)])
def test_work_bytes_monotone_and_covering(solver, precond, nvec):
    L = _lib()
    for dtype, sz in ((1, 8), (0, 4)):
        prev_n = 0
        for n in (1, 255, 2049, 40_000, 4_000_000):
            prev_k = 0
            g = L.hipk_chunk_count(n)
            for k in (1, 2, 3, 4, 8, 9, 16, 17, 40):
                wb = L.hipk_multi_work_bytes(n, k, dtype, solver, precond)
                assert wb >= prev_k
                prev_k = wb
                kb = min(k, 16)
                # the vectors the loop keeps (CG r, p, Ap; BiCGStab r, rhat, p, q, s, t (+ phat, shat)) for every column of a
                # block, plus the per-column chunk-partial slots of its dots (<p,Ap>, <r,r>, ... : at least three)
                assert wb >= kb * (nvec * n * sz + 3 * g * 8)
            wb1 = L.hipk_multi_work_bytes(n, 1, dtype, solver, precond)
            assert wb1 >= prev_n
            prev_n = wb1
