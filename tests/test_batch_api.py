"""cg_batch / bicgstab_batch without a GPU: the loop route on CPU tensors equals the single solves bit for bit, the argument checks,
the Jacobi vectors, and the workspace size function."""
import numpy as np
import pytest
import torch

from pytorch_sparse_solver.module_a import (BatchedCSR, BatchedJacobiPreconditioner, JacobiPreconditioner, bicgstab, bicgstab_batch, cg,
                                            cg_batch, get_last_stats)
from pytorch_sparse_solver.utils.matrix_utils import create_convdiff_2d_csr, create_variable_diffusion_2d_csr


def _spd(nx=9, ny=7):
    return [create_variable_diffusion_2d_csr(nx, ny, contrast=c, seed=s) for c, s in ((0.5, 0), (1.0, 1), (2.0, 3))]


def _nonsym(nx=9, ny=7):
    return [create_convdiff_2d_csr(nx, ny, g, d) for g, d in ((0.5, 0.25), (0.2, 0.1), (0.8, 0.4))]


def _rhs(S, n, seed=0):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal((S, n)))


@pytest.mark.parametrize("jacobi", [False, True])
@pytest.mark.parametrize("kind", ["cg", "bicgstab"])
@pytest.mark.parametrize("route", ["loop", "auto"])
def test_cpu_batch_equals_the_single_solves_bitwise(kind, jacobi, route):
    mats = _spd() if kind == "cg" else _nonsym()
    A = BatchedCSR.from_csr_list(mats)
    assert A.shape == (3, 63, 63) and A.crow32.dtype == torch.int32 and A.col32.dtype == torch.int32
    B, X0 = _rhs(3, 63, 1), _rhs(3, 63, 2)
    M = BatchedJacobiPreconditioner(A) if jacobi else None
    batch, single = (cg_batch, cg) if kind == "cg" else (bicgstab_batch, bicgstab)
    X, info = batch(A, B, X0, tol=1e-9, M=M, route=route)
    st = get_last_stats()
    assert info.dtype == torch.int64 and tuple(info.shape) == (3,) and st.path == "loop" and st.launches == 0
    assert len(st.iterations) == len(st.matvecs) == len(st.info) == len(st.breakdown) == 3
    for s, As in enumerate(mats):
        x, i = single(As, B[s], X0[s], tol=1e-9, M=JacobiPreconditioner(As) if jacobi else None)
        assert torch.equal(X[s], x) and int(info[s]) == int(i), s
    X2, info2 = batch(A, B, tol=1e-9, M=M, maxiter=4)
    for s, As in enumerate(mats):
        x, i = single(As, B[s], tol=1e-9, M=JacobiPreconditioner(As) if jacobi else None, maxiter=4)
        assert torch.equal(X2[s], x) and int(info2[s]) == int(i) == -1, s


def test_batched_jacobi_rows_are_the_single_preconditioners():
    for mats in (_spd(), _nonsym(), [m.to(torch.float32) for m in _spd()]):
        A = BatchedCSR.from_csr_list(mats)
        M = BatchedJacobiPreconditioner(A)
        assert M.dinv.shape == (3, 63) and M.dinv.dtype == mats[0].dtype
        for s, As in enumerate(mats):
            assert torch.equal(M.dinv[s], JacobiPreconditioner(As).dinv)
    crow, col = torch.tensor([0, 2, 4]), torch.tensor([0, 1, 0, 1])
    with pytest.raises(ValueError, match="zero on the diagonal"):
        BatchedJacobiPreconditioner(BatchedCSR(crow, col, torch.tensor([[1.0, 2.0, 3.0, 4.0], [1.0, 2.0, 3.0, 0.0]], dtype=torch.float64)))


def test_from_csr_list_rejects_a_differing_pattern():
    a = _spd()
    other = create_variable_diffusion_2d_csr(7, 9)
    with pytest.raises(ValueError, match="sparsity pattern"):
        BatchedCSR.from_csr_list([a[0], other])
    dense = a[0].to_dense()
    dense[0, 5] = 1.0
    with pytest.raises(ValueError, match="sparsity pattern|differs from matrix 0"):
        BatchedCSR.from_csr_list([a[0], dense.to_sparse_csr()])
    with pytest.raises(ValueError, match="square torch CSR"):
        BatchedCSR.from_csr_list([a[0], a[1].to_dense()])
    with pytest.raises(ValueError, match="differs from matrix 0"):
        BatchedCSR.from_csr_list([a[0], a[1].to(torch.float32)])
    with pytest.raises(ValueError, match="empty"):
        BatchedCSR.from_csr_list([])


def test_argument_errors():
    A = BatchedCSR.from_csr_list(_spd())
    B = _rhs(3, 63)
    with pytest.raises(ValueError, match=r"B must have shape \(S, n\)"):
        cg_batch(A, B[0])
    with pytest.raises(ValueError, match=r"B must have shape \(S, n\)"):
        cg_batch(A, B.T.contiguous())
    with pytest.raises(ValueError, match=r"X0 must have shape \(S, n\)"):
        bicgstab_batch(A, B, B[:2])
    with pytest.raises(ValueError, match="real floating-point"):
        cg_batch(A, B.to(torch.complex128))
    with pytest.raises(ValueError, match="real floating-point"):
        cg_batch(A, B.to(torch.int64))
    with pytest.raises(ValueError, match="B is torch.float32, the matrices are torch.float64"):
        cg_batch(A, B.to(torch.float32))
    with pytest.raises(ValueError, match="X0 is torch.float32"):
        bicgstab_batch(A, B, B.to(torch.float32))
    with pytest.raises(ValueError, match="is on meta"):
        cg_batch(A, B.to("meta"))
    with pytest.raises(ValueError, match="M must be None or a BatchedJacobiPreconditioner"):
        cg_batch(A, B, M=JacobiPreconditioner(A.system(0)))
    with pytest.raises(ValueError, match="M must be None or a BatchedJacobiPreconditioner"):
        bicgstab_batch(A, B, M=lambda v: v)
    with pytest.raises(ValueError, match="does not match A"):
        cg_batch(A, B, M=BatchedJacobiPreconditioner(BatchedCSR.from_csr_list(_spd()[:2])))
    with pytest.raises(ValueError, match="not differentiable: call cg_differentiable"):
        cg_batch(A, B.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="not differentiable: call bicgstab_differentiable"):
        bicgstab_batch(A, B, B.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="not differentiable"):
        BatchedCSR(A.crow, A.col, A.values.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="A must be a BatchedCSR"):
        cg_batch(A.system(0), B)
    with pytest.raises(ValueError, match="route must be"):
        cg_batch(A, B, route="fast")
    with pytest.raises(ValueError, match="route='kernel' needs device tensors"):
        cg_batch(A, B, route="kernel")
    with pytest.raises(ValueError, match="route='kernel' needs device tensors"):
        bicgstab_batch(A, B, route="kernel")
    with pytest.raises(ValueError, match="float64 or float32"):
        BatchedCSR(A.crow, A.col, A.values.to(torch.float16))
    with pytest.raises(ValueError, match=r"values must have shape \(S, nnz\)"):
        BatchedCSR(A.crow, A.col, A.values[:, :-1])
    with pytest.raises(ValueError, match="row pointer"):
        BatchedCSR(torch.flip(A.crow, [0]), A.col, A.values)
    with pytest.raises(ValueError, match="column index"):
        BatchedCSR(A.crow, A.col + 1, A.values)


def test_batch_work_bytes_without_a_gpu():
    from pytorch_sparse_solver import _hipk
    for method in ("cg", "bicgstab"):
        for pre in (False, True):
            for dt in (torch.float64, torch.float32):
                last = 0
                for S in (1, 2, 5, 300, 4096):
                    wb = _hipk.batch_work_bytes(1025, 5000, S, dt, method, pre)
                    assert wb % 256 == 0 and wb >= last and wb >= S * 1025 * (8 if dt == torch.float64 else 4)
                    last = wb
                last = 0
                for n in (1, 35, 255, 256, 257, 1024, 1025, 2048, 2049, 4096):
                    wb = _hipk.batch_work_bytes(n, 5 * n, 7, dt, method, pre)
                    assert wb % 256 == 0 and wb >= last
                    last = wb
    assert _hipk.batch_work_bytes(64, 300, 3, torch.float64, "bicgstab", True) > _hipk.batch_work_bytes(64, 300, 3, torch.float64, "cg", False)
