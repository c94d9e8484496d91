"""gmres_batch without a GPU: the loop route on CPU tensors equals the single solves bit for bit, the argument checks, and the
workspace size function."""
import numpy as np
import pytest
import torch

from pytorch_sparse_solver.module_a import (BatchedCSR, BatchedJacobiPreconditioner, JacobiPreconditioner, get_last_stats, gmres,
                                            gmres_batch)
from pytorch_sparse_solver.utils.matrix_utils import create_convdiff_2d_csr


def _nonsym(nx=9, ny=7):
    return [create_convdiff_2d_csr(nx, ny, g, d) for g, d in ((0.5, 0.25), (0.2, 0.1), (0.8, 0.4))]


def _rhs(S, n, seed=0):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal((S, n)))


@pytest.mark.parametrize("jacobi", [False, True])
@pytest.mark.parametrize("method", ["batched", "incremental"])
@pytest.mark.parametrize("route", ["loop", "auto"])
def test_cpu_batch_equals_the_single_solves_bitwise(method, jacobi, route):
    mats = _nonsym()
    A = BatchedCSR.from_csr_list(mats)
    B, X0 = _rhs(3, 63, 1), _rhs(3, 63, 2)
    M = BatchedJacobiPreconditioner(A) if jacobi else None
    X, info = gmres_batch(A, B, X0, tol=1e-9, restart=7, M=M, solve_method=method, route=route)
    st = get_last_stats()
    assert info.dtype == torch.int64 and tuple(info.shape) == (3,) and st.path == "loop" and st.launches == 0
    assert st.method == ("pgmres_jacobi_batch" if jacobi else "gmres_batch")
    assert len(st.iterations) == len(st.matvecs) == len(st.info) == len(st.breakdown) == 3
    for s, As in enumerate(mats):
        x, i = gmres(As, B[s], X0[s], tol=1e-9, restart=7, M=JacobiPreconditioner(As) if jacobi else None, solve_method=method)
        assert torch.equal(X[s], x) and int(info[s]) == int(i), s
    # restart beyond the kernel's bound and a cycle budget: still the single solves
    X2, info2 = gmres_batch(A, B, tol=1e-9, restart=40, M=M, solve_method=method, maxiter=1, route=route)
    for s, As in enumerate(mats):
        x, i = gmres(As, B[s], tol=1e-9, restart=40, M=JacobiPreconditioner(As) if jacobi else None, solve_method=method, maxiter=1)
        assert torch.equal(X2[s], x) and int(info2[s]) == int(i), s
    X3, info3 = gmres_batch(A, B, tol=1e-9, restart=2, M=M, solve_method=method, maxiter=2, route=route)
    assert [int(i) for i in info3] == [-1, -1, -1] and get_last_stats().iterations == [2, 2, 2]


def test_argument_errors():
    A = BatchedCSR.from_csr_list(_nonsym())
    B = _rhs(3, 63)
    with pytest.raises(ValueError, match=r"gmres_batch: B must have shape \(S, n\)"):
        gmres_batch(A, B[0])
    with pytest.raises(ValueError, match=r"X0 must have shape \(S, n\)"):
        gmres_batch(A, B, B[:2])
    with pytest.raises(ValueError, match="real floating-point"):
        gmres_batch(A, B.to(torch.complex128))
    with pytest.raises(ValueError, match="B is torch.float32, the matrices are torch.float64"):
        gmres_batch(A, B.to(torch.float32))
    with pytest.raises(ValueError, match="is on meta"):
        gmres_batch(A, B.to("meta"))
    with pytest.raises(ValueError, match="M must be None or a BatchedJacobiPreconditioner"):
        gmres_batch(A, B, M=JacobiPreconditioner(A.system(0)))
    with pytest.raises(ValueError, match="does not match A"):
        gmres_batch(A, B, M=BatchedJacobiPreconditioner(BatchedCSR.from_csr_list(_nonsym()[:2])))
    with pytest.raises(ValueError, match="not differentiable: call gmres_differentiable"):
        gmres_batch(A, B.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="A must be a BatchedCSR"):
        gmres_batch(A.system(0), B)
    with pytest.raises(ValueError, match="route must be"):
        gmres_batch(A, B, route="fast")
    with pytest.raises(ValueError, match="route='kernel' needs device tensors"):
        gmres_batch(A, B, route="kernel")
    for restart in (0, -3):
        with pytest.raises(ValueError, match="restart must be at least 1"):
            gmres_batch(A, B, restart=restart)
    with pytest.raises(ValueError, match="Unsupported solve_method: qr"):
        gmres_batch(A, B, solve_method="qr")


def test_gmres_batch_work_bytes_without_a_gpu():
    from pytorch_sparse_solver import _hipk
    for pre in (False, True):
        for dt in (torch.float64, torch.float32):
            es = 8 if dt == torch.float64 else 4
            last = 0
            for S in (1, 2, 5, 300, 4096):
                wb = _hipk.gmres_batch_work_bytes(1025, 5000, S, dt, 20, pre)
                assert wb % 256 == 0 and wb > last and wb >= S * 21 * 1025 * es
                last = wb
            last = 0
            for restart in range(1, 32):
                wb = _hipk.gmres_batch_work_bytes(257, 1300, 7, dt, restart, pre)
                assert wb % 256 == 0 and wb > last and wb >= 7 * (restart + 1) * 257 * es
                last = wb
            last = 0
            for n in (1, 35, 255, 256, 257, 1024, 1025, 2048, 2049, 4096):
                wb = _hipk.gmres_batch_work_bytes(n, 5 * n, 7, dt, 9, pre)
                assert wb % 256 == 0 and wb >= last
                last = wb
            for restart in (-1, 0, 32, 255):
                assert _hipk.gmres_batch_work_bytes(257, 1300, 7, dt, restart, pre) == 0
