"""BatchedBlockJacobiPreconditioner and the batch solves that take it, without a GPU: the blocks, the argument checks, and the loop
route on CPU tensors against the single solves with `M.system(s)`, bit for bit."""
import numpy as np
import pytest
import torch

from pytorch_sparse_solver.module_a import (BatchedBlockJacobiPreconditioner, BatchedCSR, BatchedJacobiPreconditioner,
                                            BlockJacobiPreconditioner, bicgstab, bicgstab_batch, cg, cg_batch, get_last_stats, gmres,
                                            gmres_batch)
from pytorch_sparse_solver.module_a import batch as batch_mod
from pytorch_sparse_solver.module_a.preconditioners import _diagonal_blocks
from pytorch_sparse_solver.utils.matrix_utils import create_convdiff_2d_csr, create_variable_diffusion_2d_csr


def _spd(nx=9, ny=7):
    return [create_variable_diffusion_2d_csr(nx, ny, contrast=c, seed=s) for c, s in ((0.5, 0), (1.0, 1), (2.0, 3))]


def _nonsym(nx=9, ny=7):
    return [create_convdiff_2d_csr(nx, ny, g, d) for g, d in ((0.5, 0.25), (0.2, 0.1), (0.8, 0.4))]


def _rhs(S, n, seed=0):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal((S, n)))


@pytest.mark.parametrize("bs", [1, 3, 4, 7, 32])
def test_blocks_are_the_diagonal_blocks_of_every_system(bs):
    for mats in (_spd(), _nonsym(), [m.to(torch.float32) for m in _nonsym()]):
        A = BatchedCSR.from_csr_list(mats)
        M = BatchedBlockJacobiPreconditioner(A, block_size=bs)
        nb = (63 + bs - 1) // bs
        assert M.binv.shape == (3, nb, bs, bs) and M.binv.is_contiguous() and M.binv.dtype == mats[0].dtype
        assert M.block_size == bs and M.shape == A.shape
        blocks = torch.stack([_diagonal_blocks(As, bs) for As in mats])
        assert torch.equal(M.binv, torch.linalg.inv(blocks.view(3 * nb, bs, bs)).view(3, nb, bs, bs))
        if 63 % bs:       # the ragged last block is completed with identity, which its inverse keeps
            k = 63 % bs
            tail = M.binv[:, nb - 1]
            assert torch.equal(tail[:, k:, k:], torch.eye(bs - k, dtype=tail.dtype).expand(3, -1, -1))
            assert not tail[:, :k, k:].any() and not tail[:, k:, :k].any()
        # to rounding the single preconditioner's own blocks (it inverts a batch of another size)
        for s, As in enumerate(mats):
            assert torch.allclose(M.binv[s], BlockJacobiPreconditioner(As, block_size=bs).binv, rtol=1e-5 if As.dtype == torch.float32 else 1e-12)


def test_entries_stored_twice_add():
    # rows [0: (0, 0, 1)], [1: (1, 0, 1)]: the entry (0, 0) is stored twice, (1, 1) twice
    crow, col = torch.tensor([0, 3, 6]), torch.tensor([0, 0, 1, 1, 0, 1])
    vals = torch.tensor([[1.0, 2.0, 0.5, 4.0, 0.25, 1.0], [2.0, 2.0, 1.0, 3.0, 0.5, 5.0]], dtype=torch.float64)
    A = BatchedCSR(crow, col, vals)
    M2 = BatchedBlockJacobiPreconditioner(A, block_size=2)
    want = torch.tensor([[[3.0, 0.5], [0.25, 5.0]], [[4.0, 1.0], [0.5, 8.0]]], dtype=torch.float64)
    assert torch.equal(M2.binv[:, 0], torch.linalg.inv(want))
    M1 = BatchedBlockJacobiPreconditioner(A, block_size=1)
    assert torch.equal(M1.binv.view(2, 2), BatchedJacobiPreconditioner(A).dinv)
    for s in range(2):
        assert torch.equal(_diagonal_blocks(A.system(s), 2)[0], want[s])


def test_a_singular_block_and_a_bad_block_size_raise():
    crow, col = torch.tensor([0, 2, 4]), torch.tensor([0, 1, 0, 1])
    A = BatchedCSR(crow, col, torch.tensor([[1.0, 2.0, 3.0, 4.0], [1.0, 2.0, 2.0, 4.0]], dtype=torch.float64))
    with pytest.raises(ValueError, match="singular"):
        BatchedBlockJacobiPreconditioner(A, block_size=2)
    BatchedBlockJacobiPreconditioner(A, block_size=1)
    for bs in (0, 33, -1):
        with pytest.raises(ValueError, match=r"block_size must be in \[1, 32\]"):
            BatchedBlockJacobiPreconditioner(A, block_size=bs)
    with pytest.raises(ValueError, match="needs a BatchedCSR"):
        BatchedBlockJacobiPreconditioner(A.system(0))


def test_given_blocks_are_used_as_they_are_and_checked():
    A = BatchedCSR.from_csr_list(_spd())
    eye = torch.eye(4, dtype=torch.float64).expand(3, 16, 4, 4).contiguous()
    M = BatchedBlockJacobiPreconditioner(A, block_size=4, binv=eye)
    assert M.binv.data_ptr() == eye.data_ptr() and M.block_size == 4 and M.shape == A.shape
    with pytest.raises(ValueError, match=r"binv must have shape \(S, ceil\(n / bs\), bs, bs\) = \(3, 16, 4, 4\)"):
        BatchedBlockJacobiPreconditioner(A, block_size=4, binv=eye[:, :15])
    with pytest.raises(ValueError, match="binv must have shape"):
        BatchedBlockJacobiPreconditioner(A, block_size=3, binv=eye)
    with pytest.raises(ValueError, match="binv must have shape"):
        BatchedBlockJacobiPreconditioner(A, block_size=4, binv=eye.numpy())
    with pytest.raises(ValueError, match="binv is torch.float32"):
        BatchedBlockJacobiPreconditioner(A, block_size=4, binv=eye.to(torch.float32))
    with pytest.raises(ValueError, match="on meta"):
        BatchedBlockJacobiPreconditioner(A, block_size=4, binv=eye.to("meta"))
    with pytest.raises(ValueError, match="contiguous"):
        BatchedBlockJacobiPreconditioner(A, block_size=4, binv=eye.transpose(2, 3).transpose(2, 3)[:, :, ::1].permute(0, 1, 3, 2))


def test_system_shares_the_storage_of_its_blocks():
    A = BatchedCSR.from_csr_list(_nonsym())
    M = BatchedBlockJacobiPreconditioner(A, block_size=3)
    for s in range(3):
        P = M.system(s)
        assert isinstance(P, BlockJacobiPreconditioner) and P.block_size == 3 and P.shape == (63, 63)
        assert P.binv.data_ptr() == M.binv[s].data_ptr() and torch.equal(P.binv, M.binv[s]) and P.binv.is_contiguous()
        v = _rhs(1, 63, s)[0]
        want = torch.bmm(M.binv[s], v.view(21, 3, 1)).view(-1)
        assert torch.equal(P(v), want)


@pytest.mark.parametrize("bs", [4, 5])
@pytest.mark.parametrize("kind", ["cg", "bicgstab"])
@pytest.mark.parametrize("route", ["loop", "auto"])
def test_cpu_batch_equals_the_single_solves_bitwise(kind, bs, route):
    mats = _spd() if kind == "cg" else _nonsym()
    A = BatchedCSR.from_csr_list(mats)
    B, X0 = _rhs(3, 63, 1), _rhs(3, 63, 2)
    M = BatchedBlockJacobiPreconditioner(A, block_size=bs)
    batch, single = (cg_batch, cg) if kind == "cg" else (bicgstab_batch, bicgstab)
    X, info = batch(A, B, X0, tol=1e-9, M=M, route=route)
    st = get_last_stats()
    assert info.dtype == torch.int64 and tuple(info.shape) == (3,) and st.path == "loop" and st.launches == 0
    assert "blockjacobi" in st.method and len(st.iterations) == 3
    for s, As in enumerate(mats):
        x, i = single(As, B[s], X0[s], tol=1e-9, M=M.system(s))
        assert torch.equal(X[s], x) and int(info[s]) == int(i), s
        assert float(torch.linalg.norm(As @ x - B[s])) <= 1e-6 * float(torch.linalg.norm(B[s])), s
    X2, info2 = batch(A, B, tol=1e-9, M=M, maxiter=3)
    for s, As in enumerate(mats):
        x, i = single(As, B[s], tol=1e-9, M=M.system(s), maxiter=3)
        assert torch.equal(X2[s], x) and int(info2[s]) == int(i) == -1, s
    with pytest.raises(ValueError, match="route='kernel' needs device tensors"):
        batch(A, B, M=M, route="kernel")


def test_identity_blocks_solve_like_no_preconditioner():
    mats = _spd()
    A = BatchedCSR.from_csr_list(mats)
    B = _rhs(3, 63, 4)
    eye = torch.eye(4, dtype=torch.float64).expand(3, 16, 4, 4).contiguous()
    X, info = cg_batch(A, B, tol=1e-9, M=BatchedBlockJacobiPreconditioner(A, block_size=4, binv=eye))
    X0, info0 = cg_batch(A, B, tol=1e-9)
    assert torch.equal(info, info0) and torch.allclose(X, X0, rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("route", ["loop", "auto"])
def test_gmres_batch_runs_the_loop_and_its_kernel_route_raises(route):
    mats = _nonsym()
    A = BatchedCSR.from_csr_list(mats)
    B = _rhs(3, 63, 3)
    M = BatchedBlockJacobiPreconditioner(A, block_size=4)
    X, info = gmres_batch(A, B, tol=1e-9, restart=10, M=M, route=route)
    assert get_last_stats().path == "loop"
    for s, As in enumerate(mats):
        x, i = gmres(As, B[s], tol=1e-9, restart=10, M=M.system(s))
        assert torch.equal(X[s], x) and int(info[s]) == int(i) == 0, s
    with pytest.raises(ValueError, match="the GMRES batch kernel has no block-Jacobi form"):
        gmres_batch(A, B, M=M, route="kernel")


def test_a_foreign_preconditioner_and_one_of_another_batch_raise():
    A = BatchedCSR.from_csr_list(_spd())
    B = _rhs(3, 63)
    for fn in (cg_batch, bicgstab_batch, gmres_batch):
        with pytest.raises(ValueError, match="M must be None or a BatchedJacobiPreconditioner"):
            fn(A, B, M=BlockJacobiPreconditioner(A.system(0), block_size=4))
        with pytest.raises(ValueError, match="BatchedBlockJacobiPreconditioner, got function"):
            fn(A, B, M=lambda v: v)
        with pytest.raises(ValueError, match="does not match A"):
            fn(A, B, M=BatchedBlockJacobiPreconditioner(BatchedCSR.from_csr_list(_spd()[:2]), block_size=4))
        with pytest.raises(ValueError, match="does not match A"):
            fn(A, B, M=BatchedBlockJacobiPreconditioner(BatchedCSR.from_csr_list(_spd(7, 5)), block_size=4))


def test_the_auto_threshold_is_its_own_constant_and_the_work_size_is_host_code():
    from pytorch_sparse_solver import _hipk
    assert isinstance(batch_mod.BJ_BATCH_MIN_SYSTEMS, int) and batch_mod.BJ_BATCH_MIN_SYSTEMS >= 1
    for method, nvec in (("cg", 3), ("bicgstab", 5)):
        for dt, es in ((torch.float64, 8), (torch.float32, 4)):
            last = 0
            for n in (1, 35, 255, 256, 257, 1024, 1025, 2048, 2049, 4096):
                wb = _hipk.bj_batch_work_bytes(n, 5 * n, 7, dt, method, 4)
                assert wb % 256 == 0 and wb >= last and wb >= 7 * nvec * n * es
                assert wb == _hipk.bj_batch_work_bytes(n, 5 * n, 7, dt, method, 32)
                last = wb
    # the existing size function keeps its values
    assert _hipk.batch_work_bytes(64, 300, 3, torch.float64, "cg", True) == 256 + 3 * 256 + 3 * 2 * 512
