"""cg_batch_differentiable / bicgstab_batch_differentiable / gmres_batch_differentiable on CPU tensors, through the loop route (no GPU):
the forward is the plain batch solve bit for bit, the gradients of system s are those of the single solve differentiated alone (X0 =
None) or the mirror (tests/_vgrad_mirror.py) of X and an explicit batch solve of the transposed systems; and the pieces they stand on:
`BatchedCSR.with_values`, `BatchedCSR.transposed`, `BatchedBlockJacobiPreconditioner.transposed`."""
import numpy as np
import pytest
import torch

import _batch_patterns as BP
import _vgrad_mirror as VM

S, NP = 4, 40


def _batch(solver="cg", transform=None, S=S, n=NP, seed=3):
    from pytorch_sparse_solver.module_a import BatchedCSR
    crow, col, vals = BP.build_pattern(("rag31", n), transform, solver, S, np.random.default_rng(seed))
    return BatchedCSR(torch.from_numpy(crow), torch.from_numpy(col), torch.from_numpy(vals))


def _rand(shape, seed):
    return torch.randn(shape, dtype=torch.float64, generator=torch.Generator().manual_seed(seed))


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _funcs(kind):
    from pytorch_sparse_solver import module_a as MA
    return getattr(MA, f"{kind}_batch"), getattr(MA, f"{kind}_batch_differentiable"), getattr(MA, kind)


def _precond(A, which):
    from pytorch_sparse_solver.module_a import BatchedBlockJacobiPreconditioner, BatchedJacobiPreconditioner
    return {None: lambda: None, "jacobi": lambda: BatchedJacobiPreconditioner(A), "bj": lambda: BatchedBlockJacobiPreconditioner(A, 4)}[which]()


@pytest.mark.parametrize("kind", ["cg", "bicgstab", "gmres"])
def test_forward_is_the_plain_batch_solve(kind):
    plain, diff, _ = _funcs(kind)
    A = _batch(kind)
    B, X0 = _rand((S, NP), 1), _rand((S, NP), 2)
    X, info = plain(A, B, X0, tol=1e-9, route="loop")
    Xd = diff(A, B.clone().requires_grad_(), X0, values=A.values.clone().requires_grad_(), tol=1e-9, route="loop")
    assert Xd.requires_grad and _bits(Xd.detach().numpy(), X.numpy())


@pytest.mark.parametrize("precond", [None, "jacobi"])
def test_cg_gradients_are_those_of_the_single_solves_differentiated_alone(precond):
    from pytorch_sparse_solver.module_a import cg, cg_batch_differentiable, get_last_grad_stats
    A = _batch("cg")
    M = _precond(A, precond)
    B, W = _rand((S, NP), 1), _rand((S, NP), 4)
    vals, Bb = A.values.clone().requires_grad_(), B.clone().requires_grad_()
    X = cg_batch_differentiable(A, Bb, values=vals, tol=1e-9, M=M, route="loop")
    (X * W).sum().backward()
    st = get_last_grad_stats()
    assert (st.route, st.launches, st.nnz, st.batch) == ("torch", 0, A.nnz, S)
    assert vals.grad.shape == (S, A.nnz) and Bb.grad.shape == (S, NP)
    for s in range(S):
        As = A.system(s).requires_grad_()
        bs = B[s].clone().requires_grad_()
        x, _ = cg(As, bs, tol=1e-9, M=None if M is None else M.system(s))
        assert _bits(x.detach().numpy(), X[s].detach().numpy())
        (x * W[s]).sum().backward()
        assert _bits(Bb.grad[s].numpy(), bs.grad.numpy()), f"grad_B of system {s}"
        assert _bits(vals.grad[s].numpy(), As.grad.values().numpy()), f"grad_values of system {s}"


@pytest.mark.parametrize("kind,precond", [("cg", None), ("cg", "bj"), ("bicgstab", "jacobi"), ("bicgstab", "bj"), ("gmres", None),
                                          ("gmres", "jacobi")])
def test_gradients_with_a_start_vector_are_the_mirror_of_x_and_the_transposed_batch_solve(kind, precond):
    """The adjoint solve starts from X0 = None whatever the forward's X0 was."""
    plain, diff, _ = _funcs(kind)
    A = _batch(kind, transform="dup_shuf")
    M = _precond(A, precond)
    B, X0, W = _rand((S, NP), 1), _rand((S, NP), 2), _rand((S, NP), 4)
    vals, Bb = A.values.clone().requires_grad_(), B.clone().requires_grad_()
    X = diff(A, Bb, X0, values=vals, tol=1e-9, M=M, route="loop")
    (X * W).sum().backward()
    Mt = M.transposed() if precond == "bj" else M
    Lam, _ = plain(A.transposed(), W.clone(), None, tol=1e-9, M=Mt, route="loop")
    assert _bits(Bb.grad.numpy(), Lam.numpy())
    want = VM.batch_grad_values(A.crow.numpy(), A.col.numpy(), Lam.numpy(), X.detach().numpy(), np.float64)
    assert _bits(vals.grad.numpy(), want)


def test_only_the_needed_gradients_are_formed():
    from pytorch_sparse_solver.module_a import cg_batch_differentiable
    A = _batch("cg")
    B, W = _rand((S, NP), 1), _rand((S, NP), 4)
    Bb = B.clone().requires_grad_()
    X = cg_batch_differentiable(A, Bb, tol=1e-9, route="loop")                   # values=None: A.values, no gradient
    (X * W).sum().backward()
    assert Bb.grad is not None and A.values.grad is None
    vals = A.values.clone().requires_grad_()
    X = cg_batch_differentiable(A, B, values=vals, tol=1e-9, route="loop")       # only the values
    (X * W).sum().backward()
    assert vals.grad is not None and B.grad is None
    X = cg_batch_differentiable(A, B, tol=1e-9, route="loop")
    assert not X.requires_grad


def test_with_values_shares_the_pattern_objects():
    A = _batch("cg")
    P, perm = A.transpose_pattern()
    A2 = A.with_values(A.values * 2.0)
    assert A2.crow is A.crow and A2.col is A.col and A2.crow32 is A.crow32 and A2.col32 is A.col32
    assert (A2.n, A2.nnz, A2.batch, A2.max_row_len, A2.shape) == (A.n, A.nnz, A.batch, A.max_row_len, A.shape)
    assert A2.transpose_pattern()[0] is P and A2.transpose_pattern()[1] is perm
    A3 = A.with_values(A.values[:2])
    assert A3.batch == 2 and A3.shape == (2, A.n, A.n)
    with pytest.raises(ValueError, match="shape"):
        A.with_values(A.values[:, :-1])
    with pytest.raises(ValueError, match="float64 or float32"):
        A.with_values(A.values.to(torch.float16))
    with pytest.raises(ValueError, match="not differentiable"):
        A.with_values(A.values.clone().requires_grad_())


@pytest.mark.parametrize("transform", [None, "rev", "shuf", "dup", "dup_shuf", "zero"])
@pytest.mark.parametrize("pattern", ["rag31", "empty"])
def test_transposed_matches_the_dense_transposes(pattern, transform):
    from pytorch_sparse_solver.module_a import BatchedCSR
    n = 300 if pattern == "empty" else NP
    crow, col, vals = BP.build_pattern((pattern, n), transform, "bicgstab", 3, np.random.default_rng(1))
    A = BatchedCSR(torch.from_numpy(crow), torch.from_numpy(col), torch.from_numpy(vals))
    At = A.transposed()
    assert (At.n, At.nnz, At.batch) == (A.n, A.nnz, A.batch) and At.crow32.dtype == torch.int32
    for s in range(3):
        assert torch.equal(At.system(s).to_dense(), A.system(s).to_dense().T)     # entries stored twice add on both sides
    tc, tj = At.crow.numpy(), At.col.numpy()
    for r in range(n):
        assert np.all(np.diff(tj[tc[r]:tc[r + 1]]) >= 0)     # a stable sort by column: every row of A^T lists its source rows ascending
    assert int(At.max_row_len) == int(np.diff(tc).max())
    assert A.transposed().crow is At.crow and A.transposed().col32 is At.col32   # the pattern is cached, the values gathered per call


def test_transposed_block_jacobi_preconditioner():
    from pytorch_sparse_solver.module_a import BatchedBlockJacobiPreconditioner
    A = _batch("bicgstab", n=42)          # 42 = 10 blocks of 4 and a ragged one of 2
    M = BatchedBlockJacobiPreconditioner(A, 4)
    Mt = M.transposed()
    assert Mt.block_size == 4 and Mt.shape == M.shape and Mt.binv.is_contiguous()
    assert torch.equal(Mt.binv, M.binv.transpose(-1, -2))
    direct = BatchedBlockJacobiPreconditioner(A.transposed(), 4)      # inverts the blocks of A^T: equal up to the inverse's rounding
    assert torch.allclose(Mt.binv, direct.binv, rtol=1e-12, atol=1e-14)
    v = _rand((42,), 9)
    for s in range(2):
        assert torch.allclose(Mt.system(s)(v), direct.system(s)(v), rtol=1e-12, atol=1e-14)


def test_argument_errors():
    from pytorch_sparse_solver.module_a import cg_batch_differentiable, gmres_batch_differentiable
    A = _batch("cg")
    B = _rand((S, NP), 1)
    with pytest.raises(ValueError, match="BatchedCSR"):
        cg_batch_differentiable(A.system(0), B)
    with pytest.raises(ValueError, match="values must be"):
        cg_batch_differentiable(A, B, values=A.values[:, :-1])
    with pytest.raises(ValueError, match="values must be"):
        cg_batch_differentiable(A, B, values=A.values.float())
    with pytest.raises(ValueError, match="values must be"):
        cg_batch_differentiable(A, B, values=A.values[:2])
    with pytest.raises(ValueError, match="X0 is not differentiated"):
        cg_batch_differentiable(A, B, B.clone().requires_grad_())
    with pytest.raises(ValueError, match="shape"):
        cg_batch_differentiable(A, B[:, :-1])
    with pytest.raises(ValueError, match="route"):
        cg_batch_differentiable(A, B, route="fast")
    with pytest.raises(ValueError, match="route='kernel' needs device tensors"):
        cg_batch_differentiable(A, B, route="kernel")
    with pytest.raises(ValueError, match="restart"):
        gmres_batch_differentiable(A, B, restart=0)


def test_the_plain_batch_solves_still_refuse_requires_grad():
    from pytorch_sparse_solver.module_a import BatchedCSR, bicgstab_batch, cg_batch, gmres_batch
    A = _batch("cg")
    B = _rand((S, NP), 1)
    for f in (cg_batch, bicgstab_batch, gmres_batch):
        with pytest.raises(ValueError, match="not differentiable"):
            f(A, B.clone().requires_grad_(), route="loop")
    with pytest.raises(ValueError, match="not differentiable"):
        BatchedCSR(A.crow, A.col, A.values.clone().requires_grad_())


def test_values_modified_in_place_before_backward_are_an_error():
    """The values are saved through autograd: an optimiser step between forward and backward must not give an adjoint solve on
    the new coefficients."""
    from pytorch_sparse_solver.module_a import cg_batch_differentiable
    A = _batch("cg")
    B, W = _rand((S, NP), 1), _rand((S, NP), 4)
    vals = A.values.clone().requires_grad_()
    X = cg_batch_differentiable(A, B, values=vals, tol=1e-9, route="loop")
    with torch.no_grad():
        vals.mul_(1.5)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        (X * W).sum().backward()
