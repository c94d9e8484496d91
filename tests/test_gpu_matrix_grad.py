"""Matrix gradients of the public solves on the GPU: the kernel route (hipk_csr_grad_values on the cached handle of the forward solve,
hipk_batch_grad_values for the batch solves) asserted literally, the values bit for bit against tests/_vgrad_mirror.py applied to the
returned x and an explicitly solved lam, and the whole against an exact gradient computed on the CPU."""
import numpy as np
import pytest
import torch

import _order_cases as OC
import _vgrad_mirror as VM

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _vec(n, seed, dtype=torch.float64):
    return torch.randn(n, dtype=torch.float64, generator=torch.Generator().manual_seed(seed)).to(dtype)


def _csr(crow, col, val, n, device=DEV):
    return torch.sparse_csr_tensor(torch.as_tensor(crow, device=device), torch.as_tensor(col, device=device), torch.as_tensor(val, device=device),
                                   size=(n, n))


def _poisson(nx, ny, dtype=torch.float64):
    from pytorch_sparse_solver.utils.matrix_utils import create_poisson_2d_csr
    return create_poisson_2d_csr(nx, ny, dtype=dtype)


def _convdiff(nx):
    from pytorch_sparse_solver.utils.matrix_utils import create_convdiff_2d_csr
    return create_convdiff_2d_csr(nx, nx)


def _duplicates(A):
    crow, col, val = OC.TRANSFORMS["dup_shuf"](A.crow_indices().numpy(), A.col_indices().numpy(), A.values().numpy(), seed=3)
    return _csr(crow, col, val, A.shape[0], device="cpu")


def _exact(A, b, w):
    """(G at the stored positions, lam, x) in fp64 from a sparse LU of A on the CPU: the dense gradient of torch.linalg.solve up to
    the rounding of a direct solve (1e-14 here), without the n x n matrix (n = 22 500 for the 150 x 150 grid)."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spl
    crow, col = A.crow_indices().numpy(), A.col_indices().numpy()
    n = A.shape[0]
    lu = spl.splu(sp.csr_matrix((A.values().numpy().astype(np.float64), col, crow), shape=(n, n)).tocsc())       # stored twice: summed
    x, lam = lu.solve(b.numpy().astype(np.float64)), lu.solve(w.numpy().astype(np.float64), trans="T")
    rows = np.repeat(np.arange(n), np.diff(crow))
    return -(lam[rows] * x[col]), lam, x


# name -> (solver, CPU matrix, tol, bound).  The bound is ten times the relative deviation (max norm over the stored positions) of
# the CPU solve's gradient from the exact one, measured on CPU with the same b, w (seeds 5, 6) and tol: cg Poisson 17 x 13 2.4e-8;
# cg Poisson 150 x 150 9.7e-9; bicgstab convection-diffusion 32 x 32 3.9e-8 (info = 0); gmres convection-diffusion 32 x 32 3.3e-8;
# cg Poisson 17 x 13 with duplicated columns 2.4e-8.  At tol = 1e-8 the deviation is the truncation error of the stopped iteration,
# which a different summation order on the device does not move by an order of magnitude.
SINGLE = {
    "cg_poisson17x13": ("cg", lambda: _poisson(17, 13), 1e-8, 2.4e-7),
    "cg_poisson150x150": ("cg", lambda: _poisson(150, 150), 1e-8, 9.7e-8),
    "bicgstab_convdiff32": ("bicgstab", lambda: _convdiff(32), 1e-8, 3.9e-7),
    "gmres_convdiff32": ("gmres", lambda: _convdiff(32), 1e-8, 3.3e-7),
    "cg_duplicate_columns": ("cg", lambda: _duplicates(_poisson(17, 13)), 1e-8, 2.4e-7),
}


def _solve_and_check_bits(hipk, kind, Ac, tol, idx=None):
    """The public solve with A and b requiring grad on the device; returns (A.grad values, b.grad, exact G, exact lam) as numpy."""
    from pytorch_sparse_solver import module_a as MA
    solver = getattr(MA, kind)
    n = Ac.shape[0]
    dt = Ac.dtype
    crow, col = Ac.crow_indices(), Ac.col_indices()
    if idx is not None:
        crow, col = crow.to(idx), col.to(idx)
    A = torch.sparse_csr_tensor(crow.to(DEV), col.to(DEV), Ac.values().to(DEV), size=Ac.shape).requires_grad_()
    b, w = _vec(n, 5, dt), _vec(n, 6, dt)
    bd = b.to(DEV).requires_grad_()
    x, info = solver(A, bd, tol=tol)
    assert info == 0
    (x * w.to(DEV)).sum().backward()
    st = MA.get_last_grad_stats()
    assert st.route == "kernel"
    assert (st.launches, st.nnz, st.batch) == (1, col.numel(), 1)
    assert A.grad is not None and A.grad.layout == torch.sparse_csr and A.grad.dtype == dt
    assert torch.equal(A.grad.crow_indices(), A.detach().crow_indices()) and torch.equal(A.grad.col_indices(), A.detach().col_indices())
    lam, _ = solver(A.detach().t(), w.to(DEV), tol=tol)                  # the adjoint solve, made explicitly
    assert torch.equal(bd.grad, lam), "b.grad is not the adjoint solution bit for bit"
    ndt, bits = (np.float64, np.uint64) if dt == torch.float64 else (np.float32, np.uint32)
    want = VM.grad_values_rows(crow.numpy(), col.numpy(), lam.cpu().numpy(), x.detach().cpu().numpy(), ndt)
    got = A.grad.values().cpu().numpy()
    assert got.dtype == want.dtype and np.array_equal(got.view(bits), want.view(bits)), "A.grad differs from the mirror of x and lam"
    if col.numel() <= 20_000:                                            # ... and from the scalar loop itself where that is quick
        loop = VM.grad_values(crow.numpy(), col.numpy(), lam.cpu().numpy(), x.detach().cpu().numpy(), ndt)
        assert np.array_equal(got.view(bits), loop.view(bits))
    G, lam_x, x_x = _exact(Ac, b, w)
    return got, bd.grad.cpu().numpy(), G, lam_x, x_x


@pytest.mark.parametrize("name", sorted(SINGLE))
def test_single_solves_take_the_kernel_and_match_the_mirror_and_the_exact_gradient(hipk, name):
    kind, make, tol, bound = SINGLE[name]
    got, gb, G, lam_x, _ = _solve_and_check_bits(hipk, kind, make(), tol)
    dev = float(np.abs(got - G).max() / np.abs(G).max())
    devb = float(np.abs(gb - lam_x).max() / np.abs(lam_x).max())
    print(f"{name}: deviation from the exact gradient {dev:.3e} (bound {bound:.1e}); of b.grad {devb:.3e}")
    assert dev <= bound


def test_int64_indices_go_through_the_handle_int32_copies(hipk):
    _solve_and_check_bits(hipk, "cg", _poisson(17, 13), 1e-8, idx=torch.int64)
    _solve_and_check_bits(hipk, "cg", _poisson(17, 13), 1e-8, idx=torch.int32)


def test_fp32_matrix(hipk):
    """An fp32 matrix solves in fp32 storage.  The CPU solvers refuse it, so the bound is not a measured one but this: with kappa the
    2-norm condition number of A (99 for the 17 x 13 grid), a solve stopped at ||b - A x|| <= tol ||b|| has ||dx|| <= kappa tol ||x||,
    where the residual test itself is evaluated in fp32 (allow 32 eps32 for a 5-entry row sum and the norm).  The same holds for lam.
    Then ||dG||_F over ANY set of positions is at most (e_lam + e_x + e_lam e_x) ||lam|| ||x|| with e = kappa (tol + 32 eps32), plus
    the casts and the one multiplication in fp32 (3 eps32).  So the deviation is taken in that norm: ||G - G_exact||_2 over the
    stored positions, divided by ||lam||_2 ||x||_2."""
    tol, eps = 1e-5, float(np.finfo(np.float32).eps)
    Ac = _poisson(17, 13, dtype=torch.float32)
    got, _, G, lam_x, x_x = _solve_and_check_bits(hipk, "cg", Ac, tol)
    assert got.dtype == np.float32
    kappa = float(torch.linalg.cond(Ac.to_dense().double()))
    e = kappa * (tol + 32 * eps)
    bound = 2 * e + e * e + 3 * eps
    dev = float(np.linalg.norm(got.astype(np.float64) - G) / (np.linalg.norm(lam_x) * np.linalg.norm(x_x)))
    print(f"fp32: kappa {kappa:.1f}, deviation {dev:.3e} (bound {bound:.3e})")
    assert dev <= bound


def test_only_the_matrix_requires_grad(hipk):
    from pytorch_sparse_solver.module_a import cg_differentiable, get_last_grad_stats
    Ac = _poisson(17, 13)
    A = Ac.to(DEV).requires_grad_()
    b, w = _vec(221, 5).to(DEV), _vec(221, 6).to(DEV)
    x = cg_differentiable(A, b, tol=1e-8)
    (x * w).sum().backward()
    assert get_last_grad_stats().route == "kernel" and b.grad is None
    from pytorch_sparse_solver.module_a import cg
    lam, _ = cg(A.detach().t(), w, tol=1e-8)
    want = VM.grad_values(Ac.crow_indices().numpy(), Ac.col_indices().numpy(), lam.cpu().numpy(), x.detach().cpu().numpy(), np.float64)
    assert np.array_equal(A.grad.values().cpu().numpy().view(np.uint64), want.view(np.uint64))


# ------------------------------------------------------------------------------------------------ batch solves
S = 12


def _batch(kind, nx, ny):
    """S systems on one grid pattern: the Poisson matrix (cg) or the convection-diffusion matrix, the diagonal raised by 0.1 (s + 1)."""
    from pytorch_sparse_solver.module_a import BatchedCSR
    from pytorch_sparse_solver.utils.matrix_utils import create_convdiff_2d_csr
    A0 = _poisson(nx, ny) if kind == "cg" else create_convdiff_2d_csr(nx, ny)
    crow, col, val = A0.crow_indices(), A0.col_indices(), A0.values()
    rows = torch.repeat_interleave(torch.arange(nx * ny), crow[1:] - crow[:-1])
    vals = val.repeat(S, 1)
    vals[:, rows == col] += 0.1 * torch.arange(1, S + 1, dtype=torch.float64)[:, None]
    return BatchedCSR(crow.to(DEV), col.to(DEV), vals.to(DEV))


def _precond(A, which):
    from pytorch_sparse_solver.module_a import BatchedBlockJacobiPreconditioner, BatchedJacobiPreconditioner
    return {"none": lambda: None, "jacobi": lambda: BatchedJacobiPreconditioner(A), "bj": lambda: BatchedBlockJacobiPreconditioner(A, 4)}[which]()


@pytest.mark.parametrize("grid", [(7, 5), (32, 32)])
@pytest.mark.parametrize("precond", ["none", "jacobi", "bj"])
@pytest.mark.parametrize("kind", ["cg", "bicgstab", "gmres"])
def test_batch_differentiable_solves(hipk, kind, precond, grid):
    from pytorch_sparse_solver import module_a as MA
    plain, diff = getattr(MA, f"{kind}_batch"), getattr(MA, f"{kind}_batch_differentiable")
    A = _batch(kind, *grid)
    M = _precond(A, precond)
    n = A.n
    B = torch.randn((S, n), dtype=torch.float64, generator=torch.Generator().manual_seed(1)).to(DEV)
    W = torch.randn((S, n), dtype=torch.float64, generator=torch.Generator().manual_seed(4)).to(DEV)
    fast = "auto" if (kind == "gmres" and precond == "bj") else "kernel"       # the GMRES batch kernel has no block-Jacobi form
    grads = {}
    for route in (fast, "loop"):
        X0, _ = plain(A, B, tol=1e-8, M=M, route=route)
        path = MA.get_last_stats().path
        vals, Bb = A.values.clone().requires_grad_(), B.clone().requires_grad_()
        X = diff(A, Bb, values=vals, tol=1e-8, M=M, route=route)
        assert MA.get_last_stats().path == path and (path != "loop") == (route == "kernel")
        assert torch.equal(X.detach(), X0), f"route {route}: X is not the plain batch solve bit for bit"
        (X * W).sum().backward()
        st = MA.get_last_grad_stats()
        assert st.route == "kernel"
        assert (st.launches, st.nnz, st.batch) == (1, A.nnz, S)
        assert tuple(vals.grad.shape) == (S, A.nnz) and vals.grad.is_contiguous()
        grads[route] = (vals.grad, Bb.grad, X.detach())
    assert torch.equal(grads[fast][0], grads["loop"][0]) and torch.equal(grads[fast][1], grads["loop"][1])
    Mt = M.transposed() if precond == "bj" else M
    Lam, _ = plain(A.transposed(), W, tol=1e-8, M=Mt, route=fast)
    gv, gb, X = grads[fast]
    assert torch.equal(gb, Lam), "grad_B is not the transposed batch solve bit for bit"
    want = VM.batch_grad_values(A.crow.cpu().numpy(), A.col.cpu().numpy(), Lam.cpu().numpy(), X.cpu().numpy(), np.float64, fast=True)
    assert np.array_equal(gv.cpu().numpy().view(np.uint64), want.view(np.uint64)), "grad_values differ from the mirror"
    if grid == (7, 5):
        loop = VM.batch_grad_values(A.crow.cpu().numpy(), A.col.cpu().numpy(), Lam.cpu().numpy(), X.cpu().numpy(), np.float64)
        assert np.array_equal(want.view(np.uint64), loop.view(np.uint64))


def test_batch_values_none_with_only_b_requiring_grad(hipk):
    from pytorch_sparse_solver.module_a import cg_batch, cg_batch_differentiable
    A = _batch("cg", 7, 5)
    B = torch.randn((S, 35), dtype=torch.float64, generator=torch.Generator().manual_seed(1)).to(DEV).requires_grad_()
    W = torch.randn((S, 35), dtype=torch.float64, generator=torch.Generator().manual_seed(4)).to(DEV)
    X = cg_batch_differentiable(A, B, tol=1e-8, route="kernel")
    (X * W).sum().backward()
    Lam, _ = cg_batch(A.transposed(), W, tol=1e-8, route="kernel")
    assert torch.equal(B.grad, Lam) and A.values.grad is None


def test_kernel_route_backward_when_a_column_is_longer_than_the_envelope(hipk):
    """Rows of 1 or 2 entries, column 0 with 64: the forward takes the batch kernel, the transposed pattern has a row of 64 entries,
    which the kernel refuses, so the adjoint solve picks its own route instead of failing in backward."""
    from pytorch_sparse_solver import module_a as MA
    n = 64
    crow = torch.cat([torch.tensor([0, 1]), 1 + 2 * torch.arange(1, n)])
    col = torch.cat([torch.tensor([0])] + [torch.tensor([0, r]) for r in range(1, n)])
    g = torch.Generator().manual_seed(8)
    vals = torch.where(col == torch.repeat_interleave(torch.arange(n), crow[1:] - crow[:-1]), 4.0 + torch.rand((S, col.numel()), generator=g, dtype=torch.float64),
                       0.05 * torch.rand((S, col.numel()), generator=g, dtype=torch.float64))
    A = MA.BatchedCSR(crow.to(DEV), col.to(DEV), vals.to(DEV))
    assert A.in_envelope() and not A.transposed().in_envelope()
    B = torch.randn((S, n), dtype=torch.float64, generator=g).to(DEV)
    W = torch.randn((S, n), dtype=torch.float64, generator=g).to(DEV)
    v, Bb = A.values.clone().requires_grad_(), B.clone().requires_grad_()
    X = MA.bicgstab_batch_differentiable(A, Bb, values=v, tol=1e-10, route="kernel")
    assert MA.get_last_stats().path != "loop"
    (X * W).sum().backward()
    assert MA.get_last_stats().path == "loop" and MA.get_last_grad_stats().route == "kernel"
    Lam, _ = MA.bicgstab_batch(A.transposed(), W, tol=1e-10, route="loop")
    assert torch.equal(Bb.grad, Lam)
    want = VM.batch_grad_values(crow.numpy(), col.numpy(), Lam.cpu().numpy(), X.detach().cpu().numpy(), np.float64)
    assert np.array_equal(v.grad.cpu().numpy().view(np.uint64), want.view(np.uint64))
