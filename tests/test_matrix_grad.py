"""dL/dA of cg / bicgstab / gmres and the three *_differentiable functions on CPU tensors (module_a/matrix_grad.py; no GPU).

Before this feature `A.grad` stayed None after backward through a solve with a matrix that requires grad.  Now, with x the returned
solution, g = dL/dx and lam the adjoint solution A^-T g, every stored entry k of A gets G[k] = -(lam[row(k)] * x[col(k)]) and
b.grad = lam.  The values are checked bit for bit against tests/_vgrad_mirror.py applied to the returned x and to lam from an explicit
public solve with the transposed matrix, then against the dense gradient of torch.linalg.solve."""
import numpy as np
import pytest
import torch

import _order_cases as OC
import _vgrad_mirror as VM

N = 63   # the 9 x 7 grid


def _vec(seed):
    return torch.randn(N, dtype=torch.float64, generator=torch.Generator().manual_seed(seed))


B, W = _vec(5), _vec(6)


def _matrix(kind):
    from pytorch_sparse_solver.utils.matrix_utils import create_convdiff_2d_csr, create_variable_diffusion_2d_csr
    return create_variable_diffusion_2d_csr(9, 7) if kind == "cg" else create_convdiff_2d_csr(9, 7)


def _solvers():
    from pytorch_sparse_solver import module_a as MA
    return {"cg": MA.cg, "bicgstab": MA.bicgstab, "gmres": MA.gmres}


def _solve(name, A, b, x0=None, tol=1e-10):
    """x of the public solver `name` ('cg' ... or 'cg_differentiable' ...)."""
    from pytorch_sparse_solver import module_a as MA
    if name.endswith("_differentiable"):
        return getattr(MA, name)(A, b, x0, tol=tol)
    return getattr(MA, name)(A, b, x0, tol=tol)[0]


def _form(A, form):
    A = A.detach()
    return {"csr": lambda: torch.sparse_csr_tensor(A.crow_indices().clone(), A.col_indices().clone(), A.values().clone(), size=A.shape),
            "coo": lambda: A.to_sparse_coo(), "dense": lambda: A.to_dense()}[form]()


def _transposed(A):
    A = A.detach()
    return A.T if A.layout == torch.strided else A.t()


def _pattern(A, form):
    """crow, col of the stored entries in the order the gradient lists them (dense: every (i, j), row-major)."""
    if form == "dense":
        n = A.shape[0]
        return np.arange(0, n * n + 1, n), np.tile(np.arange(n), n)
    return A.crow_indices().numpy(), A.col_indices().numpy()


def _grad_values(G, form):
    if form == "csr":
        assert G.layout == torch.sparse_csr
        return G.values().numpy()
    if form == "coo":
        assert G.layout == torch.sparse_coo
        return G._values().numpy()
    assert G.layout == torch.strided
    return G.reshape(-1).numpy()


SOLVERS = ["cg", "bicgstab", "gmres", "cg_differentiable", "bicgstab_differentiable", "gmres_differentiable"]


@pytest.mark.parametrize("which", ["A", "b", "both"])
@pytest.mark.parametrize("form", ["csr", "coo", "dense"])
@pytest.mark.parametrize("name", SOLVERS)
def test_gradients_are_the_mirror_of_x_and_the_explicit_adjoint_solve(name, form, which):
    kind = name.split("_")[0]
    A0 = _matrix(kind)
    A = _form(A0, form).requires_grad_(which in ("A", "both"))
    b = B.clone().requires_grad_(which in ("b", "both"))
    x = _solve(name, A, b)
    (x * W).sum().backward()
    lam = _solve(kind, _transposed(A), W.clone())          # the adjoint solve, made explicitly through the public solver
    if which in ("b", "both"):
        assert torch.equal(b.grad, lam), "b.grad is not the adjoint solution bit for bit"
    else:
        assert b.grad is None
    if which == "b":
        assert A.grad is None
        return
    assert A.grad is not None, "A.grad is None: the solve returned no gradient for the matrix"
    assert A.grad.layout == A.layout and A.grad.dtype == A.dtype and tuple(A.grad.shape) == tuple(A.shape)
    crow, col = _pattern(A0, form)
    want = VM.grad_values(crow, col, lam.numpy(), x.detach().numpy(), np.float64)
    got = _grad_values(A.grad, form)
    assert got.shape == want.shape and np.array_equal(got.view(np.uint64), want.view(np.uint64))
    if form == "coo":
        assert torch.equal(A.grad._indices(), A.detach()._indices())
    if form == "csr":
        assert torch.equal(A.grad.crow_indices(), A0.crow_indices()) and torch.equal(A.grad.col_indices(), A0.col_indices())


def test_csr_gradient_is_built_on_the_matrix_own_index_tensors():
    from pytorch_sparse_solver.module_a import cg, get_last_grad_stats
    A = _form(_matrix("cg"), "csr").requires_grad_()
    x, _ = cg(A, B, tol=1e-10)
    (G,) = torch.autograd.grad((x * W).sum(), A)
    assert G.crow_indices().data_ptr() == A.crow_indices().data_ptr() and G.col_indices().data_ptr() == A.col_indices().data_ptr()
    st = get_last_grad_stats()
    assert (st.route, st.launches, st.nnz, st.batch) == ("torch", 0, A.col_indices().numel(), 1)


def test_the_x0_of_the_forward_goes_to_the_adjoint_solve_as_in_the_reference():
    from pytorch_sparse_solver.module_a import cg
    A = _form(_matrix("cg"), "csr").requires_grad_()
    b = B.clone().requires_grad_()
    x0 = _vec(7)
    x, _ = cg(A, b, x0, tol=1e-10)
    (x * W).sum().backward()
    lam, _ = cg(_transposed(A), W.clone(), x0, tol=1e-10)
    assert torch.equal(b.grad, lam)
    want = VM.grad_values(A.crow_indices().numpy(), A.col_indices().numpy(), lam.numpy(), x.detach().numpy(), np.float64)
    assert np.array_equal(A.grad.values().numpy().view(np.uint64), want.view(np.uint64))


def test_values_as_the_leaf():
    from pytorch_sparse_solver.module_a import cg
    A0 = _matrix("cg")
    vals = A0.values().clone().requires_grad_()
    A = torch.sparse_csr_tensor(A0.crow_indices(), A0.col_indices(), vals, size=A0.shape)
    x, _ = cg(A, B, tol=1e-10)
    (x * W).sum().backward()
    lam, _ = cg(A0.t(), W.clone(), tol=1e-10)
    want = VM.grad_values(A0.crow_indices().numpy(), A0.col_indices().numpy(), lam.numpy(), x.detach().numpy(), np.float64)
    assert vals.grad is not None and vals.grad.layout == torch.strided
    assert np.array_equal(vals.grad.numpy().view(np.uint64), want.view(np.uint64))


@pytest.mark.parametrize("transform", ["dup", "dup_shuf", "zero"])
@pytest.mark.parametrize("kind", ["cg", "gmres"])
def test_a_column_stored_twice_and_a_stored_zero(kind, transform):
    A0 = _matrix(kind)
    crow, col, val = OC.TRANSFORMS[transform](A0.crow_indices().numpy(), A0.col_indices().numpy(), A0.values().numpy(), seed=3)
    assert len(col) > A0.col_indices().numel()
    if transform == "zero":
        assert (val == 0).any()
    A = torch.sparse_csr_tensor(torch.from_numpy(crow), torch.from_numpy(col), torch.from_numpy(val), size=A0.shape).requires_grad_()
    b = B.clone().requires_grad_()
    x = _solve(kind, A, b)
    (x * W).sum().backward()
    lam = _solve(kind, _transposed(A), W.clone())
    assert torch.equal(b.grad, lam)
    want = VM.grad_values(crow, col, lam.numpy(), x.detach().numpy(), np.float64)
    got = A.grad.values().numpy()
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert np.all(got[val == 0] != 0) or transform != "zero"      # a stored zero gets a gradient like any other entry
    # the dense gradient sums the two halves of a split entry: each half carries the whole dL/dA_ij.  Both solves stop at a relative
    # residual of 1e-10 and both 63 x 63 matrices have condition numbers below 1e3, so x and lam are within 1e-7 of the exact
    # solutions and their products within 2e-7: 1e-6 tells "the whole value" from "a quarter of it" with five digits to spare
    Ad = A.detach().to_dense().requires_grad_()
    (torch.linalg.solve(Ad, B) * W).sum().backward()
    rows = np.repeat(np.arange(N), np.diff(crow))
    ref = Ad.grad.numpy()[rows, col]
    assert np.abs(got - ref).max() <= 1e-6 * np.abs(ref).max()


@pytest.mark.parametrize("form", ["csr", "coo", "dense"])
def test_fp32_matrices_get_an_fp32_gradient_from_operands_cast_first(form):
    """The CPU solvers promote b to fp64 and refuse an fp32 matrix in their matvec (as the reference does), so the expression is
    called as backward calls it: fp64 lam and x, cast to the matrix dtype before the one multiplication."""
    from pytorch_sparse_solver.module_a import matrix_grad
    A0 = _matrix("gmres")
    A = _form(A0, form).to(torch.float32)
    lam, x = _vec(11), _vec(12)
    G = matrix_grad.matrix_grad(A, lam, x)
    assert G.dtype == torch.float32 and G.layout == A.layout
    crow, col = _pattern(A0, form)
    want = VM.grad_values(crow, col, lam.numpy(), x.numpy(), np.float32)
    assert np.array_equal(_grad_values(G, form).view(np.uint32), want.view(np.uint32))


def test_the_row_sliced_mirror_is_the_scalar_loop():
    rng = np.random.default_rng(8)
    lens = rng.integers(0, 9, 300)
    lens[[0, 17, 18, 299]] = 0
    crow = np.concatenate([[0], np.cumsum(lens)])
    col = rng.integers(0, 200, crow[-1])
    lam, x = rng.standard_normal(300), rng.standard_normal(200)
    lam[5], x[3], x[4] = np.inf, -0.0, 0.0
    for dt, bits in ((np.float64, np.uint64), (np.float32, np.uint32)):
        a, b = VM.grad_values(crow, col, lam, x, dt), VM.grad_values_rows(crow, col, lam, x, dt)
        assert a.dtype == b.dtype == dt and np.array_equal(a.view(bits), b.view(bits))


def test_sparse_solver_solve_returns_the_matrix_gradient():
    from pytorch_sparse_solver.solver import SparseSolver
    A = _form(_matrix("cg"), "csr").requires_grad_()
    b = B.clone().requires_grad_()
    x, res = SparseSolver().solve(A, b, method="cg", backend="module_a", tol=1e-10)
    assert res.converged
    (x * W).sum().backward()
    lam = _solve("cg", _transposed(A), W.clone())
    want = VM.grad_values(A.crow_indices().numpy(), A.col_indices().numpy(), lam.numpy(), x.detach().numpy(), np.float64)
    assert np.array_equal(A.grad.values().numpy().view(np.uint64), want.view(np.uint64)) and torch.equal(b.grad, lam)


def test_complex_and_callable_operators_are_unchanged():
    from pytorch_sparse_solver.module_a import gmres
    Ad = _matrix("gmres").to_dense()
    Ac = (Ad + 0.1j * torch.eye(N, dtype=torch.float64)).requires_grad_()
    b = (B + 0j).requires_grad_()
    x, info = gmres(Ac, b, tol=1e-10)
    assert info == 0
    (x * W).sum().abs().backward()
    assert Ac.grad is None and b.grad is not None
    b2 = B.clone().requires_grad_()
    x, info = gmres(lambda v: Ad @ v, b2, tol=1e-10)       # a callable operator takes no implicit-function backward
    assert info == 0 and isinstance(x, torch.Tensor)


def _dense_reference(A):
    Ad = A.detach().to_dense().requires_grad_()
    (torch.linalg.solve(Ad, B) * W).sum().backward()
    rows = torch.repeat_interleave(torch.arange(N), A.crow_indices()[1:] - A.crow_indices()[:-1])
    return Ad.grad[rows, A.col_indices()]


# solver, tol, bound = 10 x the deviation measured on CPU (the docstring below)
DENSE = [("cg", 1e-12, 1.06e-13), ("gmres", 1e-12, 1.02e-14), ("bicgstab", 1e-10, 1.28e-7)]


@pytest.mark.parametrize("kind,tol,bound", DENSE)
def test_against_the_dense_gradient_of_torch_linalg_solve(kind, tol, bound):
    """max |G - G_dense| / max |G_dense| over the stored positions, G_dense from autograd through torch.linalg.solve.  Measured on
    CPU by this test itself (it prints the figure) with B, W of seeds 5 and 6, the same with 1 and 4 threads: cg (variable diffusion
    9 x 7, tol 1e-12) 1.059e-14; gmres (convection-diffusion 9 x 7, tol 1e-12) 1.016e-15; bicgstab (convection-diffusion 9 x 7)
    1.279e-8 at tol 1e-10, the tightest tol at which the CPU solve returns info = 0 (3e-11, 1e-11 and 1e-12 stagnate: info = -1).
    The bound is ten times the measured value, for platform differences in torch's dense solve."""
    A = _form(_matrix(kind), "csr").requires_grad_()
    x, info = _solvers()[kind](A, B, tol=tol)
    assert info == 0
    (x * W).sum().backward()
    ref = _dense_reference(A)
    dev = float((A.grad.values() - ref).abs().max() / ref.abs().max())
    print(f"{kind}: relative deviation from the dense gradient {dev:.3e} (bound {bound:.1e})")
    assert dev <= bound
