"""cg_multi / bicgstab_multi: k right-hand sides on one matrix.

Column j of the result is what `cg(A, B[:, j], X0[:, j], ...)` (or `bicgstab`) returns, bit for bit, and `info[j]` its info.
`_block_solve` runs the block launch sequence of libhipk.so (csrc/hipk_multi.hip) on a real CUDA/ROCm matrix (CSR, COO or
dense) with device `B` and `M` None or a `JacobiPreconditioner`: blocks of at most 16 columns, the matrix read once per block
iteration for all of them, every column stopping at its own iteration.  As measured so far it is slower than the column loop for
every class of handle (routing comment in `_multi`), so `cg_multi` / `bicgstab_multi` run a plain loop over the columns through
`cg` / `bicgstab` -- with exactly their behaviour and their bits -- for device operands as for everything else (CPU tensors,
callable `A`, other `M`, PyTrees, complex).
"""
from __future__ import annotations

import time
from typing import Any, Callable, Optional, Tuple, Union

import torch

from .torch_sparse_linalg import _identity, _jacobi_of, _set_stats, bicgstab, cg, get_last_stats
from .torch_tree_util import tree_flatten, tree_leaves, tree_map, tree_unflatten


def _requires_grad(x) -> bool:
    if x is None or callable(x) and not isinstance(x, torch.Tensor):
        return False
    return any(isinstance(l, torch.Tensor) and l.requires_grad for l in tree_leaves(x))


def _block_ok(A, B, X0, M) -> bool:
    """The HIP block path: the conditions of the single solves' fast path, with a 2-D B."""
    return (isinstance(A, torch.Tensor) and A.is_cuda and A.ndim == 2 and not torch.is_complex(A)
            and A.dtype in (torch.float64, torch.float32)
            and isinstance(B, torch.Tensor) and B.is_cuda and B.device == A.device and not torch.is_complex(B)
            and (X0 is None or (isinstance(X0, torch.Tensor) and X0.device == B.device and not torch.is_complex(X0)))
            and (M is None or M is _identity or _jacobi_of(M) is not None))


def _check_device_operands(A, B, X0):
    if A.shape[0] != A.shape[1]:
        raise ValueError(f'linear operator must be a square matrix, but has shape: {A.shape}')
    if X0 is not None and X0.shape != B.shape:
        raise ValueError(f'arrays in x0 and b must have matching shapes: {X0.shape} vs {B.shape}')
    if A.shape[1] != B.shape[0]:
        raise RuntimeError(f'size mismatch, got input ({A.shape[0]}x{A.shape[1]}), vec ({B.shape[0]})')


def _block_solve(kind: str, A, B, X0, tol, atol, maxiter, M):
    """The block launch sequence of libhipk.so (hipk_{cg,bicgstab}_solve_multi) on device operands (`_block_ok`)."""
    from .. import _hipk

    _check_device_operands(A, B, X0)
    h = _hipk.handle_for(A)  # raises HipkError when libhipk.so is missing: no fallback
    work_dtype = torch.float64 if h.dtype == torch.float64 else torch.float32   # as _fast_solve
    BB = _hipk.aligned(B.detach().to(work_dtype))
    X = torch.zeros_like(BB) if X0 is None else _hipk.aligned(X0.detach().to(work_dtype).clone())
    dinv = None
    jac = _jacobi_of(M)
    if jac is not None:
        if jac.shape != tuple(A.shape):
            raise ValueError(f'preconditioner shape {jac.shape} does not match the operator {tuple(A.shape)}')
        dinv = _hipk.aligned(jac.dinv.detach().to(device=BB.device, dtype=work_dtype))
    st = _hipk.solve_multi(kind, h, dinv, BB, X, tol=tol, atol=atol, maxiter=maxiter)
    _set_stats(st)
    return X, torch.tensor([c.info for c in st.columns], dtype=torch.int64)


def _column_loop(kind: str, A, B, X0, tol, atol, maxiter, M):
    from .. import _hipk

    solver = cg if kind == 'cg' else bicgstab
    k = tree_leaves(B)[0].shape[1]
    xs, infos, stats = [], [], []
    t0 = time.perf_counter()
    for j in range(k):
        # copies of the columns: the values of B[:, j], contiguous and aligned as the device path of the single solves needs
        bj = tree_map(lambda l: l[:, j].clone(), B)
        xj = None if X0 is None else tree_map(lambda l: l[:, j].clone(), X0)
        x, info = solver(A, bj, xj, tol=tol, atol=atol, maxiter=maxiter, M=M)
        xs.append(x)
        infos.append(int(info))
        stats.append(get_last_stats())
    ms = (time.perf_counter() - t0) * 1e3
    leaves0, treedef = tree_flatten(xs[0])
    per_col = [tree_leaves(x) for x in xs]
    X = tree_unflatten(treedef, [torch.stack([c[i] for c in per_col], dim=1) for i in range(len(leaves0))])
    _set_stats(_hipk.MultiSolveStats(method=f'{kind}_multi', columns=stats, block_spmvs=0, solve_ms=ms))
    return X, torch.tensor(infos, dtype=torch.int64)


def _multi(kind: str, A, B, X0, tol, atol, maxiter, M):
    name = f'{kind}_multi'
    if (isinstance(A, torch.Tensor) and A.requires_grad) or _requires_grad(B) or _requires_grad(X0):
        raise ValueError(f'{name} is not differentiable: call {kind}_differentiable on each column instead')
    leaves = tree_leaves(B)
    if not leaves:
        raise ValueError(f'{name}: B must have shape (n, k), got an empty tree')
    for l in leaves:
        if not isinstance(l, torch.Tensor) or l.ndim != 2 or l.shape[1] < 1:
            raise ValueError(f'{name}: B must have shape (n, k) with k >= 1, got {tuple(getattr(l, "shape", ()))}')
    k = leaves[0].shape[1]
    if any(l.shape[1] != k for l in leaves):
        raise ValueError(f'{name}: every leaf of B must have the same number of columns k')
    if isinstance(B, torch.Tensor) and _block_ok(A, B, X0, M):
        _check_device_operands(A, B, X0)
        # Routing (tools/multi_rhs_probe.py, one MI355X, CG, 60-400 iterations per column, k = 1..16): the block launch sequence
        # reached 0.62-0.77x of the column loop's column-iterations per second on general CSR at N = 4 M, 0.20-0.46x with the
        # coded form, 0.22-0.58x at n = 40 k and 0.18-0.47x at n = 250 k -- slower for every class of handle measured, so every
        # device operand takes the column loop (bitwise the same result); _block_solve stays reachable for the tests and the probe.
        return _column_loop(kind, A, B, X0, tol, atol, maxiter, M)
    if X0 is not None:
        for bl, xl in zip(leaves, tree_leaves(X0)):
            if not isinstance(xl, torch.Tensor) or xl.shape != bl.shape:
                raise ValueError(f'arrays in x0 and b must have matching shapes: {tuple(getattr(xl, "shape", ()))} vs {tuple(bl.shape)}')
    return _column_loop(kind, A, B, X0, tol, atol, maxiter, M)


def cg_multi(A: Union[torch.Tensor, Callable[[Any], Any]], B: Any, X0: Optional[Any] = None,
             *, tol: float = 1e-5, atol: float = 0.0, maxiter: Optional[int] = None,
             M: Optional[Callable[[Any], Any]] = None) -> Tuple[Any, torch.Tensor]:
    """Conjugate gradients for the k systems A X[:, j] = B[:, j], B of shape (n, k).

    Returns `(X, info)`: X of shape (n, k) (fp64; fp32 when a device `A` is fp32), info a 1-D int64 CPU tensor of length k with
    `info[j]` = the info of `cg(A, B[:, j], X0[:, j], ...)`.  `get_last_stats()` is then a `MultiSolveStats`.  Not differentiable.
    """
    return _multi('cg', A, B, X0, tol, atol, maxiter, M)


def bicgstab_multi(A: Union[torch.Tensor, Callable[[Any], Any]], B: Any, X0: Optional[Any] = None,
                   *, tol: float = 1e-5, atol: float = 0.0, maxiter: Optional[int] = None,
                   M: Optional[Callable[[Any], Any]] = None) -> Tuple[Any, torch.Tensor]:
    """BiCGStab for the k systems A X[:, j] = B[:, j] (see `cg_multi`); breakdowns (-10, -11) are decided per column."""
    return _multi('bicgstab', A, B, X0, tol, atol, maxiter, M)
