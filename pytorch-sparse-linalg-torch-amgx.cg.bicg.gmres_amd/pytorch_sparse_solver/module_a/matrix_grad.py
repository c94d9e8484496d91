"""dL/dA of a linear solve, on A's own sparsity pattern.

With x = A^-1 b, g = dL/dx and lam = A^-T g (the adjoint solve the backward pass makes anyway: dL/db = lam), the gradient with respect
to the stored entry k of A, in row row(k) and column col(k), is

    G[k] = -(lam[row(k)] * x[col(k)])

one multiplication in the dtype of A's values (lam and x are cast to it first), then a negation.  x is the solution the forward solve
returned, whatever its `info`.  A column stored twice in a row gives both entries the same value, a stored zero gets a gradient like
any other entry, and the result has A's pattern: nothing is symmetrised, for cg either.

| A                         | gradient                                                                     |
|---------------------------|------------------------------------------------------------------------------|
| sparse CSR                | sparse CSR on A's own crow_indices() / col_indices() tensors                 |
| sparse COO                | sparse COO on A's stored index list (coalesced or not, as A is)              |
| strided                   | -torch.outer(lam, x)                                                         |
| complex, other layouts    | none (as before)                                                             |

A real fp32 / fp64 CSR matrix on the device takes hipk_csr_grad_values (csrc/hipk_vgrad.hip) on the cached handle of the forward
solve -- int64 indices through the handle's int32 copies; everything else, CPU tensors included, the torch expression of the same
formula below.  `get_last_grad_stats()` says which route the last gradient took.
"""
from __future__ import annotations

from typing import Optional

import torch


def get_last_grad_stats():
    """`GradStats(route, launches, nnz, batch)` of the most recent matrix gradient formed in this process, or None.  Module-level,
    not thread-local: autograd runs backward on a thread of its own."""
    from .. import _hipk
    return _hipk.last_grad_stats()


def supported(A) -> bool:
    """Whether a solve with `A` gives a matrix gradient (the table above)."""
    return (isinstance(A, torch.Tensor) and A.dim() == 2 and not torch.is_complex(A) and A.dtype.is_floating_point
            and A.layout in (torch.sparse_csr, torch.sparse_coo, torch.strided))


def csr_rows(crow: torch.Tensor) -> torch.Tensor:
    """row(k) of every stored entry of a CSR pattern."""
    n = crow.numel() - 1
    return torch.repeat_interleave(torch.arange(n, device=crow.device), (crow[1:] - crow[:-1]).to(torch.int64))


def grad_values_torch(rows: torch.Tensor, cols: torch.Tensor, lam: torch.Tensor, x: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """The formula as a torch expression: lam, x of shape (n,) or (S, n) -> values of shape (nnz,) or (S, nnz)."""
    lam, x = lam.to(dtype), x.to(dtype)
    return -(lam.index_select(-1, rows) * x.index_select(-1, cols.to(torch.int64)))


def _kernel_ok(A: torch.Tensor) -> bool:
    return A.layout == torch.sparse_csr and A.is_cuda and A.dtype in (torch.float64, torch.float32)


def matrix_grad(A: torch.Tensor, lam: torch.Tensor, x: torch.Tensor) -> Optional[torch.Tensor]:
    """The gradient of the table above for `A` (detached here), from the adjoint solution `lam` and the forward solution `x`."""
    from .. import _hipk
    if not supported(A):
        return None
    A = A.detach()
    lam, x = lam.detach().reshape(-1), x.detach().reshape(-1)
    if A.layout == torch.strided:
        _hipk.set_grad_stats("torch", 0, A.numel(), 1)
        return -torch.outer(lam.to(A.dtype), x.to(A.dtype))
    if A.layout == torch.sparse_coo:
        idx = A._indices()
        vals = grad_values_torch(idx[0], idx[1], lam, x, A.dtype)
        _hipk.set_grad_stats("torch", 0, vals.numel(), 1)
        return torch.sparse_coo_tensor(idx, vals, A.shape, is_coalesced=A.is_coalesced())
    crow, col = A.crow_indices(), A.col_indices()
    if _kernel_ok(A):
        vals = _hipk.csr_grad_values(_hipk.handle_for(A), lam, x)      # the handle of the forward solve (cached); fills the stats
    else:
        vals = grad_values_torch(csr_rows(crow), col, lam, x, A.dtype)
        _hipk.set_grad_stats("torch", 0, vals.numel(), 1)
    return torch.sparse_csr_tensor(crow, col, vals, size=A.shape, check_invariants=False)
