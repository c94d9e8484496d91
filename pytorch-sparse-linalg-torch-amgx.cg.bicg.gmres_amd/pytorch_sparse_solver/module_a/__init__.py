"""Module A: JAX-style iterative solvers (cg, bicgstab, gmres), MI355X-native.

Same exports as the reference's `module_a/__init__.py:47-63`; CUDA/ROCm tensor inputs run
on hand-written gfx950 kernels (libhipk.so), everything else on the generic torch path.
`get_last_stats()` (iteration counts the reference never returns), `JacobiPreconditioner` (a callable for the
reference's `M` hook that the fast path runs device-resident), `ChebyshevPreconditioner` (a polynomial in D^-1 A whose steps
run in the SpMV kernels' epilogue), `AggregationMultigridPreconditioner` (a V-cycle of aggregation multigrid for a matrix on a
structured grid or, `from_graph`, for any matrix, with `pairwise_aggregates` from the matrix graph), `cg_multi` / `bicgstab_multi` (k right-hand sides per matrix read) and `cg_batch` /
`bicgstab_batch` / `gmres_batch` (many small systems with one sparsity pattern, one workgroup per system; point- or block-Jacobi
preconditioned) are the additions, and so are matrix gradients: a solve through a real CSR, COO or dense `A` that requires grad
returns dL/dA on A's pattern (module_a/matrix_grad.py, `get_last_grad_stats()`), and `cg_batch_differentiable` /
`bicgstab_batch_differentiable` / `gmres_batch_differentiable` differentiate the batch solves with respect to per-system values.
"""
from .torch_sparse_linalg import (
    cg, bicgstab, gmres,
    cg_differentiable, bicgstab_differentiable, gmres_differentiable,
    LinearSolveFunction, ImplicitAdjointFunction, get_last_stats,
)
from .multi_rhs import cg_multi, bicgstab_multi
from .batch import BatchedCSR, BatchedJacobiPreconditioner, BatchedBlockJacobiPreconditioner, cg_batch, bicgstab_batch, gmres_batch
from .batch import cg_batch_differentiable, bicgstab_batch_differentiable, gmres_batch_differentiable
from .matrix_grad import get_last_grad_stats
from .torch_tree_util import tree_leaves, tree_map, tree_flatten, tree_unflatten, Partial
from .preconditioners import BlockJacobiPreconditioner, ChebyshevPreconditioner, JacobiPreconditioner
from .multigrid import AggregationMultigridPreconditioner, pairwise_aggregates


def refresh_matrix(A, like=None) -> bool:
    """New values on the pattern of a matrix the solvers have seen: the cached handle of `A` (changed in place), or of `like`
    (a CSR tensor whose index tensors `A` shares), takes A's values instead of being rebuilt by the next solve.  True when a
    handle was updated, False when there was none (the next solve then builds one as always).  See `_hipk.refresh_matrix`."""
    from .. import _hipk
    return _hipk.refresh_matrix(A, like)


__all__ = [
    'refresh_matrix',
    'cg', 'bicgstab', 'gmres', 'cg_multi', 'bicgstab_multi',
    'BatchedCSR', 'BatchedJacobiPreconditioner', 'BatchedBlockJacobiPreconditioner', 'cg_batch', 'bicgstab_batch', 'gmres_batch',
    'cg_differentiable', 'bicgstab_differentiable', 'gmres_differentiable',
    'cg_batch_differentiable', 'bicgstab_batch_differentiable', 'gmres_batch_differentiable', 'get_last_grad_stats',
    'LinearSolveFunction',
    'tree_leaves', 'tree_map', 'tree_flatten', 'tree_unflatten', 'Partial',
    'get_last_stats', 'JacobiPreconditioner', 'BlockJacobiPreconditioner', 'ChebyshevPreconditioner',
    'AggregationMultigridPreconditioner', 'pairwise_aggregates',
]

__version__ = '1.0.0'
