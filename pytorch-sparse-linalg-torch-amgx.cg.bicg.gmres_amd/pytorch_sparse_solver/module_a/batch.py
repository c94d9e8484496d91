"""cg_batch / bicgstab_batch / gmres_batch: S independent small systems that share ONE sparsity pattern.

`X[s]`, `info[s]` and the per-system statistics are what `cg(A_s, B[s], X0[s], ...)` (or `bicgstab`, `gmres`) returns for the CSR
tensor A_s of system s, bit for bit.  Two routes compute them:

  'kernel'  the batch kernels of libhipk.so (csrc/hipk_batch.hip, hipk_batch_gm.hip): one 256-thread workgroup owns one system for
            its whole solve, a launch covers all S systems.  Device operands, n <= 4096, at most 32 stored entries per row;
            gmres_batch: restart <= 31.
  'loop'    one public single solve per system: every input the single solvers accept, CPU tensors included.
  'auto'    the kernel for device operands inside its envelope when S >= BATCH_MIN_SYSTEMS (gmres_batch: GMRES_BATCH_MIN_SYSTEMS;
            with a BatchedBlockJacobiPreconditioner: BJ_BATCH_MIN_SYSTEMS), else the loop.

`M` is None, a `BatchedJacobiPreconditioner` or a `BatchedBlockJacobiPreconditioner` (csrc/hipk_batch_bj.hip; gmres_batch runs the
latter on the loop only).

The three solves refuse operands that require grad.  `cg_batch_differentiable` / `bicgstab_batch_differentiable` /
`gmres_batch_differentiable` (at the end of this file) return X only and differentiate it with respect to B and to per-system values on
A's pattern: the same batch solve of the transposed systems gives Lam = A^-T dL/dX, then grad_B = Lam and
grad_values[s, k] = -(Lam[s, row(k)] * X[s, col(k)]) (csrc/hipk_vgrad.hip).
"""
from __future__ import annotations

import time
from typing import Optional, Sequence, Tuple, Union

import torch

from .preconditioners import BlockJacobiPreconditioner, JacobiPreconditioner
from .torch_sparse_linalg import _set_stats, bicgstab, cg, get_last_stats, gmres

# The smallest S at which 'auto' takes the batch kernels: the measured crossover (tools/batch_probe.py, profiles/batch_probe.txt;
# DESIGN.md 7c).  One system alone is slower in the kernel than in the single solve's one-launch loop from n = 1024 on (0.26-0.8x:
# one workgroup against 8 to 32) and still at S = 4 for n = 4096 (0.50x); at S = 8 the kernel is level at worst (cg, n = 4096:
# 0.98x) and 2-8.4x ahead elsewhere, from S = 64 on 16-900x.
BATCH_MIN_SYSTEMS = 8


# The smallest S at which 'auto' takes hipk_cg_bjbatch_kernel / hipk_bi_bjbatch_kernel for a BatchedBlockJacobiPreconditioner: the
# measured crossover (tools/bj_batch_probe.py, profiles/bj_batch_probe.txt).  The loop here is the single solves'
# callback form (11-32 k system-iterations per second whatever n), far slower than the one-launch loops BATCH_MIN_SYSTEMS was set
# against.  At S = 2 the kernel is still behind for n = 4096 (bs = 32: cg 0.80x, bicgstab 0.61x); at S = 4 it is ahead in all twelve
# probed cases (1.18x at worst: bicgstab, n = 4096, bs = 32), at S = 8 2.3-56x.
BJ_BATCH_MIN_SYSTEMS = 4


def _aligned_rows(t: torch.Tensor) -> bool:
    """Rows of a 2-D tensor start 16-byte aligned and are contiguous inside."""
    es = t.element_size()
    return t.stride(1) == 1 and t.data_ptr() % 16 == 0 and (t.stride(0) * es) % 16 == 0 and t.stride(0) >= t.shape[1]


def _pad_rows(t: torch.Tensor) -> torch.Tensor:
    """`t` itself when its rows are aligned already, else a copy with the leading dimension rounded up to 16 bytes."""
    if _aligned_rows(t):
        return t
    per = 16 // t.element_size()
    ld = (t.shape[1] + per - 1) // per * per
    buf = torch.zeros((t.shape[0], ld), dtype=t.dtype, device=t.device)
    buf[:, :t.shape[1]] = t
    return buf[:, :t.shape[1]]


class BatchedCSR:
    """S square CSR matrices with one pattern: crow (n + 1,), col (nnz,) shared, values (S, nnz) (fp64 or fp32), on one device.
    Rows may be unsorted, hold a column twice or a stored zero, as everywhere in this library."""

    def __init__(self, crow: torch.Tensor, col: torch.Tensor, values: torch.Tensor):
        for name, t in (("crow", crow), ("col", col), ("values", values)):
            if not isinstance(t, torch.Tensor):
                raise ValueError(f"BatchedCSR: {name} must be a tensor")
        if crow.dim() != 1 or crow.numel() < 2 or col.dim() != 1 or values.dim() != 2:
            raise ValueError("BatchedCSR: crow must have shape (n + 1,), col (nnz,) and values (S, nnz)")
        if crow.dtype.is_floating_point or col.dtype.is_floating_point:
            raise ValueError("BatchedCSR: crow and col must be integer tensors")
        if values.dtype not in (torch.float64, torch.float32):
            raise ValueError(f"BatchedCSR: values must be float64 or float32, got {values.dtype}")
        if values.shape[0] < 1 or values.shape[1] != col.numel():
            raise ValueError(f"BatchedCSR: values must have shape (S, nnz) with S >= 1 and nnz = {col.numel()}, got {tuple(values.shape)}")
        if not (crow.device == col.device == values.device):
            raise ValueError("BatchedCSR: crow, col and values must be on one device")
        if values.requires_grad:
            raise ValueError("BatchedCSR: the batch solves are not differentiable")
        if int(crow[0]) != 0 or int(crow[-1]) != col.numel() or bool((crow[1:] < crow[:-1]).any()):
            raise ValueError("BatchedCSR: crow is not a row pointer array of nnz entries")
        n = crow.numel() - 1
        if col.numel() and (int(col.min()) < 0 or int(col.max()) >= n):
            raise ValueError("BatchedCSR: a column index is outside [0, n)")
        self.crow, self.col, self.values = crow, col, values
        self.n, self.nnz, self.batch = n, int(col.numel()), int(values.shape[0])
        self.shape = (self.batch, n, n)
        self.max_row_len = int((crow[1:] - crow[:-1]).max()) if n else 0
        # indices narrowed once (the kernels and the Jacobi diagonal read these)
        from .. import _hipk
        self.crow32 = _hipk.aligned(crow.to(torch.int32))
        self.col32 = _hipk.aligned(col.to(torch.int32))
        self._kernel_values = None
        self._pattern_cache = {}      # what depends on crow / col alone (the transposed pattern); shared by `with_values` objects

    @classmethod
    def _on_pattern(cls, src: "BatchedCSR", values: torch.Tensor) -> "BatchedCSR":
        new = cls.__new__(cls)
        new.crow, new.col, new.values = src.crow, src.col, values
        new.n, new.nnz, new.batch = src.n, src.nnz, int(values.shape[0])
        new.shape = (new.batch, src.n, src.n)
        new.max_row_len = src.max_row_len
        new.crow32, new.col32 = src.crow32, src.col32
        new._kernel_values = None
        new._pattern_cache = src._pattern_cache
        return new

    def with_values(self, values: torch.Tensor) -> "BatchedCSR":
        """A BatchedCSR of `values` (S', nnz) on THIS object's pattern: the pattern is not validated again and nothing is read back
        from the device; crow / col, their int32 copies and the cached transposed pattern are shared, not copied."""
        if not isinstance(values, torch.Tensor) or values.dim() != 2 or values.shape[0] < 1 or values.shape[1] != self.nnz:
            raise ValueError(f"BatchedCSR.with_values: values must have shape (S, nnz) with S >= 1 and nnz = {self.nnz}, got "
                             f"{tuple(getattr(values, 'shape', ()))}")
        if values.dtype not in (torch.float64, torch.float32):
            raise ValueError(f"BatchedCSR.with_values: values must be float64 or float32, got {values.dtype}")
        if values.device != self.crow.device:
            raise ValueError(f"BatchedCSR.with_values: values are on {values.device}, the pattern on {self.crow.device}")
        if values.requires_grad:
            raise ValueError("BatchedCSR: the batch solves are not differentiable (see cg_batch_differentiable(..., values=...))")
        return BatchedCSR._on_pattern(self, values)

    def transpose_pattern(self) -> Tuple["BatchedCSR", torch.Tensor]:
        """(P, perm): the pattern of A_s^T as a value-less BatchedCSR and the entry permutation with values(A_s^T) = values[s, perm].
        A stable sort of the entries by column, so every row of A^T lists its entries by source row, in stored order for a column
        stored twice; computed once per pattern and cached."""
        hit = self._pattern_cache.get("transpose")
        if hit is None:
            from .. import _hipk
            n = self.n
            rows = torch.repeat_interleave(torch.arange(n, device=self.crow.device), (self.crow[1:] - self.crow[:-1]).to(torch.int64))
            col = self.col.to(torch.int64)
            perm = torch.argsort(col, stable=True)
            crow_t = torch.zeros(n + 1, dtype=self.crow.dtype, device=self.crow.device)
            crow_t[1:] = torch.cumsum(torch.bincount(col, minlength=n), 0)
            P = BatchedCSR.__new__(BatchedCSR)
            P.crow, P.col, P.values = crow_t, rows[perm].to(self.col.dtype), None
            P.n, P.nnz, P.batch = n, self.nnz, 0
            P.shape = (0, n, n)
            P.max_row_len = int((crow_t[1:] - crow_t[:-1]).max()) if n else 0
            P.crow32 = _hipk.aligned(P.crow.to(torch.int32))
            P.col32 = _hipk.aligned(P.col.to(torch.int32))
            P._kernel_values = None
            P._pattern_cache = {}
            hit = self._pattern_cache["transpose"] = (P, perm)
        return hit

    def transposed(self) -> "BatchedCSR":
        """The BatchedCSR of the S matrices A_s^T: the cached transposed pattern with the values gathered as `values[:, perm]`."""
        P, perm = self.transpose_pattern()
        return BatchedCSR._on_pattern(P, self.values[:, perm])

    @property
    def device(self):
        return self.values.device

    @property
    def dtype(self):
        return self.values.dtype

    @classmethod
    def from_csr_list(cls, mats: Sequence[torch.Tensor]) -> "BatchedCSR":
        mats = list(mats)
        if not mats:
            raise ValueError("BatchedCSR.from_csr_list: empty list")
        for A in mats:
            if not (isinstance(A, torch.Tensor) and A.layout == torch.sparse_csr and A.dim() == 2 and A.shape[0] == A.shape[1]):
                raise ValueError("BatchedCSR.from_csr_list: every matrix must be a square torch CSR tensor")
        crow, col = mats[0].crow_indices(), mats[0].col_indices()
        for s, A in enumerate(mats[1:], 1):
            if A.shape != mats[0].shape or A.dtype != mats[0].dtype or A.device != mats[0].device:
                raise ValueError(f"BatchedCSR.from_csr_list: matrix {s} differs from matrix 0 in shape, dtype or device")
            if not (torch.equal(A.crow_indices(), crow) and torch.equal(A.col_indices(), col)):
                raise ValueError(f"BatchedCSR.from_csr_list: matrix {s} does not share the sparsity pattern (crow / col) of matrix 0")
        return cls(crow, col, torch.stack([A.values() for A in mats]))

    def system(self, s: int) -> torch.Tensor:
        """The CSR tensor A_s (its values a copy when row s of `values` does not start 16-byte aligned, as the single solves need)."""
        from .. import _hipk
        return torch.sparse_csr_tensor(self.crow, self.col, _hipk.aligned(self.values[s]), size=(self.n, self.n))

    def kernel_values(self) -> torch.Tensor:
        """`values` with 16-byte aligned rows: `values` itself, or a padded copy that is made again whenever `values` was written to
        (keyed on its address and version counter, as the handle cache of the single solves is)."""
        key = (self.values.data_ptr(), self.values._version)
        if self._kernel_values is None or self._kernel_values[0] != key:
            self._kernel_values = (key, _pad_rows(self.values))
        return self._kernel_values[1]

    def in_envelope(self) -> bool:
        from .. import _hipk
        return 1 <= self.n <= _hipk.BATCH_MAX_N and self.max_row_len <= _hipk.BATCH_MAX_ROW


class BatchedJacobiPreconditioner:
    """M_s(v) = v / diag(A_s) for every system of a BatchedCSR: `dinv` (S, n), row s bitwise `JacobiPreconditioner(A_s).dinv`."""

    def __init__(self, A: BatchedCSR):
        if not isinstance(A, BatchedCSR):
            raise ValueError("BatchedJacobiPreconditioner needs a BatchedCSR")
        n = A.n
        rows = torch.repeat_interleave(torch.arange(n, device=A.device), A.crow[1:] - A.crow[:-1])
        on = A.col == rows
        d = torch.zeros((A.batch, n), dtype=A.dtype, device=A.device)
        d.index_add_(1, rows[on], A.values[:, on])          # duplicate diagonal entries add, as in A @ e_i
        if bool((d == 0).any()):
            raise ValueError("BatchedJacobiPreconditioner: zero on the diagonal")
        self.dinv = torch.reciprocal(d)
        self.shape = A.shape

    def system(self, s: int) -> JacobiPreconditioner:
        J = JacobiPreconditioner.__new__(JacobiPreconditioner)
        from .. import _hipk
        J.dinv = _hipk.aligned(self.dinv[s])
        J.shape = (self.shape[1], self.shape[2])
        return J


class BatchedBlockJacobiPreconditioner:
    """M_s(v) = blockdiag(A_s)^-1 v for every system of a BatchedCSR, with `block_size` x `block_size` diagonal blocks
    (1 <= block_size <= 32): `binv` (S, ceil(n / block_size), block_size, block_size), contiguous, in the dtype and on the device of
    `A.values`.  The blocks of all systems are taken in one pass over the shared pattern (entries stored twice add, a ragged last
    block is completed with identity) and inverted by one `torch.linalg.inv`.  `binv=` given: those blocks are M as they are (an
    approximate inverse; identity blocks make M the identity)."""

    def __init__(self, A: BatchedCSR, block_size: int = 4, binv: Optional[torch.Tensor] = None):
        if not isinstance(A, BatchedCSR):
            raise ValueError("BatchedBlockJacobiPreconditioner needs a BatchedCSR")
        if not 1 <= int(block_size) <= 32:
            raise ValueError("block_size must be in [1, 32]")
        bs = self.block_size = int(block_size)
        n = A.n
        nb = (n + bs - 1) // bs
        self.shape = A.shape
        if binv is not None:
            want = (A.batch, nb, bs, bs)
            if not isinstance(binv, torch.Tensor) or tuple(binv.shape) != want:
                raise ValueError(f"BatchedBlockJacobiPreconditioner: binv must have shape (S, ceil(n / bs), bs, bs) = {want}, got "
                                 f"{tuple(getattr(binv, 'shape', ()))}")
            if binv.dtype != A.dtype or binv.device != A.device:
                raise ValueError(f"BatchedBlockJacobiPreconditioner: binv is {binv.dtype} on {binv.device}, the matrices are "
                                 f"{A.dtype} on {A.device}")
            if not binv.is_contiguous():
                raise ValueError("BatchedBlockJacobiPreconditioner: binv must be contiguous")
            self.binv = binv.detach()
            return
        rows = torch.repeat_interleave(torch.arange(n, device=A.device), A.crow[1:] - A.crow[:-1])
        cols = A.col.to(torch.int64)
        on = torch.div(rows, bs, rounding_mode="floor") == torch.div(cols, bs, rounding_mode="floor")
        blocks = torch.zeros((A.batch, nb * bs * bs), dtype=A.dtype, device=A.device)
        blocks.index_add_(1, rows[on] * bs + cols[on] % bs, A.values[:, on])   # block b, local row i: (b bs + i) bs = row bs
        blocks = blocks.view(A.batch, nb, bs, bs)
        pad = nb * bs - n
        if pad:
            idx = torch.arange(bs - pad, bs, device=A.device)
            blocks[:, nb - 1, idx, idx] = 1.0
        try:
            self.binv = torch.linalg.inv(blocks.view(A.batch * nb, bs, bs)).view(A.batch, nb, bs, bs).contiguous()
        except RuntimeError as e:
            raise ValueError(f"BatchedBlockJacobiPreconditioner: a diagonal block is singular ({e})") from None

    def system(self, s: int) -> BlockJacobiPreconditioner:
        """The single solves' preconditioner of system s; its `binv` IS `self.binv[s]` (not inverted again: a batched inverse need
        not give the same bits for another batch size)."""
        P = BlockJacobiPreconditioner.__new__(BlockJacobiPreconditioner)
        P.block_size = self.block_size
        P.shape = (self.shape[1], self.shape[2])
        P.binv = self.binv[s]
        return P

    def transposed(self) -> "BatchedBlockJacobiPreconditioner":
        """The preconditioner of the transposed systems: blockdiag(A_s^T)^-1 = (blockdiag(A_s)^-1)^T, the blocks transposed."""
        T = BatchedBlockJacobiPreconditioner.__new__(BatchedBlockJacobiPreconditioner)
        T.block_size, T.shape = self.block_size, self.shape
        T.binv = self.binv.transpose(-1, -2).contiguous()
        return T


BatchedPreconditioner = Union[BatchedJacobiPreconditioner, BatchedBlockJacobiPreconditioner]


def _check(name, A, B, X0, M, route):
    if not isinstance(A, BatchedCSR):
        raise ValueError(f"{name}: A must be a BatchedCSR")
    if route not in ("auto", "kernel", "loop"):
        raise ValueError(f"{name}: route must be 'auto', 'kernel' or 'loop', got {route!r}")
    for what, t in (("B", B), ("X0", X0)):
        if t is None and what == "X0":
            continue
        if not isinstance(t, torch.Tensor) or t.dim() != 2 or tuple(t.shape) != (A.batch, A.n):
            raise ValueError(f"{name}: {what} must have shape (S, n) = ({A.batch}, {A.n}), got {tuple(getattr(t, 'shape', ()))}")
        if torch.is_complex(t) or not t.dtype.is_floating_point:
            raise ValueError(f"{name}: {what} must be a real floating-point tensor, got {t.dtype}")
        if t.device != A.device:
            raise ValueError(f"{name}: {what} is on {t.device}, the matrices on {A.device}")
        if t.dtype != A.dtype:
            raise ValueError(f"{name}: {what} is {t.dtype}, the matrices are {A.dtype}")
        if t.requires_grad:
            raise ValueError(f"{name} is not differentiable: call {name.split('_')[0]}_differentiable on each system instead")
    if M is not None:
        if not isinstance(M, (BatchedJacobiPreconditioner, BatchedBlockJacobiPreconditioner)):
            raise ValueError(f"{name}: M must be None or a BatchedJacobiPreconditioner or a BatchedBlockJacobiPreconditioner, "
                             f"got {type(M).__name__}")
        where = (M.binv if isinstance(M, BatchedBlockJacobiPreconditioner) else M.dinv).device
        if tuple(M.shape) != tuple(A.shape) or where != A.device:
            raise ValueError(f"{name}: the preconditioner (shape {tuple(M.shape)}, {where}) does not match A "
                             f"(shape {tuple(A.shape)}, {A.device})")


def _kernel_solve(kind, A: BatchedCSR, B, X0, tol, atol, maxiter, M, **gm):
    from .. import _hipk
    dt = A.dtype                                  # fp64, or fp32 storage when the matrices are fp32 (as the single solves)
    BB = _pad_rows(B.detach().to(dt))
    if X0 is None:
        X = _pad_rows(torch.zeros((A.batch, A.n), dtype=dt, device=A.device))
    else:
        X = X0.detach().to(dt).clone()
        if not _aligned_rows(X):
            X = _pad_rows(X)
    if isinstance(M, BatchedBlockJacobiPreconditioner):
        st = _hipk.solve_batch_bj(kind, A.n, A.nnz, A.crow32, A.col32, A.kernel_values(), _hipk.aligned(M.binv.to(dt)), M.block_size, BB, X,
                                  tol=tol, atol=atol, maxiter=maxiter)
        return X.contiguous(), st
    dinv = None if M is None else _pad_rows(M.dinv.detach().to(dt))
    st = _hipk.solve_batch(kind, A.n, A.nnz, A.crow32, A.col32, A.kernel_values(), dinv, BB, X, tol=tol, atol=atol, maxiter=maxiter,
                            **gm)
    return X.contiguous(), st


def _loop_solve(kind, A: BatchedCSR, B, X0, tol, atol, maxiter, M, **gm):
    from .. import _hipk
    solver = {"cg": cg, "bicgstab": bicgstab, "gmres": gmres}[kind]
    xs, infos, stats = [], [], []
    t0 = time.perf_counter()
    for s in range(A.batch):
        x, info = solver(A.system(s), B[s].clone(), None if X0 is None else X0[s].clone(), tol=tol, atol=atol, maxiter=maxiter,
                          M=None if M is None else M.system(s), **gm)
        xs.append(x)
        infos.append(int(info))
        stats.append(get_last_stats())
    ms = (time.perf_counter() - t0) * 1e3
    f = lambda name, default: [getattr(c, name, default) if c is not None else default for c in stats]
    tag = "blockjacobi" if isinstance(M, BatchedBlockJacobiPreconditioner) else "jacobi"
    name = kind if M is None else {"cg": f"pcg_{tag}", "bicgstab": f"pbicgstab_{tag}", "gmres": f"pgmres_{tag}"}[kind]
    st = _hipk.BatchSolveStats(method=f"{name}_batch", iterations=f("iterations", 0), matvecs=f("matvecs", 0), info=infos,
                               breakdown=f("breakdown", 0), b_norm=f("b_norm", 0.0), residual_norm=f("residual_norm", 0.0),
                               x_norm=f("x_norm", 0.0), threshold=f("threshold", 0.0), recurrence_rs=f("recurrence_rs", 0.0),
                               path="loop", launches=0, solve_ms=ms)
    return torch.stack(xs), st


def _batch(kind: str, A, B, X0, tol, atol, maxiter, M, route):
    name = f"{kind}_batch"
    _check(name, A, B, X0, M, route)
    on_device = A.values.is_cuda
    if route == "kernel":
        if not on_device:
            raise ValueError(f"{name}: route='kernel' needs device tensors (A is on {A.device}); use route='loop'")
        if not A.in_envelope():
            raise ValueError(f"{name}: route='kernel' takes systems of at most 4096 rows with at most 32 stored entries per row "
                             f"(n = {A.n}, longest row {A.max_row_len}); use route='loop'")
    least = BJ_BATCH_MIN_SYSTEMS if isinstance(M, BatchedBlockJacobiPreconditioner) else BATCH_MIN_SYSTEMS
    use_kernel = route == "kernel" or (route == "auto" and on_device and A.in_envelope() and A.batch >= least)
    X, st = (_kernel_solve if use_kernel else _loop_solve)(kind, A, B, X0, tol, atol, maxiter, M)
    _set_stats(st)
    return X, torch.tensor([int(i) for i in st.info], dtype=torch.int64)


def cg_batch(A: BatchedCSR, B: torch.Tensor, X0: Optional[torch.Tensor] = None, *, tol: float = 1e-5, atol: float = 0.0,
             maxiter: Optional[int] = None, M: Optional[BatchedPreconditioner] = None,
             route: str = "auto") -> Tuple[torch.Tensor, torch.Tensor]:
    """Conjugate gradients for the S systems A_s X[s] = B[s], B of shape (S, n).

    Returns `(X, info)`: X of shape (S, n), info a 1-D int64 CPU tensor of length S with `info[s]` = the info of
    `cg(A_s, B[s], X0[s], ...)`.  `get_last_stats()` is then a `BatchSolveStats`.  Not differentiable."""
    return _batch("cg", A, B, X0, tol, atol, maxiter, M, route)


def bicgstab_batch(A: BatchedCSR, B: torch.Tensor, X0: Optional[torch.Tensor] = None, *, tol: float = 1e-5, atol: float = 0.0,
                   maxiter: Optional[int] = None, M: Optional[BatchedPreconditioner] = None,
                   route: str = "auto") -> Tuple[torch.Tensor, torch.Tensor]:
    """BiCGStab for the S systems A_s X[s] = B[s] (see `cg_batch`); breakdowns (-10, -11) are decided per system."""
    return _batch("bicgstab", A, B, X0, tol, atol, maxiter, M, route)


# The smallest S at which 'auto' takes hipk_gm_batch_kernel.  PROVISIONAL: the crossover measured for cg_batch / bicgstab_batch
# (BATCH_MIN_SYSTEMS); no run of tools/gmres_batch_probe.py is recorded yet, the value is to be set from its first one.
GMRES_BATCH_MIN_SYSTEMS = 8


def gmres_batch(A: BatchedCSR, B: torch.Tensor, X0: Optional[torch.Tensor] = None, *, tol: float = 1e-5, atol: float = 0.0,
                restart: int = 20, maxiter: Optional[int] = None, M: Optional[BatchedPreconditioner] = None,
                solve_method: str = "batched", route: str = "auto") -> Tuple[torch.Tensor, torch.Tensor]:
    """Restarted GMRES for the S systems A_s X[s] = B[s] (see `cg_batch`): `maxiter` counts restart cycles, every system stops at its
    own cycle and, with solve_method='incremental', at its own Arnoldi step inside a cycle; happy breakdown is decided per system.
    The kernel route takes restart <= 31."""
    from .. import _hipk
    name = "gmres_batch"
    _check(name, A, B, X0, M, route)
    if int(restart) < 1:
        raise ValueError(f"{name}: restart must be at least 1, got {restart}")
    if solve_method not in ("batched", "incremental"):
        raise ValueError(f"Unsupported solve_method: {solve_method}")
    on_device = A.values.is_cuda
    block = isinstance(M, BatchedBlockJacobiPreconditioner)
    inside = A.in_envelope() and int(restart) <= _hipk.GMRES_BATCH_MAX_RESTART and not block
    if route == "kernel":
        if block:
            raise ValueError(f"{name}: the GMRES batch kernel has no block-Jacobi form (M is a BatchedBlockJacobiPreconditioner); "
                             f"use route='loop' or route='auto', which run one gmres per system")
        if not on_device:
            raise ValueError(f"{name}: route='kernel' needs device tensors (A is on {A.device}); use route='loop'")
        if not A.in_envelope():
            raise ValueError(f"{name}: route='kernel' takes systems of at most 4096 rows with at most 32 stored entries per row "
                             f"(n = {A.n}, longest row {A.max_row_len}); use route='loop'")
        if not inside:
            raise ValueError(f"{name}: route='kernel' takes a restart of at most {_hipk.GMRES_BATCH_MAX_RESTART} (restart = {restart}); "
                             f"use route='loop'")
    use_kernel = route == "kernel" or (route == "auto" and on_device and inside and A.batch >= GMRES_BATCH_MIN_SYSTEMS)
    X, st = (_kernel_solve if use_kernel else _loop_solve)("gmres", A, B, X0, tol, atol, maxiter, M, restart=int(restart),
                                                           solve_method=solve_method)
    _set_stats(st)
    return X, torch.tensor([int(i) for i in st.info], dtype=torch.int64)


# ------------------------------------------------------------------------- differentiable batch solves
def _batch_grad_values(A: BatchedCSR, Lam: torch.Tensor, X: torch.Tensor) -> torch.Tensor:
    """(S, nnz): G[s, k] = -(Lam[s, row(k)] * X[s, col(k)]) in the dtype of the matrices (module_a/matrix_grad.py): hipk_batch_grad_values
    on the device, for any n and row length, the torch expression of the same formula on CPU."""
    from .. import _hipk
    from . import matrix_grad
    Lam, X = Lam.to(A.dtype), X.to(A.dtype)
    if A.values.is_cuda:
        return _hipk.batch_grad_values(A.n, A.nnz, A.crow32, A.col32, Lam, X)   # (S, nnz), rows 16-byte aligned: a view when padded
    G = matrix_grad.grad_values_torch(matrix_grad.csr_rows(A.crow), A.col, Lam, X, A.dtype)
    _hipk.set_grad_stats("torch", 0, A.nnz, A.batch)
    return G


class BatchSolveFunction(torch.autograd.Function):
    """X = solve(A(values), B) for the S systems of a BatchedCSR pattern, with the implicit-function backward: ONE batch solve of the
    transposed systems, Lam = A^-T dL/dX, gives grad_B = Lam and grad_values[s, k] = -(Lam[s, row(k)] * X[s, col(k)])."""

    @staticmethod
    def forward(ctx, values, B, A, X0, M, solve, opts):
        X, _ = solve(A.with_values(values.detach()), B.detach(), None if X0 is None else X0.detach(), M=M, **opts)
        # the values go through save_for_backward: an in-place update between forward and backward (an optimiser step) is then an
        # error, not an adjoint solve on the new coefficients
        ctx.save_for_backward(values, X)
        ctx.A, ctx.M, ctx.solve, ctx.opts = A, M, solve, opts
        return X

    @staticmethod
    def backward(ctx, grad_output):
        if not (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
            return (None,) * 7
        values, X = ctx.saved_tensors
        M = ctx.M
        Aw = ctx.A.with_values(values.detach())          # on the cached pattern: no validation, no host sync
        At = Aw.transposed()
        opts = ctx.opts
        if opts["route"] == "kernel" and not At.in_envelope():
            # A's longest COLUMN is the transposed pattern's longest row: it may exceed the batch kernels' 32 entries although no
            # row of A does.  The forward ran, so backward must: the adjoint solve then picks its route itself
            opts = dict(opts, route="auto")
        Mt = M.transposed() if isinstance(M, BatchedBlockJacobiPreconditioner) else M     # the point Jacobi M serves A^T unchanged
        Lam, _ = ctx.solve(At, grad_output.detach().to(Aw.dtype).contiguous(), None, M=Mt, **opts)
        grad_values = _batch_grad_values(Aw, Lam, X) if ctx.needs_input_grad[0] else None
        return (grad_values, Lam if ctx.needs_input_grad[1] else None) + (None,) * 5


def _batch_differentiable(name, solve, A, B, X0, values, M, opts):
    if not isinstance(A, BatchedCSR):
        raise ValueError(f"{name}: A must be a BatchedCSR")
    if values is None:
        values = A.values
    elif (not isinstance(values, torch.Tensor) or tuple(values.shape) != (A.batch, A.nnz) or values.dtype != A.dtype
          or values.device != A.device):
        raise ValueError(f"{name}: values must be a {A.dtype} tensor of shape (S, nnz) = ({A.batch}, {A.nnz}) on {A.device}, got "
                         f"{getattr(values, 'dtype', None)} {tuple(getattr(values, 'shape', ()))}")
    if not isinstance(B, torch.Tensor):
        raise ValueError(f"{name}: B must be a tensor")
    if X0 is not None and isinstance(X0, torch.Tensor) and X0.requires_grad:
        raise ValueError(f"{name}: X0 is not differentiated; pass X0.detach()")
    return BatchSolveFunction.apply(values, B, A, X0, M, solve, opts)


def cg_batch_differentiable(A: BatchedCSR, B: torch.Tensor, X0: Optional[torch.Tensor] = None, *, values: Optional[torch.Tensor] = None,
                            tol: float = 1e-5, atol: float = 0.0, maxiter: Optional[int] = None,
                            M: Optional[BatchedPreconditioner] = None, route: str = "auto") -> torch.Tensor:
    """`cg_batch` returning only X, differentiable with respect to `B` and to `values`, an (S, nnz) tensor that stands in for
    `A.values` on A's validated pattern (None: A.values, which carries no gradient).  The forward is `cg_batch` on the detached
    operands: the same routes and bits, `get_last_stats()` as there.  Backward: one `cg_batch` of the transposed systems (same tol,
    atol, maxiter, M and route; its start vector is X0 = None, whatever the forward's X0 was) gives Lam = A^-T dL/dX; grad_B = Lam
    and grad_values[s, k] = -(Lam[s, row(k)] * X[s, col(k)]) (hipk_batch_grad_values on the device, for any n; `get_last_grad_stats()`).
    With route='kernel' the adjoint solve takes the kernel too, unless a COLUMN of the pattern holds more than 32 entries (a row of
    the transposed pattern outside the kernels' envelope): it then runs with route='auto' instead of failing in backward.  `values`
    must not be modified in place between forward and backward (autograd raises if it was)."""
    return _batch_differentiable("cg_batch_differentiable", cg_batch, A, B, X0, values, M,
                                 dict(tol=tol, atol=atol, maxiter=maxiter, route=route))


def bicgstab_batch_differentiable(A: BatchedCSR, B: torch.Tensor, X0: Optional[torch.Tensor] = None, *,
                                  values: Optional[torch.Tensor] = None, tol: float = 1e-5, atol: float = 0.0,
                                  maxiter: Optional[int] = None, M: Optional[BatchedPreconditioner] = None,
                                  route: str = "auto") -> torch.Tensor:
    """`bicgstab_batch` returning only X, differentiable with respect to `B` and `values` (see `cg_batch_differentiable`; the adjoint
    solve starts from X0 = None)."""
    return _batch_differentiable("bicgstab_batch_differentiable", bicgstab_batch, A, B, X0, values, M,
                                 dict(tol=tol, atol=atol, maxiter=maxiter, route=route))


def gmres_batch_differentiable(A: BatchedCSR, B: torch.Tensor, X0: Optional[torch.Tensor] = None, *, values: Optional[torch.Tensor] = None,
                               tol: float = 1e-5, atol: float = 0.0, restart: int = 20, maxiter: Optional[int] = None,
                               M: Optional[BatchedPreconditioner] = None, solve_method: str = "batched",
                               route: str = "auto") -> torch.Tensor:
    """`gmres_batch` returning only X, differentiable with respect to `B` and `values` (see `cg_batch_differentiable`; the adjoint
    solve uses the same restart and solve_method and starts from X0 = None)."""
    return _batch_differentiable("gmres_batch_differentiable", gmres_batch, A, B, X0, values, M,
                                 dict(tol=tol, atol=atol, restart=restart, maxiter=maxiter, solve_method=solve_method, route=route))
