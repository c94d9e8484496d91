"""Preconditioners for the `M` argument of cg / bicgstab / gmres (TSL:1019-1021, 849).

The reference takes any callable `M`.  A `JacobiPreconditioner` IS such a callable (`M(v) = v / diag(A)`), so it
works on every path and with the reference's own solvers; on the HIP fast path `cg` recognises it and runs the
preconditioned iteration device-resident (`hipk_pcg_solve`: the scaling is fused into the update and direction
kernels, 16 n extra bytes per iteration instead of a separate pass) -- SURVEY 8f-3.  On a `RowBlockCSR` (one rank's rows of a
global system) `JacobiPreconditioner(A)` holds the rank's slice of the reciprocal diagonal, and the row-partitioned
cg / bicgstab / gmres run it in their C-driven loops (`hipk_dist_p*_solve`).  `ChebyshevPreconditioner.for_row_block(A_rb)` is the
Chebyshev polynomial of the global system on such an operand, for the row-partitioned cg (`hipk_dist_chebcg_solve`).
"""
import ctypes
import math

import torch

__all__ = ["JacobiPreconditioner", "BlockJacobiPreconditioner", "ChebyshevPreconditioner"]


def _diagonal(A: torch.Tensor) -> torch.Tensor:
    if A.layout == torch.strided:
        return torch.diagonal(A).clone()
    if A.layout == torch.sparse_csr:
        crow, col, val = A.crow_indices(), A.col_indices(), A.values()
        n = A.shape[0]
        rows = torch.repeat_interleave(torch.arange(n, device=val.device), crow[1:] - crow[:-1])
        on = col == rows
        d = torch.zeros(n, dtype=val.dtype, device=val.device)
        return d.index_add_(0, rows[on], val[on])          # duplicate diagonal entries add, as in A @ e_i
    if A.layout == torch.sparse_coo:
        Ac = A.coalesce()
        i, v = Ac.indices(), Ac.values()
        on = i[0] == i[1]
        d = torch.zeros(A.shape[0], dtype=v.dtype, device=v.device)
        return d.index_add_(0, i[0][on], v[on])
    return _diagonal(A.to_sparse_csr())


def _row_block_diagonal(A) -> torch.Tensor:
    """The diagonal of a RowBlockCSR's rows: the entries with global column row0 + i of local row i (duplicates add)."""
    crow, col, val = A.crow, A.col, A.val
    n, row0 = A.part.n_local, A.part.row0
    rows = torch.repeat_interleave(torch.arange(n, device=val.device), crow[1:] - crow[:-1])
    on = col == rows + row0
    d = torch.zeros(n, dtype=val.dtype, device=val.device)
    return d.index_add_(0, rows[on], val[on])


def _all_ranks_ok(A, ok: bool) -> bool:
    """MIN all-reduce of a flag over the RowBlockCSR's process group: a failing check on one rank fails on every rank, so no
    rank goes on into the solve's set-up collectives while another has raised."""
    import torch.distributed as dist
    if A.part.world == 1 or not dist.is_initialized():
        return ok
    dev = A.val.device if dist.get_backend(A.group) == "nccl" else torch.device("cpu")
    t = torch.tensor([1 if ok else 0], dtype=torch.int32, device=dev)
    dist.all_reduce(t, op=dist.ReduceOp.MIN, group=A.group)
    return bool(t.item())


class JacobiPreconditioner:
    """M(v) = v / diag(A).  `dinv` is the reciprocal diagonal, computed once (one rounding per entry).

    `A` may be a `RowBlockCSR`: every rank of its process group builds the preconditioner from its block (a collective: a zero
    on the diagonal of any rank's rows makes every rank raise).  `dinv` is then the rank's slice (rows `row_range`), `shape` the
    global one, and M applies to the rank's slices of vectors."""

    def __init__(self, A: torch.Tensor):
        if getattr(A, "_hipk_row_block", False) is True:
            d = _row_block_diagonal(A)
            if not _all_ranks_ok(A, not bool((d == 0).any())):
                raise ValueError("JacobiPreconditioner: zero on the diagonal (of some rank's rows of the RowBlockCSR)")
            self.dinv = torch.reciprocal(d)
            self.shape = tuple(A.shape)
            self.row_range = (A.part.row0, A.part.row1)
            return
        if not (isinstance(A, torch.Tensor) and A.ndim == 2 and A.shape[0] == A.shape[1]):
            raise ValueError("JacobiPreconditioner needs a square matrix tensor")
        d = _diagonal(A.detach())
        if bool((d == 0).any()):
            raise ValueError("JacobiPreconditioner: zero on the diagonal")
        self.dinv = torch.reciprocal(d)
        self.shape = tuple(A.shape)

    def __call__(self, v):
        return self.dinv.to(v.dtype) * v


def _diagonal_blocks(A: torch.Tensor, bs: int) -> torch.Tensor:
    """[ceil(n / bs), bs, bs]: the diagonal blocks of A; a ragged last block is completed with identity."""
    n = A.shape[0]
    nb = (n + bs - 1) // bs
    if A.layout == torch.strided:
        rows, cols = torch.nonzero(A, as_tuple=True)
        vals = A[rows, cols]
    else:
        coo = A.to_sparse_coo().coalesce() if A.layout != torch.sparse_coo else A.coalesce()
        rows, cols, vals = coo.indices()[0], coo.indices()[1], coo.values()
    on = torch.div(rows, bs, rounding_mode="floor") == torch.div(cols, bs, rounding_mode="floor")
    r, c, v = rows[on], cols[on], vals[on]
    blocks = torch.zeros(nb * bs * bs, dtype=vals.dtype, device=vals.device)
    blocks.index_add_(0, (torch.div(r, bs, rounding_mode="floor") * bs + r % bs) * bs + c % bs, v)
    blocks = blocks.view(nb, bs, bs)
    pad = nb * bs - n
    if pad:
        idx = torch.arange(bs - pad, bs, device=vals.device)
        blocks[nb - 1, idx, idx] = 1.0
    return blocks


class BlockJacobiPreconditioner:
    """M(v) = blockdiag(A)^-1 v with `block_size` x `block_size` diagonal blocks (1 <= block_size <= 32), inverted once.

    A callable for the reference's `M` hook (TSL:849, 908, 922, 351).  On device vectors the apply is a hand-written
    kernel (`hipk_block_jacobi_apply`) that cg / bicgstab / gmres run between their fused kernels on the solver's stream
    (no synchronisation); on CPU tensors it is a batched matmul.  For unknowns ordered with several degrees of freedom per
    node (systems of PDEs) or for strongly anisotropic stencils, where the point-Jacobi diagonal is a poor approximation."""

    def __init__(self, A: torch.Tensor, block_size: int = 4):
        if not (isinstance(A, torch.Tensor) and A.ndim == 2 and A.shape[0] == A.shape[1]):
            raise ValueError("BlockJacobiPreconditioner needs a square matrix tensor")
        if not 1 <= int(block_size) <= 32:
            raise ValueError("block_size must be in [1, 32]")
        self.block_size = int(block_size)
        self.shape = tuple(A.shape)
        blocks = _diagonal_blocks(A.detach(), self.block_size)
        try:
            self.binv = torch.linalg.inv(blocks).contiguous()
        except RuntimeError as e:
            raise ValueError(f"BlockJacobiPreconditioner: a diagonal block is singular ({e})") from None

    def __call__(self, v):
        n, bs = self.shape[0], self.block_size
        if v.shape != (n,):
            raise ValueError(f"BlockJacobiPreconditioner for {n} unknowns applied to a vector of shape {tuple(v.shape)}")
        binv = self.binv if self.binv.dtype == v.dtype else self.binv.to(v.dtype)
        if v.is_cuda and v.dtype in (torch.float64, torch.float32):
            from .. import _hipk
            if binv is not self.binv:
                self.binv = binv          # keep the converted copy: the solver calls with one dtype
            return _hipk.block_jacobi_apply(binv, bs, _hipk.aligned(v))
        nb = binv.shape[0]
        vp = torch.zeros(nb * bs, dtype=v.dtype, device=v.device)
        vp[:n] = v
        return torch.bmm(binv.to(v.device), vp.view(nb, bs, 1)).view(-1)[:n]


class _SpecSpmv:
    """y = A x on CPU tensors in the ONE summation order of the library's SpMV kernels (csrc/hipk_spmv.h), from element-wise torch
    ops only: a row of at most 32 entries is s = 0, s = s + a_ij x_j in CSR order; a longer row is 64 strided partial sums (entry
    j of the row to lane j % 64, each lane ascending) folded by v[l] += v[l + s], s = 32 .. 1.  Products and sums are separate
    roundings."""

    LONG_ROW = 32

    def __init__(self, crow: torch.Tensor, col: torch.Tensor, val: torch.Tensor):
        crow, col = crow.to(torch.int64), col.to(torch.int64)
        n = crow.numel() - 1
        lens = crow[1:] - crow[:-1]
        rows = torch.repeat_interleave(torch.arange(n), lens)
        pos = torch.arange(col.numel()) - crow[:-1][rows]            # position of an entry in its row
        self.n, self.dtype = n, val.dtype
        short = lens <= self.LONG_ROW
        self.K = int(lens[short].max()) if bool(short.any()) else 0
        e = short[rows]
        self.col_s = torch.zeros(n, max(self.K, 1), dtype=torch.int64)
        self.val_s = torch.zeros(n, max(self.K, 1), dtype=val.dtype)
        self.has_s = torch.zeros(n, max(self.K, 1), dtype=torch.bool)
        self.col_s[rows[e], pos[e]] = col[e]
        self.val_s[rows[e], pos[e]] = val[e]
        self.has_s[rows[e], pos[e]] = True
        self.long_rows = torch.nonzero(~short).view(-1)
        if self.long_rows.numel():
            slot = torch.full((n,), -1, dtype=torch.int64)
            slot[self.long_rows] = torch.arange(self.long_rows.numel())
            e = ~e
            steps = (int(lens.max()) + 63) // 64
            shape = (self.long_rows.numel(), steps, 64)
            self.col_l = torch.zeros(shape, dtype=torch.int64)
            self.val_l = torch.zeros(shape, dtype=val.dtype)
            self.has_l = torch.zeros(shape, dtype=torch.bool)
            idx = (slot[rows[e]], pos[e] // 64, pos[e] % 64)
            self.col_l[idx] = col[e]
            self.val_l[idx] = val[e]
            self.has_l[idx] = True

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        y = torch.zeros(self.n, dtype=self.dtype)
        for k in range(self.K):
            p = self.val_s[:, k] * x[self.col_s[:, k]]
            y = torch.where(self.has_s[:, k], y + p, y)
        if self.long_rows.numel():
            v = torch.zeros(self.long_rows.numel(), 64, dtype=self.dtype)
            for st in range(self.col_l.shape[1]):
                p = self.val_l[:, st] * x[self.col_l[:, st]]
                v = torch.where(self.has_l[:, st], v + p, v)
            s = 32
            while s >= 1:
                v = v[:, :s] + v[:, s:2 * s]
                s //= 2
            y[self.long_rows] = v[:, 0]
        return y


class ChebyshevPreconditioner:
    """M(r) = p_m(D^-1 A) D^-1 r, D = diag(A): the Chebyshev polynomial of degree m in the Jacobi-scaled matrix, m = `degree`
    SpMVs per apply (1 <= degree <= 32).  Only SpMVs and element-wise steps: no dot products, no triangular solves, so the
    apply is deterministic, independent of launch shapes, and bitwise equal to a CPU mirror of the steps below.

    For an SPD `A` it is a fixed SPD operator, so plain preconditioned CG stays valid (the supported case).  With `bicgstab` /
    `gmres` it is LEFT preconditioning by a polynomial designed for a real positive spectrum: nothing is promised for matrices
    whose D^-1 A has eigenvalues far from the positive real axis.

    `lmax` defaults to the Gershgorin bound of D^-1 A, max_i sum_j |a_ij| / a_ii (a safe upper bound), `lmin` to `lmax / ratio`;
    0 < lmin < lmax is required.  The residual polynomial is T_m((theta - lambda) / delta) / T_m(theta / delta), so p_m is
    POSITIVE on all of (0, lmax] even when `lmin` overestimates the smallest eigenvalue: a too large `lmin` costs iterations,
    never definiteness.

    Coefficients (host, double; attributes `c0`, `c1`, `c2` -- lists of length m for steps 1 .. m --, `dinv`, `scale`):
        theta = (lmax + lmin) / 2, delta = (lmax - lmin) / 2, sigma = theta / delta, rho_0 = 1 / sigma, c0 = 1 / theta,
        rho_k = 1 / (2 sigma - rho_{k-1}), c1[k] = rho_k rho_{k-1}, c2[k] = 2 rho_k / delta.
    The apply, every step a separate rounding (no fma):
        step 0:  d = c0 * (dinv * r), z = d
        step k:  res = dinv * (r - A z)   (row sums in the SpMV kernels' one summation order)
                 d = (c1[k] * d) + (c2[k] * res);  z = z + d;  the last step returns scale * (z + d) when scale != 1.

    `normalize`.  The reference decides `info` after the loop from ||M (b - A x)|| <= tol ||b|| (TSL:1007-1014).  A Chebyshev M
    approximates A^-1 and has norm above 1, so a solve whose TRUE residual is below tol ||b|| can still return info = -1.
    Scaling the OUTPUT of M by a constant changes neither the iterates nor the counts; `normalize=True` sets
    scale = 1 / (B max_i dinv_i) with B = max(p_m(0), (1 + 1 / T_m(sigma)) / lmin), a bound of p_m on (0, lmax]
    (p_m(0): what the recurrence gives for the scalar system a = 0, dinv = 1, r = 1; T_m(sigma) = cosh(m acosh sigma)), which
    bounds the norm of M by 1.  `normalize=False` sets scale = 1: the solve then behaves exactly as the reference does with
    such an M, its info = -1 included.

    CPU vectors run torch ops in exactly the order above; device fp64 / fp32 vectors run `hipk_cheb_apply` on the current
    stream without synchronisation: one launch per step where the matrix's SpMV kernel has the Chebyshev epilogue, else SpMV +
    a vector kernel (same bits).  The handle is `_hipk.handle_for(A)`, the one a solve of the same `A` holds; the apply takes no
    lock and uses none of the handle's reduction scratch.  `applies` / `spmvs` count calls and their SpMVs;
    `get_last_stats().matvecs` keeps the reference's meaning, the solver's own applications of A.

    On a `RowBlockCSR` the constructor raises; `ChebyshevPreconditioner.for_row_block(A_rb, ...)` builds the preconditioner of the
    global system there (every rank calls it), for `cg(A_rb, b_local, M=P)`."""

    def __init__(self, A: torch.Tensor, degree: int = 3, lmax=None, lmin=None, ratio: float = 30.0, normalize: bool = True):
        if getattr(A, "_hipk_row_block", False) is True:
            raise ValueError("ChebyshevPreconditioner is not available on a RowBlockCSR (the row-partitioned loops take a "
                             "JacobiPreconditioner only)")
        if not (isinstance(A, torch.Tensor) and A.ndim == 2 and A.shape[0] == A.shape[1]):
            raise ValueError("ChebyshevPreconditioner needs a square matrix tensor")
        if not 1 <= int(degree) <= 32:
            raise ValueError("degree must be in [1, 32]")
        self.degree = int(degree)
        self.shape = tuple(A.shape)
        self._A = A.detach()
        d = _diagonal(self._A)
        if bool((d <= 0).any()):
            raise ValueError("ChebyshevPreconditioner: zero or negative entry on the diagonal")
        self.dinv = torch.reciprocal(d)
        if lmax is None:
            lmax = float((self._abs_row_sums().to(torch.float64) / d.to(torch.float64)).max())
        self._set_coefficients(lmax, lmin, ratio, normalize, float(self.dinv.max()) if normalize else 0.0)
        self._cpu = None      # (spec SpMV, dinv) per dtype, built on the first CPU apply
        self._dev = None      # (handle, dinv) of the first device apply

    def _set_coefficients(self, lmax, lmin, ratio, normalize, dinv_max) -> None:
        """lmin, lmax, c0, c1, c2, scale and the counters, from the spectral bounds and max_i dinv_i (host doubles)."""
        m = self.degree
        lmax = float(lmax)
        lmin = lmax / float(ratio) if lmin is None else float(lmin)
        if not 0.0 < lmin < lmax:
            raise ValueError(f"ChebyshevPreconditioner needs 0 < lmin < lmax, got lmin = {lmin}, lmax = {lmax}")
        self.lmin, self.lmax = lmin, lmax
        theta, delta = (lmax + lmin) / 2, (lmax - lmin) / 2
        sigma = theta / delta
        rho = 1 / sigma
        self.c0, self.c1, self.c2 = 1 / theta, [], []
        for _ in range(m):
            rho_k = 1 / (2 * sigma - rho)
            self.c1.append(rho_k * rho)
            self.c2.append(2 * rho_k / delta)
            rho = rho_k
        self.scale = 1.0
        if normalize:
            dd = zz = self.c0                      # p_m(0): the recurrence on a = 0, dinv = 1, r = 1 (res = 1 in every step)
            for k in range(m):
                dd = self.c1[k] * dd + self.c2[k]
                zz = zz + dd
            bound = max(zz, (1 + 1 / math.cosh(m * math.acosh(sigma))) / lmin)
            self.scale = 1 / (bound * dinv_max)
        self._coef = (ctypes.c_double * (2 * m + 2))(self.c0, *self.c1, *self.c2, self.scale)
        self.applies = 0
        self.spmvs = 0

    @classmethod
    def for_row_block(cls, A, degree: int = 3, lmax=None, lmin=None, ratio: float = 30.0, normalize: bool = True):
        """The preconditioner of the GLOBAL system a `RowBlockCSR` is a row block of, for the row-partitioned `cg` -- see
        `RowBlockChebyshevPreconditioner`.  Every rank of the operand's process group calls it."""
        return RowBlockChebyshevPreconditioner(A, degree, lmax, lmin, ratio, normalize)

    def _abs_row_sums(self) -> torch.Tensor:
        A = self._A
        if A.layout == torch.strided:
            return A.abs().sum(dim=1)
        csr = A if A.layout == torch.sparse_csr else (A.coalesce() if A.layout == torch.sparse_coo else A).to_sparse_csr()
        crow, val = csr.crow_indices(), csr.values()
        rows = torch.repeat_interleave(torch.arange(A.shape[0], device=val.device), crow[1:] - crow[:-1])
        return torch.zeros(A.shape[0], dtype=val.dtype, device=val.device).index_add_(0, rows, val.abs())

    def _apply_torch(self, v: torch.Tensor) -> torch.Tensor:
        if self._cpu is None or self._cpu[1].dtype != v.dtype:
            A = self._A.cpu()
            csr = A if A.layout == torch.sparse_csr else (A.coalesce() if A.layout == torch.sparse_coo else A).to_sparse_csr()
            self._cpu = (_SpecSpmv(csr.crow_indices(), csr.col_indices(), csr.values().to(v.dtype)), self.dinv.cpu().to(v.dtype))
        spmv, dinv = self._cpu
        c = lambda x: torch.tensor(x, dtype=v.dtype)        # a coefficient, rounded to the working dtype once
        d = c(self.c0) * (dinv * v)
        z = d
        for k in range(self.degree):
            res = dinv * (v - spmv(z))
            d = (c(self.c1[k]) * d) + (c(self.c2[k]) * res)
            z = z + d
        if self.scale != 1.0:
            z = c(self.scale) * z
        return z

    def __call__(self, v):
        n = self.shape[0]
        if not isinstance(v, torch.Tensor) or v.shape != (n,):
            raise ValueError(f"ChebyshevPreconditioner for {n} unknowns applied to a vector of shape "
                             f"{tuple(getattr(v, 'shape', ()))}")
        if v.is_cuda:
            from .. import _hipk
            if self._dev is None:
                if not self._A.is_cuda:
                    raise ValueError("ChebyshevPreconditioner of a CPU matrix applied to a device vector")
                h = _hipk.handle_for(self._A)
                self._dev = (h, _hipk.aligned(self.dinv.to(device=h.device, dtype=h.dtype)))
            h, dinv = self._dev
            if v.dtype != h.dtype or v.device != h.device:
                raise ValueError(f"ChebyshevPreconditioner of a {h.dtype} matrix on {h.device} applied to a {v.dtype} vector on "
                                 f"{v.device}")
            z = _hipk.cheb_apply(h, self.degree, dinv, self._coef, v)
        else:
            if v.dtype not in (torch.float64, torch.float32):
                raise ValueError(f"ChebyshevPreconditioner applies to float64 / float32 vectors, not {v.dtype}")
            z = self._apply_torch(v)
        self.applies += 1
        self.spmvs += self.degree
        return z


def _row_block_abs_row_sums(A) -> torch.Tensor:
    """sum_j |a_ij| of a RowBlockCSR's rows, each row summed left to right in CSR order whatever the device: the bits
    `ChebyshevPreconditioner._abs_row_sums` gives for the same rows of the global matrix on CPU tensors."""
    crow, val = A.crow.to(torch.int64), A.val
    n = A.part.n_local
    s = torch.zeros(n, dtype=val.dtype, device=val.device)
    if n == 0 or val.numel() == 0:
        return s
    lens = crow[1:] - crow[:-1]
    K = int(lens.max())
    if K > 64:        # long rows: the sequential CPU sum
        rows = torch.repeat_interleave(torch.arange(n), lens.cpu())
        return torch.zeros(n, dtype=val.dtype).index_add_(0, rows, val.abs().cpu()).to(val.device)
    av = val.abs()
    for k in range(K):
        has = lens > k
        s = torch.where(has, s + av[torch.where(has, crow[:-1] + k, 0)], s)
    return s


class RowBlockChebyshevPreconditioner(ChebyshevPreconditioner):
    """`ChebyshevPreconditioner.for_row_block(A_rb, ...)`: the Chebyshev preconditioner of the GLOBAL system on a `RowBlockCSR`,
    for `cg(A_rb, b_local, M=P)` -- bit for bit `cg(A, b, M=ChebyshevPreconditioner(A, ...))` on one device, for any rank count.

    Every rank of the operand's process group constructs it (one MAX all-reduce: the Gershgorin `lmax` and max_i dinv_i are
    maxima over the ranks' rows, and a zero or negative diagonal entry on ANY rank raises on every rank); without a process group
    the world is 1 and nothing is exchanged.  `degree`, `lmin`, `lmax`, `c0`, `c1`, `c2`, `scale` are on every rank those of
    `ChebyshevPreconditioner(A_global, ...)` with the same arguments; `shape` is the global shape, `row_range` the rank's rows,
    `dinv` the reciprocal diagonal of those rows.

    `P(v_local)` is collective too: every rank passes its slice of a global vector and gets its slice of M v (m halo exchanges,
    no reduction).  Device vectors run `hipk_dist_cheb_apply`; CPU vectors (an operand built with an explicit `ops` backend) the
    torch steps of the class around the backend's SpMV."""

    def __init__(self, A, degree: int = 3, lmax=None, lmin=None, ratio: float = 30.0, normalize: bool = True):
        if getattr(A, "_hipk_row_block", False) is not True:
            raise ValueError("ChebyshevPreconditioner.for_row_block needs a RowBlockCSR")
        if not 1 <= int(degree) <= 32:
            raise ValueError("degree must be in [1, 32]")
        self.degree = int(degree)
        self.shape = tuple(A.shape)
        self.row_range = (A.part.row0, A.part.row1)
        self._A = A
        d = _row_block_diagonal(A)
        have = d.numel() > 0
        bad = bool((d <= 0).any())
        loc_lmax = loc_dinv = 0.0
        if not bad and have:
            if lmax is None:
                loc_lmax = float((_row_block_abs_row_sums(A).to(torch.float64) / d.to(torch.float64)).max())
            if normalize:
                loc_dinv = float(torch.reciprocal(d).max())
        bad, loc_lmax, loc_dinv = self._max_over_ranks(A, [1.0 if bad else 0.0, loc_lmax, loc_dinv])
        if bad:
            raise ValueError("ChebyshevPreconditioner: zero or negative entry on the diagonal (of some rank's rows of the "
                             "RowBlockCSR)")
        self.dinv = torch.reciprocal(d)
        self._set_coefficients(loc_lmax if lmax is None else lmax, lmin, ratio, normalize, loc_dinv)
        self._cpu = self._dev = None

    @staticmethod
    def _max_over_ranks(A, values):
        import torch.distributed as dist
        if A.part.world == 1 or not dist.is_initialized():
            return values
        dev = A.val.device if dist.get_backend(A.group) == "nccl" else torch.device("cpu")
        t = torch.tensor(values, dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX, group=A.group)
        return t.tolist()

    def __call__(self, v):
        A = self._A
        n = A.part.n_local
        if not isinstance(v, torch.Tensor) or v.shape != (n,):
            raise ValueError(f"ChebyshevPreconditioner of rows {self.row_range} applied to a vector of shape "
                             f"{tuple(getattr(v, 'shape', ()))} (this rank's slice has {n} entries)")
        if v.dtype != torch.float64 or v.device != A.val.device:
            raise ValueError(f"the row-partitioned ChebyshevPreconditioner applies to float64 vectors on {A.val.device}, not "
                             f"{v.dtype} on {v.device}")
        z = A.chebyshev_apply(self, v.detach())
        self.applies += 1
        self.spmvs += self.degree
        return z
