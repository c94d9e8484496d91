"""ctypes binding of libhipk.so (include/hipk.h) -- the MI355X kernels behind Module A.

There is NO CPU fallback in here: every function raises if the HIP library is missing
or no gfx950 device is visible.  `import torch` must come before the library is loaded
(torch's bundled libamdhip64.so.7 is then the HIP runtime the library binds to).
"""
from __future__ import annotations

import collections
import ctypes
import math
import os
import threading
from dataclasses import dataclass
from typing import Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# HIPK_LIB_PATH: load another build of the library (diagnostic builds, e.g. `make STAMPS=1`); the default is the in-tree one
LIB_PATH = os.environ.get("HIPK_LIB_PATH") or os.path.join(_HERE, "_lib", "libhipk.so")
CSRC_DIR = os.path.normpath(os.path.join(_HERE, "..", "csrc"))

HIPK_F32, HIPK_F64 = 0, 1
GMRES_BATCHED, GMRES_INCREMENTAL = 0, 1

# every symbol include/hipk.h declares (tests/test_abi.py checks the export list)
SYMBOLS = [
    "hipk_version", "hipk_build_id", "hipk_op_create", "hipk_placement_probe", "hipk_last_error", "hipk_device_count",
    "hipk_csr_create", "hipk_csr_destroy", "hipk_csr_rows", "hipk_csr_nnz", "hipk_csr_spmv_bytes",
    "hipk_csr_spmv_path", "hipk_last_spmv_kernel", "hipk_last_solve_path", "hipk_last_solve_form", "hipk_last_cg_fused_directions", "hipk_last_cg_fused_kept_p", "hipk_solve_form_count", "hipk_solve_form_name", "hipk_csr_set_path", "hipk_csr_format_bytes",
    # new values on the pattern of an existing handle
    "hipk_csr_update_values", "hipk_last_csr_update_kind", "hipk_last_csr_update_syncs", "hipk_csr_revalue_probe",
    "hipk_csr_transpose_work_bytes", "hipk_csr_transpose",
    # the matrix gradient of a solve: G[k] = -(lam[row(k)] * x[col(k)]) for one matrix and for a batch on one pattern
    "hipk_batch_grad_values", "hipk_csr_grad_values", "hipk_last_grad_values_launches",
    "hipk_chunk_size", "hipk_chunk_count", "hipk_scratch_bytes",
    "hipk_spmv", "hipk_spmv_dot", "hipk_dot", "hipk_axpy", "hipk_xpby", "hipk_block_jacobi_apply",
    "hipk_cheb_apply",
    "hipk_cg_work_bytes", "hipk_cg_solve", "hipk_pcg_work_bytes", "hipk_pcg_solve", "hipk_pgmres_solve", "hipk_pbicgstab_work_bytes", "hipk_pbicgstab_solve", "hipk_pbicgstab_solve_cb", "hipk_pgmres_solve_cb",
    "hipk_bicgstab_work_bytes", "hipk_bicgstab_solve",
    "hipk_gmres_work_bytes", "hipk_gmres_solve",
    # step API (row-partitioned multi-GPU CG)
    "hipk_csr_create_ex", "hipk_spmv_ex", "hipk_dot_parts", "hipk_reduce_parts", "hipk_gather",
    "hipk_cg_scal_bytes", "hipk_cg_start", "hipk_cg_update", "hipk_cg_direction", "hipk_cg_xupdate",
    # step API: CG with a callable preconditioner
    "hipk_cgm_start", "hipk_cgm_direction",
    # row-partitioned CG, the loop of one rank in C
    "hipk_dist_cg_work_bytes", "hipk_dist_cg_solve", "hipk_dist_bicgstab_work_bytes", "hipk_dist_bicgstab_solve",
    "hipk_dist_gmres_work_bytes", "hipk_dist_gmres_solve",
    # ... the same three loops with the Jacobi preconditioner
    "hipk_dist_pcg_work_bytes", "hipk_dist_pcg_solve", "hipk_dist_pbicgstab_work_bytes", "hipk_dist_pbicgstab_solve",
    "hipk_dist_pgmres_work_bytes", "hipk_dist_pgmres_solve",
    # ... row-partitioned GMRES at restart 32 .. 255
    "hipk_dist_gmres_wide_work_bytes", "hipk_dist_gmres_wide_solve",
    "hipk_dist_pgmres_wide_work_bytes", "hipk_dist_pgmres_wide_solve",
    # ... the Chebyshev polynomial preconditioner on a row block, and the row-partitioned CG with it
    "hipk_dist_cheb_work_bytes", "hipk_dist_cheb_apply", "hipk_dist_chebcg_work_bytes", "hipk_dist_chebcg_solve",
    # experimental mailbox exchange provider for that loop
    "hipk_p2p_create", "hipk_p2p_create2", "hipk_p2p_export", "hipk_p2p_connect", "hipk_p2p_destroy", "hipk_p2p_error",
    "hipk_p2p_group_start", "hipk_p2p_group_end", "hipk_p2p_all_gather",
    # many right-hand sides per matrix read
    "hipk_multi_work_bytes", "hipk_cg_solve_multi", "hipk_bicgstab_solve_multi",
    # many small systems with one sparsity pattern, one workgroup per system
    "hipk_batch_work_bytes", "hipk_cg_solve_batch", "hipk_bicgstab_solve_batch", "hipk_last_batch_launches",
    "hipk_gmres_batch_work_bytes", "hipk_gmres_solve_batch",
    # ... with the block-Jacobi preconditioner
    "hipk_bj_batch_work_bytes", "hipk_cg_solve_batch_bj", "hipk_bicgstab_solve_batch_bj",
    # aggregation multigrid on a grid: the transfer steps
    "hipk_mg_restrict", "hipk_mg_prolong_add", "hipk_mg_correct", "hipk_mg_diag",
    # ... and the V-cycle's small levels in one launch
    "hipk_mg_tail_work_bytes", "hipk_mg_tail_apply",
    # aggregation multigrid on a matrix graph: the transfers by index arrays, and their tail kernel
    "hipk_mg_restrict_agg", "hipk_mg_prolong_add_agg", "hipk_mg_gtail_work_bytes", "hipk_mg_gtail_apply",
    # ... with a dense coarsest level: z = cinv r as a launch, and as the tail's last level
    "hipk_mg_dense_apply", "hipk_mg_gtail_dense_work_bytes", "hipk_mg_gtail_dense_apply",
    # ... the refresh of a hierarchy for new matrix values: one level's dinv, Gershgorin bound and diagonal check
    "hipk_mg_level_scan_work_bytes", "hipk_mg_level_scan",
    # ... the W-cycle: the sum of the two coarse corrections, and the three tails with the W walk in one launch
    "hipk_mg_add", "hipk_mg_tail_work_bytes_w", "hipk_mg_tail_apply_w", "hipk_mg_gtail_work_bytes_w", "hipk_mg_gtail_apply_w",
    "hipk_mg_gtail_dense_work_bytes_w", "hipk_mg_gtail_dense_apply_w",
]


class Params(ctypes.Structure):
    _fields_ = [
        ("tol", ctypes.c_double),
        ("atol", ctypes.c_double),
        ("maxiter", ctypes.c_int64),
        ("restart", ctypes.c_int32),
        ("gmres_method", ctypes.c_int32),
        ("check_every", ctypes.c_int32),
        ("gpu_tolerances", ctypes.c_int32),
        ("profile", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
    ]


class Stats(ctypes.Structure):
    _fields_ = [
        ("iterations", ctypes.c_int64),
        ("matvecs", ctypes.c_int64),
        ("info", ctypes.c_int32),
        ("breakdown", ctypes.c_int32),
        ("b_norm", ctypes.c_double),
        ("residual_norm", ctypes.c_double),
        ("x_norm", ctypes.c_double),
        ("threshold", ctypes.c_double),
        ("recurrence_rs", ctypes.c_double),
        ("solve_ms", ctypes.c_double),
        ("spmv_ms_avg", ctypes.c_double),
        ("spmv_profiled", ctypes.c_int64),
        ("dispatch_span_ms_avg", ctypes.c_double),
    ]


@dataclass
class SolveStats:
    """Side channel for what the reference never returns."""
    method: str
    iterations: int
    matvecs: int
    info: int
    breakdown: int
    b_norm: float
    residual_norm: float
    x_norm: float
    threshold: float
    recurrence_rs: float
    solve_ms: float
    spmv_ms_avg: float
    spmv_profiled: int
    dispatch_span_ms_avg: float = 0.0
    placement_GBps: float = 0.0    # large systems: what the placement probe read on the allocation the solve ran in (0: not probed)
    placement_tries: int = 0       #   allocations drawn (1: the first one was at the fast level or probing is off)


class HipkError(RuntimeError):
    pass


# hipk_rccl / hipk_dist_plan (include/hipk.h)
COLL_GROUP_FN = ctypes.CFUNCTYPE(ctypes.c_int)
COLL_ALLGATHER_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int,
                                     ctypes.c_void_p, ctypes.c_void_p)
COLL_SENDRECV_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int,
                                    ctypes.c_void_p, ctypes.c_void_p)


class Rccl(ctypes.Structure):
    _fields_ = [("group_start", ctypes.c_void_p), ("group_end", ctypes.c_void_p), ("all_gather", ctypes.c_void_p),
                ("send", ctypes.c_void_p), ("recv", ctypes.c_void_p), ("comm", ctypes.c_void_p), ("fused", ctypes.c_void_p)]


class DistPlan(ctypes.Structure):
    _fields_ = [("rank", ctypes.c_int32), ("world", ctypes.c_int32), ("n_local", ctypes.c_int64), ("n_ext", ctypes.c_int64),
                ("n_global", ctypes.c_int64), ("chunk_rows", ctypes.c_int32), ("g_red", ctypes.c_int32),
                ("per", ctypes.c_int32), ("halo_mode", ctypes.c_int32), ("n_send", ctypes.c_int32),
                ("n_ghost", ctypes.c_int32), ("slab", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("send_idx_dev", ctypes.c_void_p), ("ghost_src_dev", ctypes.c_void_p),
                ("send_off_dev", ctypes.c_void_p), ("dest_off_dev", ctypes.c_void_p),
                ("send_counts", ctypes.POINTER(ctypes.c_int32)), ("recv_counts", ctypes.POINTER(ctypes.c_int32)),
                ("send_first", ctypes.POINTER(ctypes.c_int64))]


# hipk_precond_fn / hipk_op_fn (include/hipk.h): int f(void *user, const void *in_dev, void *out_dev)
class MgLevel(ctypes.Structure):
    """hipk_mg_level: one level of hipk_mg_tail_apply."""
    _fields_ = [("crow", ctypes.c_void_p), ("col", ctypes.c_void_p), ("val", ctypes.c_void_p), ("dinv", ctypes.c_void_p),
                ("n0", ctypes.c_int32), ("n1", ctypes.c_int32), ("n2", ctypes.c_int32), ("n", ctypes.c_int32),
                ("max_row", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("c0", ctypes.c_double), ("c1", ctypes.c_double * 32), ("c2", ctypes.c_double * 32)]


class MgGLevel(ctypes.Structure):
    """hipk_mg_glevel: one level of hipk_mg_gtail_apply."""
    _fields_ = [("crow", ctypes.c_void_p), ("col", ctypes.c_void_p), ("val", ctypes.c_void_p), ("dinv", ctypes.c_void_p),
                ("agg", ctypes.c_void_p), ("aptr", ctypes.c_void_p), ("amem", ctypes.c_void_p),
                ("n", ctypes.c_int32), ("max_row", ctypes.c_int32),
                ("c0", ctypes.c_double), ("c1", ctypes.c_double * 32), ("c2", ctypes.c_double * 32)]


PRECOND_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p)
OP_FN = PRECOND_FN


_lib = None


def build(verbose: bool = False) -> str:
    """Compile libhipk.so for gfx950 with hipcc (csrc/Makefile). Works without a GPU."""
    import subprocess
    cmd = ["make", "-C", CSRC_DIR, "-j4"]
    if not verbose:
        cmd.insert(1, "-s")
    subprocess.check_call(cmd)
    return LIB_PATH


def lib():
    """Load libhipk.so; raise loudly when it is missing (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HipkError(
            f"libhipk.so not found at {LIB_PATH}: the MI355X HIP extension is required for CUDA/ROCm tensors "
            f"(build it with `python __graft_entry__.py` or `make -C {CSRC_DIR}`); there is no CPU fallback.")
    L = ctypes.CDLL(LIB_PATH)
    vp, i64, i32, dbl = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_double
    L.hipk_version.restype = i32
    L.hipk_last_error.restype = ctypes.c_char_p
    L.hipk_build_id.restype = ctypes.c_char_p
    L.hipk_last_spmv_kernel.restype = ctypes.c_char_p
    L.hipk_last_solve_path.restype = ctypes.c_char_p
    L.hipk_last_solve_form.restype = ctypes.c_char_p
    if hasattr(L, "hipk_last_cg_fused_directions"):   # (HIPK_LIB_PATH may name an older build: A/B runs against the parent commit)
        L.hipk_last_cg_fused_directions.restype = ctypes.c_int
    if hasattr(L, "hipk_last_cg_fused_kept_p"):
        L.hipk_last_cg_fused_kept_p.restype = ctypes.c_int
    L.hipk_solve_form_count.restype = ctypes.c_int
    L.hipk_solve_form_name.restype = ctypes.c_char_p
    L.hipk_solve_form_name.argtypes = [ctypes.c_int]
    L.hipk_device_count.restype = i32
    L.hipk_csr_create.argtypes = [ctypes.POINTER(vp), i64, i64, i64, vp, vp, i32, vp, i32, vp]
    L.hipk_csr_destroy.argtypes = [vp]
    L.hipk_op_create.argtypes = [ctypes.POINTER(vp), i64, i32, OP_FN, vp, vp]
    L.hipk_placement_probe.argtypes = [i64, vp, vp, vp, i32, i32, ctypes.POINTER(ctypes.c_double), vp]
    for f in (L.hipk_csr_rows, L.hipk_csr_nnz, L.hipk_csr_spmv_bytes, L.hipk_csr_format_bytes):
        f.argtypes = [vp]
        f.restype = i64
    L.hipk_csr_transpose_work_bytes.argtypes = [vp]
    L.hipk_csr_transpose_work_bytes.restype = ctypes.c_size_t
    L.hipk_csr_transpose.argtypes = [vp, vp, vp, vp, vp, ctypes.c_size_t, vp]
    L.hipk_batch_grad_values.argtypes = [i64, i64, vp, vp, i32, vp, i64, vp, i64, vp, i64, i32, vp]
    L.hipk_csr_grad_values.argtypes = [vp, vp, vp, vp, vp]
    L.hipk_last_grad_values_launches.restype = i32
    L.hipk_csr_spmv_path.argtypes = [vp]
    L.hipk_csr_set_path.argtypes = [vp, i32]
    L.hipk_csr_update_values.argtypes = [vp, vp, vp]
    L.hipk_last_csr_update_kind.restype = i32
    L.hipk_last_csr_update_syncs.restype = i32
    L.hipk_csr_revalue_probe.argtypes = [vp, i32, vp]
    L.hipk_chunk_size.argtypes = [i64]
    L.hipk_chunk_count.argtypes = [i64]
    L.hipk_scratch_bytes.restype = ctypes.c_size_t
    L.hipk_spmv.argtypes = [vp, vp, vp, vp]
    L.hipk_spmv_dot.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.hipk_dot.argtypes = [i64, vp, vp, i32, vp, vp, vp]
    L.hipk_axpy.argtypes = [i64, dbl, vp, vp, i32, vp]
    L.hipk_xpby.argtypes = [i64, vp, dbl, vp, i32, vp]
    L.hipk_block_jacobi_apply.argtypes = [i64, i32, vp, vp, vp, i32, vp]
    L.hipk_cheb_apply.argtypes = [vp, i32, vp, ctypes.POINTER(ctypes.c_double), vp, vp, vp, vp]
    for name in ("cg", "bicgstab"):
        wb = getattr(L, f"hipk_{name}_work_bytes")
        wb.argtypes = [i64, i32]
        wb.restype = ctypes.c_size_t
        getattr(L, f"hipk_{name}_solve").argtypes = [vp, vp, vp, vp, ctypes.c_size_t, ctypes.POINTER(Params),
                                                     ctypes.POINTER(Stats), vp]
    L.hipk_gmres_work_bytes.argtypes = [i64, i32, i32]
    L.hipk_gmres_work_bytes.restype = ctypes.c_size_t
    L.hipk_gmres_solve.argtypes = [vp, vp, vp, vp, ctypes.c_size_t, ctypes.POINTER(Params), ctypes.POINTER(Stats), vp]
    L.hipk_pcg_work_bytes.argtypes = [i64, i32]
    L.hipk_pcg_work_bytes.restype = ctypes.c_size_t
    L.hipk_pcg_solve.argtypes = [vp, vp, vp, vp, vp, ctypes.c_size_t, ctypes.POINTER(Params), ctypes.POINTER(Stats), vp]
    L.hipk_pgmres_solve.argtypes = [vp, vp, vp, vp, vp, ctypes.c_size_t, ctypes.POINTER(Params), ctypes.POINTER(Stats), vp]
    L.hipk_pbicgstab_work_bytes.argtypes = [i64, i32]
    L.hipk_pbicgstab_work_bytes.restype = ctypes.c_size_t
    L.hipk_pbicgstab_solve.argtypes = [vp, vp, vp, vp, vp, ctypes.c_size_t, ctypes.POINTER(Params), ctypes.POINTER(Stats), vp]
    L.hipk_pbicgstab_solve_cb.argtypes = [vp, PRECOND_FN, vp, vp, vp, vp, ctypes.c_size_t, ctypes.POINTER(Params),
                                          ctypes.POINTER(Stats), vp]
    L.hipk_pgmres_solve_cb.argtypes = L.hipk_pbicgstab_solve_cb.argtypes
    dbl = ctypes.c_double
    L.hipk_csr_create_ex.argtypes = [ctypes.POINTER(vp), i64, i64, i64, vp, vp, i32, vp, i32, i32, vp]
    L.hipk_spmv_ex.argtypes = [vp, vp, vp, i32, vp, vp, vp, vp, vp, i64, vp]
    L.hipk_dot_parts.argtypes = [i64, i32, vp, vp, i32, vp, vp]
    L.hipk_reduce_parts.argtypes = [vp, i32, vp, vp]
    L.hipk_gather.argtypes = [i64, vp, vp, vp, i32, vp]
    L.hipk_cg_scal_bytes.restype = ctypes.c_size_t
    L.hipk_cg_start.argtypes = [i64, i32, i32, vp, vp, vp, vp, vp, i32, dbl, dbl, i64, vp]
    L.hipk_cg_update.argtypes = [i64, i32, i32, vp, i64, vp, vp, vp, vp, i32, vp]
    L.hipk_cg_direction.argtypes = [i64, i32, i32, vp, i64, i64, vp, vp, vp, vp, vp, i32, vp]
    L.hipk_cg_xupdate.argtypes = [i64, i32, i32, vp, i64, vp, vp, vp, i32, vp]
    L.hipk_cgm_start.argtypes = [i64, i32, i32, vp, vp, vp, vp, vp, vp, i32, dbl, dbl, i64, vp]
    L.hipk_cgm_direction.argtypes = [i64, i32, i32, vp, i64, i64, vp, vp, vp, vp, vp, vp, i32, vp]
    L.hipk_dist_cg_work_bytes.argtypes = [ctypes.POINTER(DistPlan)]
    L.hipk_dist_cg_work_bytes.restype = ctypes.c_size_t
    L.hipk_dist_cg_solve.argtypes = [vp, ctypes.POINTER(DistPlan), ctypes.POINTER(Rccl), vp, vp, vp, ctypes.c_size_t,
                                     ctypes.POINTER(Params), ctypes.POINTER(Stats), vp]
    L.hipk_dist_bicgstab_work_bytes.argtypes = [ctypes.POINTER(DistPlan)]
    L.hipk_dist_bicgstab_work_bytes.restype = ctypes.c_size_t
    L.hipk_dist_bicgstab_solve.argtypes = [vp, ctypes.POINTER(DistPlan), ctypes.POINTER(Rccl), vp, vp, vp, ctypes.c_size_t,
                                           ctypes.POINTER(Params), ctypes.POINTER(Stats), vp]
    for name in ("gmres", "gmres_wide"):
        getattr(L, f"hipk_dist_{name}_work_bytes").argtypes = [ctypes.POINTER(DistPlan), i32]
        getattr(L, f"hipk_dist_{name}_work_bytes").restype = ctypes.c_size_t
        getattr(L, f"hipk_dist_{name}_solve").argtypes = [vp, ctypes.POINTER(DistPlan), ctypes.POINTER(Rccl), vp, vp, vp,
                                                          ctypes.c_size_t, ctypes.POINTER(Params), ctypes.POINTER(Stats), vp]
    for name in ("pcg", "pbicgstab"):
        getattr(L, f"hipk_dist_{name}_work_bytes").argtypes = [ctypes.POINTER(DistPlan)]
        getattr(L, f"hipk_dist_{name}_work_bytes").restype = ctypes.c_size_t
    for name in ("pgmres", "pgmres_wide"):
        getattr(L, f"hipk_dist_{name}_work_bytes").argtypes = [ctypes.POINTER(DistPlan), i32]
        getattr(L, f"hipk_dist_{name}_work_bytes").restype = ctypes.c_size_t
    for name in ("pcg", "pbicgstab", "pgmres", "pgmres_wide"):   # + dinv_ext after the collective struct
        getattr(L, f"hipk_dist_{name}_solve").argtypes = [vp, ctypes.POINTER(DistPlan), ctypes.POINTER(Rccl), vp, vp, vp, vp,
                                                          ctypes.c_size_t, ctypes.POINTER(Params), ctypes.POINTER(Stats), vp]
    for name in ("cheb", "chebcg"):
        getattr(L, f"hipk_dist_{name}_work_bytes").argtypes = [ctypes.POINTER(DistPlan)]
        getattr(L, f"hipk_dist_{name}_work_bytes").restype = ctypes.c_size_t
    coef = ctypes.POINTER(ctypes.c_double)
    L.hipk_dist_cheb_apply.argtypes = [vp, ctypes.POINTER(DistPlan), ctypes.POINTER(Rccl), i32, vp, coef, vp, vp, vp, ctypes.c_size_t, vp]
    L.hipk_dist_chebcg_solve.argtypes = [vp, ctypes.POINTER(DistPlan), ctypes.POINTER(Rccl), i32, vp, coef, vp, vp, vp, ctypes.c_size_t,
                                         ctypes.POINTER(Params), ctypes.POINTER(Stats), vp]
    L.hipk_p2p_create.argtypes = [ctypes.POINTER(vp), i32, i32, ctypes.c_size_t]
    L.hipk_p2p_create2.argtypes = [ctypes.POINTER(vp), i32, i32, ctypes.c_size_t, i32, i32]
    L.hipk_p2p_export.argtypes = [vp, ctypes.c_char_p]
    L.hipk_p2p_connect.argtypes = [vp, ctypes.c_char_p]
    L.hipk_p2p_destroy.argtypes = [vp]
    L.hipk_p2p_error.argtypes = [vp]
    L.hipk_p2p_all_gather.argtypes = [vp, vp, ctypes.c_size_t, i32, vp, vp]
    L.hipk_multi_work_bytes.argtypes = [i64, i32, i32, i32, i32]
    L.hipk_multi_work_bytes.restype = ctypes.c_size_t
    for name in ("cg", "bicgstab"):
        getattr(L, f"hipk_{name}_solve_multi").argtypes = [vp, vp, i32, vp, i64, vp, i64, vp, ctypes.c_size_t, ctypes.POINTER(Params),
                                                          ctypes.POINTER(Stats), ctypes.POINTER(i64), vp]
    L.hipk_batch_work_bytes.argtypes = [i64, i64, i32, i32, i32, i32]
    L.hipk_batch_work_bytes.restype = ctypes.c_size_t
    L.hipk_gmres_batch_work_bytes.argtypes = [i64, i64, i32, i32, i32, i32]
    L.hipk_gmres_batch_work_bytes.restype = ctypes.c_size_t
    for name in ("cg", "bicgstab", "gmres"):
        getattr(L, f"hipk_{name}_solve_batch").argtypes = [i64, i64, vp, vp, vp, i64, vp, i64, i32, vp, i64, vp, i64, i32, vp,
                                                          ctypes.c_size_t, ctypes.POINTER(Params), ctypes.POINTER(Stats), vp]
    L.hipk_bj_batch_work_bytes.argtypes = [i64, i64, i32, i32, i32, i32]
    L.hipk_bj_batch_work_bytes.restype = ctypes.c_size_t
    for name in ("cg", "bicgstab"):
        getattr(L, f"hipk_{name}_solve_batch_bj").argtypes = [i64, i64, vp, vp, vp, i64, vp, i64, i32, i32, vp, i64, vp, i64, i32, vp,
                                                             ctypes.c_size_t, ctypes.POINTER(Params), ctypes.POINTER(Stats), vp]
    L.hipk_mg_restrict.argtypes = [i64, i64, i64, vp, vp, i32, vp]
    L.hipk_mg_prolong_add.argtypes = [i64, i64, i64, dbl, vp, vp, i32, vp]
    L.hipk_mg_correct.argtypes = [i64, dbl, vp, vp, i32, vp]
    L.hipk_mg_diag.argtypes = [i64, dbl, vp, vp, vp, i32, vp]
    L.hipk_mg_tail_work_bytes.argtypes = [ctypes.POINTER(MgLevel), i32, i32]
    L.hipk_mg_tail_work_bytes.restype = ctypes.c_size_t
    L.hipk_mg_tail_apply.argtypes = [ctypes.POINTER(MgLevel), vp, i32, i32, dbl, dbl, vp, vp, i32, vp, ctypes.c_size_t, vp]
    L.hipk_mg_restrict_agg.argtypes = [i64, i64, vp, vp, vp, vp, i32, vp]
    L.hipk_mg_prolong_add_agg.argtypes = [i64, i64, vp, dbl, vp, vp, i32, vp]
    L.hipk_mg_gtail_work_bytes.argtypes = [ctypes.POINTER(MgGLevel), i32, i32]
    L.hipk_mg_gtail_work_bytes.restype = ctypes.c_size_t
    L.hipk_mg_gtail_apply.argtypes = [ctypes.POINTER(MgGLevel), vp, i32, i32, dbl, dbl, vp, vp, i32, vp, ctypes.c_size_t, vp]
    L.hipk_mg_dense_apply.argtypes = [i64, i64, vp, dbl, vp, vp, i32, vp]
    L.hipk_mg_gtail_dense_work_bytes.argtypes = [ctypes.POINTER(MgGLevel), i32, i32]
    L.hipk_mg_gtail_dense_work_bytes.restype = ctypes.c_size_t
    L.hipk_mg_gtail_dense_apply.argtypes = [ctypes.POINTER(MgGLevel), vp, i32, i32, dbl, dbl, vp, i64, vp, vp, i32, vp, ctypes.c_size_t, vp]
    L.hipk_mg_level_scan_work_bytes.argtypes = [i64]
    L.hipk_mg_level_scan_work_bytes.restype = ctypes.c_size_t
    L.hipk_mg_level_scan.argtypes = [i64, vp, vp, vp, i32, i32, vp, vp, vp, ctypes.c_size_t, vp]
    L.hipk_mg_add.argtypes = [i64, vp, vp, i32, vp]
    for name in ("hipk_mg_tail", "hipk_mg_gtail", "hipk_mg_gtail_dense"):      # the W twins: their V entries' signatures
        getattr(L, name + "_work_bytes_w").argtypes = getattr(L, name + "_work_bytes").argtypes
        getattr(L, name + "_work_bytes_w").restype = ctypes.c_size_t
        getattr(L, name + "_apply_w").argtypes = getattr(L, name + "_apply").argtypes
    _lib = L
    return L


def last_solve_path() -> str:
    """The loop that finished this thread's most recent solve (hipk_last_solve_path): a one-launch kernel instantiation,
    a whole-loop kernel or "launch sequence"; "a -> b" when a one-launch kernel handed the solve back."""
    return lib().hipk_last_solve_path().decode()


def last_solve_form() -> str:
    """The form that solve finished in (hipk_last_solve_form): the instantiation of a one-launch kernel's last launch, or which
    launch sequence ("cg three-launch, small", "gmres restart > 31", ...)."""
    return lib().hipk_last_solve_form().decode()


def last_cg_fused_directions() -> int:
    """The iterations of this thread's last CG solve whose direction step ran inside the fused SpMV + update launch
    (hipk_last_cg_fused_directions); 0 when none did."""
    return int(lib().hipk_last_cg_fused_directions())


def last_cg_fused_kept_p() -> int:
    """The iterations of this thread's last CG solve whose fused launch kept p of its uniform tiles in registers for the
    direction tail (hipk_last_cg_fused_kept_p); 0 when none did."""
    return int(lib().hipk_last_cg_fused_kept_p())


def solve_forms() -> list:
    """Every form a single-device solve can report (hipk_solve_form_name; no GPU needed)."""
    L = lib()
    return [L.hipk_solve_form_name(i).decode() for i in range(L.hipk_solve_form_count())]


def _check(rc: int, what: str) -> None:
    if rc != 0:
        msg = lib().hipk_last_error().decode("utf-8", "replace")
        raise HipkError(f"{what} failed (status {rc}): {msg}")


def _stream(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _dtype_code(dt: torch.dtype) -> int:
    if dt == torch.float64:
        return HIPK_F64
    if dt == torch.float32:
        return HIPK_F32
    raise HipkError(f"unsupported dtype {dt}")


def aligned(t: torch.Tensor, align: int = 16) -> torch.Tensor:
    """The operand whose `data_ptr()` goes to libhipk.so: `t` itself (the same object, no copy) when it is contiguous and starts
    `align`-byte aligned, else a fresh contiguous copy of its values.  Never writes to `t`.  The C entry points refuse vectors
    that are not 16-byte aligned (HIPK_ERR_ALIGN: the kernels use 16-byte accesses), and `.contiguous()` keeps a contiguous view
    where it starts -- `buf[1:n + 1]`, a slab `state[n:2 * n]` with odd n -- so every wrapper routes its operands through here."""
    if t.is_contiguous() and t.data_ptr() % align == 0:
        return t
    return t.clone(memory_format=torch.contiguous_format)


class _SolveLock:
    """threading.Lock that refuses re-entry from the thread that holds it: a preconditioner callable that solves
    with the SAME matrix object would otherwise dead-lock (and would share the handle's scratch with the outer solve)."""

    def __init__(self):
        self._lock = threading.Lock()
        self._owner = None

    def __enter__(self):
        me = threading.get_ident()
        if self._owner == me:
            raise HipkError("nested solve on the same matrix from inside a preconditioner: the handle's scratch is in use "
                            "by the outer solve -- give the inner solver its own copy of the matrix (A.clone())")
        self._lock.acquire()
        self._owner = me
        return self

    def __exit__(self, *exc):
        self._owner = None
        self._lock.release()
        return False


class CsrHandle:
    """Owns a hipk_csr_t and keeps the tensors it borrows alive."""

    def __init__(self, crow: torch.Tensor, col: torch.Tensor, val: torch.Tensor, shape):
        if not val.is_cuda:
            raise HipkError("CsrHandle needs CUDA/ROCm tensors")
        self.crow = aligned(crow)
        self.col = aligned(col)
        self.val = aligned(val)     # hipk_csr_create refuses values that are not 16-byte aligned: a view's values are copied
        self.shape = (int(shape[0]), int(shape[1]))
        self.device = val.device
        self.dtype = val.dtype
        if self.crow.dtype != self.col.dtype or self.crow.dtype not in (torch.int32, torch.int64):
            raise HipkError("CSR indices must both be int32 or both int64")
        if self.crow.numel() != self.shape[0] + 1 or self.col.numel() != self.val.numel():
            raise HipkError("inconsistent CSR component sizes")
        self._h = ctypes.c_void_p()
        # the handle owns scratch its solves share (tile sums of the fused dots, the pinned signal words): one solve
        # at a time per handle; ctypes drops the GIL during a solve, so threads are serialised here
        self._lock = _SolveLock()
        with torch.cuda.device(self.device):
            rc = lib().hipk_csr_create(ctypes.byref(self._h), self.shape[0], self.shape[1], self.val.numel(),
                                       self.crow.data_ptr(), self.col.data_ptr(), self.crow.element_size(),
                                       self.val.data_ptr(), _dtype_code(self.dtype), _stream(self.device))
        _check(rc, "hipk_csr_create")

    @property
    def ptr(self):
        return self._h

    @property
    def n(self) -> int:
        return self.shape[0]

    @property
    def nnz(self) -> int:
        return int(self.val.numel())

    def spmv_bytes(self) -> int:
        return int(lib().hipk_csr_spmv_bytes(self._h))

    PATHS = {0: "tile_fast", 1: "tile", 2: "rowwave", 3: "coded", 4: "offset_coded"}

    def path(self) -> str:
        """SpMV kernel family selected by the structure analysis (include/hipk.h, hipk_spmv_path)."""
        return self.PATHS[int(lib().hipk_csr_spmv_path(self._h))]

    @staticmethod
    def last_spmv_kernel() -> str:
        """Kernel instantiation this thread's most recent SpMV launch selected (hipk_last_spmv_kernel)."""
        return lib().hipk_last_spmv_kernel().decode()

    def set_path(self, plain_only: bool) -> None:
        """plain_only=True: never use the coded form (A/B measurements, parity tests)."""
        _check(lib().hipk_csr_set_path(self._h, 1 if plain_only else 0), "hipk_csr_set_path")

    def format_bytes(self) -> int:
        """Bytes one SpMV moves in the format the selected path streams."""
        return int(lib().hipk_csr_format_bytes(self._h))

    def device_bytes(self) -> int:
        """Device memory this handle keeps alive: the CSR component tensors, the library's int32 index copies and
        tile-sum scratch, and the coded planes (format_bytes minus the two vectors an SpMV also moves)."""
        n, nnz, sv = self.shape[0], self.nnz, self.val.element_size()
        b = (self.crow.numel() + self.col.numel()) * self.crow.element_size() + nnz * sv
        b += 4 * (n + 1) + 4 * nnz + 64 * ((n + 255) // 256 + 1)
        if self.path() in ("coded", "offset_coded"):
            b += max(0, self.format_bytes() - 2 * n * sv)
        # what the handle keeps for `update_values`: the dictionary build table (hipk_dict_table: 2048 slots of 24 bytes + three
        # counters; kept by every handle that made a dictionary attempt, counted for all: a bound for those with a row of more than
        # 32 entries) and, with a coded form, the sliced-ELL plane offsets and the uniform-tile words whether or not the SpMV reads them
        if n > 0 and nnz > 0:
            b += 2048 * 24 + 12
            if self.path() in ("coded", "offset_coded"):
                b += 12 * ((n + 255) // 256 + 1) + 8
        return int(b)

    def update_values(self, values: torch.Tensor) -> "CsrHandle":
        """New values on this handle's pattern (hipk_csr_update_values): afterwards the handle is the one a fresh `CsrHandle` on
        the same index tensors and `values` would be -- same path, same kernels, same bits -- without the pattern-dependent half of
        a creation.  `values` may be the tensor the handle already holds, changed in place.  Returns self."""
        if not isinstance(values, torch.Tensor) or values.dtype != self.dtype:
            raise ValueError(f"update_values: dtype {getattr(values, 'dtype', type(values))} differs from the handle's {self.dtype}")
        if values.device != self.device:
            raise ValueError(f"update_values: device {values.device} differs from the handle's {self.device}")
        if values.dim() != 1 or values.numel() != self.val.numel():
            raise ValueError(f"update_values: {tuple(values.shape)} values differ from the handle's nnz {self.val.numel()}")
        val = aligned(values)       # a misaligned view's values are copied, as in the constructor
        with self._lock, torch.cuda.device(self.device):
            rc = lib().hipk_csr_update_values(self._h, val.data_ptr(), _stream(self.device))
            _check(rc, "hipk_csr_update_values")
            self.val = val
            self._transposed = None     # it holds a gathered copy of the old values
        return self

    @staticmethod
    def last_update_kind() -> int:
        """1 values only, 2 re-encoded in place, 3 the form changed (hipk_last_csr_update_kind); 0 before this thread's first."""
        return int(lib().hipk_last_csr_update_kind())

    def transposed(self) -> "CsrHandle":
        """Handle of A^T, built on the device from this handle's int32 arrays (hipk_csr_transpose: stable sort of the entries
        by column, so the rows of A^T come out column-sorted) and cached here: the adjoint solve of every backward pass
        reuses it (`ImplicitAdjointFunction.backward`, TSL:1237-1248)."""
        ht = getattr(self, "_transposed", None)
        if ht is not None:
            return ht
        L = lib()
        n_rows, n_cols = self.shape
        with torch.cuda.device(self.device):
            crow_t = torch.empty(n_cols + 1, dtype=torch.int32, device=self.device)
            col_t = torch.empty(max(self.nnz, 1), dtype=torch.int32, device=self.device)[:self.nnz]
            val_t = torch.empty(max(self.nnz, 1), dtype=self.dtype, device=self.device)[:self.nnz]
            wb = int(L.hipk_csr_transpose_work_bytes(self._h))
            work = torch.empty(wb, dtype=torch.uint8, device=self.device)
            _check(L.hipk_csr_transpose(self._h, crow_t.data_ptr(), col_t.data_ptr(), val_t.data_ptr(), work.data_ptr(), wb,
                                        _stream(self.device)), "hipk_csr_transpose")
            ht = CsrHandle(crow_t, col_t, val_t, (n_cols, n_rows))
        del work
        self._transposed = ht
        return ht

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            try:
                lib().hipk_csr_destroy(self._h)
            finally:
                self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# -------------------------------------------------------------------- handle cache
# Repeated solves with the same matrix (the LDC stepper: one matrix, thousands of RHS)
# reuse the analysed handle.  Keyed on storage identity + version counters + the VIEW
# (strides, storage offset, conj/neg bits): a dense `A` and its view `A.T` share storage
# and version but are different matrices (the adjoint solve of the implicit-diff backward,
# TSL:1245, asks for exactly that pair).
# The cache pins the source tensors and the handles' own device arrays (int32 index copies,
# coded planes): it is bounded by entries AND by bytes (HIPK_CACHE_BYTES, default 8 GiB; the
# most recent handle is always kept).  `clear_cache()` drops everything.
_CACHE: "collections.OrderedDict[tuple, tuple]" = collections.OrderedDict()
_CACHE_MAX = 8
_CACHE_BYTES_DEFAULT = 8 << 30


def _cache_budget() -> int:
    try:
        return int(os.environ.get("HIPK_CACHE_BYTES", _CACHE_BYTES_DEFAULT))
    except ValueError:
        return _CACHE_BYTES_DEFAULT


def _part_key(p: torch.Tensor):
    return (p.data_ptr(), p._version, p.numel(), tuple(p.stride()), p.storage_offset(), p.is_conj(), p.is_neg())


def _cache_key(A: torch.Tensor):
    if A.layout == torch.sparse_csr:
        parts = (A.crow_indices(), A.col_indices(), A.values())
    elif A.layout == torch.sparse_coo:
        parts = (A._indices(), A._values())
    elif A.layout == torch.sparse_csc:          # e.g. the transpose view of a CSR matrix (adjoint solves)
        parts = (A.ccol_indices(), A.row_indices(), A.values())
    elif A.layout == torch.strided:
        parts = (A,)
    else:
        raise HipkError(f"unsupported tensor layout {A.layout}")
    return (str(A.layout), tuple(A.shape), str(A.device), A.dtype) + tuple(_part_key(p) for p in parts)


def _pinned_bytes(h: "CsrHandle", src: torch.Tensor) -> int:
    """Device bytes an entry keeps alive: the handle's arrays + (when it was converted) the source tensor."""
    b = h.device_bytes()
    if src.layout == torch.strided:
        b += src.numel() * src.element_size()
    elif src.layout == torch.sparse_coo:
        b += src._indices().numel() * 8 + src._values().numel() * src._values().element_size()
    return b


def _store(key, h: "CsrHandle", src: torch.Tensor) -> None:
    _CACHE[key] = (h, src, _pinned_bytes(h, src))  # keep the source alive so its pointers cannot be recycled
    budget = _cache_budget()
    while len(_CACHE) > 1 and (len(_CACHE) > _CACHE_MAX or sum(e[2] for e in _CACHE.values()) > budget):
        _CACHE.popitem(last=False)


def handle_for(A: torch.Tensor) -> CsrHandle:
    """CSR handle of a CUDA tensor in any layout (dense / COO / CSR / CSC), converted once and cached."""
    key = _cache_key(A)
    hit = _CACHE.get(key)
    if hit is not None:
        _CACHE.move_to_end(key)
        return hit[0]
    src = A.detach()
    # transposed views (what the adjoint solve of the implicit-diff backward passes, TSL:1245): the handle of the base
    # matrix, transposed on the device -- no torch CSC -> CSR re-conversion, no second dense -> CSR pass
    if src.layout == torch.sparse_csc and src.dim() == 2:
        base = torch.sparse_csr_tensor(src.ccol_indices(), src.row_indices(), src.values(),
                                       size=(src.shape[1], src.shape[0]), check_invariants=False)
        h = handle_for(base).transposed()
        _store(key, h, src)
        return h
    if (src.layout == torch.strided and src.dim() == 2 and not src.is_contiguous() and src.t().is_contiguous()
            and not src.is_conj() and not src.is_neg()):
        h = handle_for(src.t()).transposed()
        _store(key, h, src)
        return h
    if src.layout == torch.sparse_csr:
        csr = src
    elif src.layout == torch.sparse_coo:
        csr = src.coalesce().to_sparse_csr()
    elif src.layout == torch.strided:
        csr = src.resolve_conj().resolve_neg().to_sparse_csr()
    else:
        csr = src.to_sparse_csr()
    h = CsrHandle(csr.crow_indices(), csr.col_indices(), csr.values(), csr.shape)
    _store(key, h, src)
    return h


def _no_version(part_key):
    return part_key[:1] + part_key[2:]


def _same_but_version(k1, k2) -> bool:
    """Two cache keys that agree in everything but the version counters (field 1 of a part key).  `crow_indices()`,
    `col_indices()` and `values()` of a sparse tensor all report the SPARSE tensor's counter, so an in-place change of the values
    moves all three: the counter cannot say which component was written, the caller of refresh_matrix does."""
    return len(k1) == len(k2) and k1[:4] == k2[:4] and all(_no_version(a) == _no_version(b) for a, b in zip(k1[4:], k2[4:]))


def refresh_matrix(A: torch.Tensor, like: Optional[torch.Tensor] = None) -> bool:
    """Give the cached handle of a CSR matrix new values instead of letting the next solve build a new handle.

    like=None: `A`'s values were changed in place (`A.values().mul_(2)`).  The cache entry whose key equals A's in everything but
    the version counter is updated (`CsrHandle.update_values`) and re-keyed, and entries of other views of the same values (the transpose an
    adjoint solve cached) are dropped; True.  No such entry: False, and the next solve
    builds a handle as it always did.
    like=A_old: `A` is a CSR tensor on A_old's index tensors -- `crow_indices()` / `col_indices()` the same tensors, compared by
    identity (pointer, size, view: their part keys without the version counter, which is the sparse tensor's, not theirs), never by contents -- with values of its own.  A takes over A_old's cached handle; a later
    solve with A_old builds a new one.  True, or False when A_old has no cached handle.  Another layout, shape, dtype or device,
    or index tensors of their own: ValueError."""
    if not isinstance(A, torch.Tensor) or A.layout != torch.sparse_csr:
        raise ValueError(f"refresh_matrix: A must be a sparse CSR tensor, not {getattr(A, 'layout', type(A))}")
    key = _cache_key(A)
    if like is None:
        if key in _CACHE:
            return True                 # nothing changed since the handle was built or refreshed
        stale = [k for k in _CACHE if _same_but_version(k, key)]       # A solved at several versions: every one of them is stale
        old_key = stale[-1] if stale else None                         # the most recently used takes the new values ...
        for k in stale[:-1]:                                           # ... the others are dropped
            del _CACHE[k]
    else:
        if not isinstance(like, torch.Tensor) or like.layout != torch.sparse_csr:
            raise ValueError(f"refresh_matrix: like must be a sparse CSR tensor, not {getattr(like, 'layout', type(like))}")
        for what, a, b in (("shape", tuple(A.shape), tuple(like.shape)), ("dtype", A.dtype, like.dtype),
                           ("device", A.device, like.device)):
            if a != b:
                raise ValueError(f"refresh_matrix: {what} {a} differs from like's {b}")
        old_key = _cache_key(like)
        if [_no_version(p) for p in old_key[4:6]] != [_no_version(p) for p in key[4:6]]:
            raise ValueError("refresh_matrix: A must share like's crow_indices() and col_indices() tensors (the same storage, "
                             "same view); it has index tensors of its own")
        if old_key == key:
            return key in _CACHE
    hit = _CACHE.get(old_key) if old_key is not None else None
    if hit is None:
        return False
    h = hit[0]
    h.update_values(A.values().detach())
    if like is None:
        # other entries on the same values -- the transposed view an adjoint solve asked for, and the CSR tensor handle_for made of
        # it, which counts its own versions -- hold handles of the old numbers: dropped, the next backward pass rebuilds them
        vptr = A.values().data_ptr()
        for k in [k for k in _CACHE if k not in (key, old_key) and any(p[0] == vptr for p in k[4:])]:
            del _CACHE[k]
    del _CACHE[old_key]
    _store(key, h, A.detach())
    return True


def clear_cache() -> None:
    """Drop every cached handle (and the source matrices / index copies / coded planes they pin on the GPU)."""
    _CACHE.clear()


def cache_info():
    """(entries, pinned device bytes) of the handle cache."""
    return len(_CACHE), sum(e[2] for e in _CACHE.values())


# -------------------------------------------------------------------- primitives
def scratch(device) -> torch.Tensor:
    return torch.empty(int(lib().hipk_scratch_bytes()), dtype=torch.uint8, device=device)


def spmv(h: CsrHandle, x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    assert x.is_contiguous() and x.dtype == h.dtype and x.numel() == h.shape[1]
    y = torch.empty(h.shape[0], dtype=h.dtype, device=h.device) if out is None else out
    with torch.cuda.device(h.device):
        _check(lib().hipk_spmv(h.ptr, x.data_ptr(), y.data_ptr(), _stream(h.device)), "hipk_spmv")
    return y


def spmv_dot(h: CsrHandle, x: torch.Tensor, w: torch.Tensor):
    """(A x, <w, A x>) with the dot fused into the SpMV epilogue."""
    y = torch.empty(h.shape[0], dtype=h.dtype, device=h.device)
    out = torch.empty(1, dtype=torch.float64, device=h.device)
    sc = scratch(h.device)
    with torch.cuda.device(h.device):
        _check(lib().hipk_spmv_dot(h.ptr, x.data_ptr(), y.data_ptr(), w.data_ptr(), out.data_ptr(), sc.data_ptr(),
                                   _stream(h.device)), "hipk_spmv_dot")
    return y, out


def dot(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    assert x.is_cuda and x.is_contiguous() and y.is_contiguous() and x.dtype == y.dtype and x.numel() == y.numel()
    out = torch.empty(1, dtype=torch.float64, device=x.device)
    sc = scratch(x.device)
    with torch.cuda.device(x.device):
        _check(lib().hipk_dot(x.numel(), x.data_ptr(), y.data_ptr(), _dtype_code(x.dtype), out.data_ptr(),
                              sc.data_ptr(), _stream(x.device)), "hipk_dot")
    return out


def axpy(a: float, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """y <- y + a*x in place."""
    with torch.cuda.device(x.device):
        _check(lib().hipk_axpy(x.numel(), float(a), x.data_ptr(), y.data_ptr(), _dtype_code(x.dtype),
                               _stream(x.device)), "hipk_axpy")
    return y


def xpby(x: torch.Tensor, b: float, y: torch.Tensor) -> torch.Tensor:
    """y <- x + b*y in place."""
    with torch.cuda.device(x.device):
        _check(lib().hipk_xpby(x.numel(), x.data_ptr(), float(b), y.data_ptr(), _dtype_code(x.dtype),
                               _stream(x.device)), "hipk_xpby")
    return y


def block_jacobi_apply(binv: torch.Tensor, block_size: int, v: torch.Tensor) -> torch.Tensor:
    """z = blockdiag(binv) v on the device (hipk_block_jacobi_apply); binv: [ceil(n / bs), bs, bs] contiguous."""
    assert v.is_cuda and v.is_contiguous() and binv.is_contiguous() and binv.dtype == v.dtype and binv.device == v.device
    out = torch.empty_like(v)
    with torch.cuda.device(v.device):
        _check(lib().hipk_block_jacobi_apply(v.numel(), int(block_size), binv.data_ptr(), v.data_ptr(), out.data_ptr(),
                                             _dtype_code(v.dtype), _stream(v.device)), "hipk_block_jacobi_apply")
    return out


def cheb_apply(h: CsrHandle, degree: int, dinv: torch.Tensor, coef, v: torch.Tensor, work: Optional[torch.Tensor] = None,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """z = p_m(D^-1 A) D^-1 v on the device (hipk_cheb_apply), enqueued on the current stream.  `coef`: a ctypes array of
    2 * degree + 2 doubles (c0, c1[1..m], c2[1..m], scale).  Takes no lock and touches none of the handle's reduction scratch:
    it is what a solve that HOLDS the handle calls as its preconditioner.  `work`: None or the caller's two work vectors, a
    contiguous uint8 tensor on the handle's device, 16-byte aligned, of at least 2 * ((n + 3) & ~3) elements' bytes; `out`: None
    or where z goes (contiguous, 16-byte aligned, n elements)."""
    assert v.is_cuda and v.dtype == h.dtype and v.device == h.device and v.numel() == h.n and h.shape[0] == h.shape[1]
    assert dinv.is_contiguous() and dinv.dtype == v.dtype and dinv.device == v.device and dinv.numel() == h.n
    assert len(coef) == 2 * int(degree) + 2
    v = aligned(v)
    if out is None:
        out = torch.empty_like(v)
    assert out.is_contiguous() and out.dtype == v.dtype and out.device == v.device and out.numel() == h.n and out.data_ptr() % 16 == 0
    work = _workspace(work, v.device, 2 * ((h.n + 3) & ~3) * v.element_size(), 16)   # ordered by the stream, as the launches are
    with torch.cuda.device(v.device):
        _check(lib().hipk_cheb_apply(h.ptr, int(degree), dinv.data_ptr(), coef, v.data_ptr(), out.data_ptr(), work.data_ptr(),
                                     _stream(v.device)), "hipk_cheb_apply")
    return out


@dataclass
class GradStats:
    """Side channel of the matrix-gradient step of a backward pass (`get_last_grad_stats()`): the route that formed the gradient
    ("kernel": hipk_csr_vgrad_kernel, or "torch": the torch expression of the same formula), the kernel launches it took (0 on the
    torch route), the stored entries per matrix and the number of systems.  One per process, NOT per thread: autograd runs backward
    on a thread of its own, where a thread-local record would be invisible to the caller."""
    route: str
    launches: int
    nnz: int
    batch: int


_last_grad_stats: Optional[GradStats] = None


def last_grad_stats() -> Optional[GradStats]:
    return _last_grad_stats


def set_grad_stats(route: str, launches: int, nnz: int, batch: int) -> None:
    global _last_grad_stats
    _last_grad_stats = GradStats(route=route, launches=int(launches), nnz=int(nnz), batch=int(batch))


def csr_grad_values(h: CsrHandle, lam: torch.Tensor, x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """hipk_csr_grad_values: out[k] = -(lam[row(k)] * x[col(k)]) for the nnz stored entries of the handle's matrix, in the handle's
    dtype (lam of n_rows, x of n_cols elements are cast to it).  `out`, if given, receives the values (through an aligned
    temporary when it is a misaligned or strided view)."""
    lam = aligned(lam.detach().to(device=h.device, dtype=h.dtype))
    x = aligned(x.detach().to(device=h.device, dtype=h.dtype))
    if lam.dim() != 1 or x.dim() != 1 or lam.numel() != h.shape[0] or x.numel() != h.shape[1]:
        raise HipkError(f"csr_grad_values: lam must have {h.shape[0]} and x {h.shape[1]} elements, got {tuple(lam.shape)} and {tuple(x.shape)}")
    if out is not None and (out.dim() != 1 or out.numel() != h.nnz or out.dtype != h.dtype or out.device != h.device):
        raise HipkError(f"csr_grad_values: out must be a {h.dtype} vector of {h.nnz} elements on {h.device}")
    direct = out is not None and out.is_contiguous() and out.data_ptr() % 16 == 0
    g = out if direct else torch.empty(h.nnz, dtype=h.dtype, device=h.device)
    L = lib()
    with torch.cuda.device(h.device):
        rc = L.hipk_csr_grad_values(h.ptr, lam.data_ptr(), x.data_ptr(), g.data_ptr(), _stream(h.device))
    _check(rc, "hipk_csr_grad_values")
    set_grad_stats("kernel", L.hipk_last_grad_values_launches(), h.nnz, 1)
    if out is not None and not direct:
        out.copy_(g)
        return out
    return g


def batch_grad_values(n: int, nnz: int, crow32: torch.Tensor, col32: torch.Tensor, lam: torch.Tensor, x: torch.Tensor,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """hipk_batch_grad_values: out[s, k] = -(lam[s, row(k)] * x[s, col(k)]) for S systems of n rows on one pattern (int32 crow (n + 1,),
    col (nnz,)); lam, x (S, n) of one dtype (fp64 or fp32) on one device, out (S, nnz).  Rows that do not start 16-byte aligned go
    through padded copies, as in the batch solves."""
    from .module_a.batch import _aligned_rows, _pad_rows
    dev, dt = lam.device, lam.dtype
    if lam.dim() != 2 or x.dim() != 2 or lam.shape != x.shape or lam.shape[1] != n or x.dtype != dt or x.device != dev:
        raise HipkError(f"batch_grad_values: lam and x must both be (S, {n}) tensors of one dtype on one device")
    S = int(lam.shape[0])
    assert crow32.dtype == torch.int32 and col32.dtype == torch.int32 and crow32.numel() == n + 1 and col32.numel() == nnz
    assert crow32.device == dev and col32.device == dev
    if out is not None and (tuple(out.shape) != (S, nnz) or out.dtype != dt or out.device != dev):
        raise HipkError(f"batch_grad_values: out must be a ({S}, {nnz}) {dt} tensor on {dev}")
    crow32, col32 = aligned(crow32), aligned(col32)
    lam, x = _pad_rows(lam.detach()), _pad_rows(x.detach())
    direct = out is not None and _aligned_rows(out)
    if direct:
        g = out
    else:       # a fresh buffer whose rows start 16-byte aligned: allocated padded, never initialised (the kernel writes every [s, k < nnz])
        per = 16 // lam.element_size()
        g = torch.empty((S, (nnz + per - 1) // per * per), dtype=dt, device=dev)[:, :nnz]
    ld = lambda t: int(t.stride(0)) if t.shape[0] > 1 else max(int(t.stride(0)), int(t.shape[1]))
    L = lib()
    with torch.cuda.device(dev):
        rc = L.hipk_batch_grad_values(int(n), int(nnz), crow32.data_ptr(), col32.data_ptr(), S, lam.data_ptr(), ld(lam), x.data_ptr(), ld(x),
                                      g.data_ptr(), ld(g), _dtype_code(dt), _stream(dev))
    _check(rc, "hipk_batch_grad_values")
    set_grad_stats("kernel", L.hipk_last_grad_values_launches(), nnz, S)
    if out is not None and not direct:
        out.copy_(g)
        return out
    return g


def spmv_residual(h: CsrHandle, x: torch.Tensor, b: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """out = b - A x, the SpMV's residual form (hipk_spmv_ex, mode 4), on the current stream.  No fused dot, so it takes no lock
    and touches none of the handle's reduction scratch: a preconditioner may call it inside a solve that holds the handle."""
    for v in (x, b, out):
        assert v.is_contiguous() and v.dtype == h.dtype and v.device == h.device and v.numel() == h.n
    with torch.cuda.device(h.device):
        _check(lib().hipk_spmv_ex(h.ptr, x.data_ptr(), out.data_ptr(), 4, None, b.data_ptr(), None, None, None, 0,
                                  _stream(h.device)), "hipk_spmv_ex")
    return out


def _grid3(dims):
    """(n0, n1, n2) of a 2- or 3-dimensional grid, slowest dimension first (a two-dimensional one has n0 = 1)."""
    d = tuple(int(v) for v in dims)
    return (1,) * (3 - len(d)) + d


def mg_restrict(dims, t: torch.Tensor, rc: torch.Tensor) -> torch.Tensor:
    """rc[I] = the sum of t over aggregate I in ascending fine index (hipk_mg_restrict); `dims` is the FINE grid."""
    n0, n1, n2 = _grid3(dims)
    assert t.is_cuda and t.is_contiguous() and rc.is_contiguous() and rc.dtype == t.dtype and rc.device == t.device
    assert t.numel() == n0 * n1 * n2 and rc.numel() == ((n0 + 1) // 2) * ((n1 + 1) // 2) * ((n2 + 1) // 2)
    with torch.cuda.device(t.device):
        _check(lib().hipk_mg_restrict(n0, n1, n2, t.data_ptr(), rc.data_ptr(), _dtype_code(t.dtype), _stream(t.device)),
               "hipk_mg_restrict")
    return rc


def mg_prolong_add(dims, omega: float, e: torch.Tensor, z: torch.Tensor) -> torch.Tensor:
    """z[i] += omega * e[agg(i)] in place (hipk_mg_prolong_add); `dims` is the FINE grid, z's."""
    n0, n1, n2 = _grid3(dims)
    assert z.is_cuda and z.is_contiguous() and e.is_contiguous() and e.dtype == z.dtype and e.device == z.device
    assert z.numel() == n0 * n1 * n2 and e.numel() == ((n0 + 1) // 2) * ((n1 + 1) // 2) * ((n2 + 1) // 2)
    with torch.cuda.device(z.device):
        _check(lib().hipk_mg_prolong_add(n0, n1, n2, float(omega), e.data_ptr(), z.data_ptr(), _dtype_code(z.dtype),
                                         _stream(z.device)), "hipk_mg_prolong_add")
    return z


def mg_correct(scale: float, d: torch.Tensor, z: torch.Tensor) -> torch.Tensor:
    """z = scale * (z + d) in place (hipk_mg_correct)."""
    assert z.is_cuda and z.is_contiguous() and d.is_contiguous() and d.dtype == z.dtype and d.device == z.device and d.numel() == z.numel()
    with torch.cuda.device(z.device):
        _check(lib().hipk_mg_correct(z.numel(), float(scale), d.data_ptr(), z.data_ptr(), _dtype_code(z.dtype), _stream(z.device)),
               "hipk_mg_correct")
    return z


def mg_diag(scale: float, dinv: torch.Tensor, r: torch.Tensor, z: torch.Tensor) -> torch.Tensor:
    """z = scale * (dinv * r) (hipk_mg_diag)."""
    assert z.is_cuda and all(v.is_contiguous() and v.dtype == z.dtype and v.device == z.device and v.numel() == z.numel() for v in (dinv, r, z))
    with torch.cuda.device(z.device):
        _check(lib().hipk_mg_diag(z.numel(), float(scale), dinv.data_ptr(), r.data_ptr(), z.data_ptr(), _dtype_code(z.dtype),
                                  _stream(z.device)), "hipk_mg_diag")
    return z


MG_TAIL_MAX_N = 4096      # the envelope of hipk_mg_tail_apply: unknowns per level ...
MG_TAIL_MAX_ROW = 32      # ... and stored entries per row (the batch kernels')


class _MgDescriptors:
    """What `MgTail` and `MgGTail` share: the descriptors of a run of levels on the host (`host`) and as one device blob (`blob`),
    the tensors they point into, and `work_bytes` of the entry point that takes them."""

    def _build(self, struct, levels, nsparse: int, degree: int, dtype, device, work_bytes: str, cycle: str = "V") -> None:
        """Levels [0, nsparse) are dicts with int32 `crow` / `col`, `val`, `dinv` (contiguous device tensors of one dtype),
        `max_row` and the smoother's `c0`, `c1`, `c2` (absent or None where there is no smoother): the fields both descriptor
        structs have.  A level past them is a dict of which only `n` is read.  `self._level(j, d, lev, nc)` then fills what only
        one kind of level has; `nc` is the next level's size, None on the last.  `cycle` "W": `work_bytes` of the entry's W twin
        (six vectors per level, at most `MG_TAIL_W_MAX_LEVELS` levels)."""
        assert cycle in ("V", "W"), cycle
        self.nlev, self.degree, self.dtype, self.device, self.cycle = len(levels), int(degree), dtype, device, cycle
        sizes = [int(lev["dinv"].numel()) for lev in levels[:nsparse]] + [int(lev["n"]) for lev in levels[nsparse:]]
        self.host = (struct * self.nlev)()
        self._keep = []
        for j, (d, lev) in enumerate(zip(self.host, levels)):
            d.n = sizes[j]
            if j >= nsparse:
                continue
            for name in ("crow", "col", "val", "dinv"):
                t = lev[name]
                assert t.is_cuda and t.is_contiguous() and t.device == device
                assert t.dtype == (torch.int32 if name in ("crow", "col") else dtype)
                self._keep.append(t)
                setattr(d, name, t.data_ptr())
            assert lev["crow"].numel() == d.n + 1 and lev["col"].numel() == lev["val"].numel()
            d.max_row = int(lev["max_row"])
            if lev.get("c0") is not None:
                d.c0 = float(lev["c0"])
                for k in range(self.degree):
                    d.c1[k], d.c2[k] = float(lev["c1"][k]), float(lev["c2"][k])
            self._level(j, d, lev, sizes[j + 1] if j + 1 < self.nlev else None)
        raw = torch.frombuffer(bytearray(bytes(self.host)), dtype=torch.uint8)
        self.blob = raw.to(device)
        self.work_bytes = int(getattr(lib(), work_bytes + ("_w" if cycle == "W" else ""))(self.host, self.nlev, _dtype_code(dtype)))


class MgTail(_MgDescriptors):
    """The descriptors of hipk_mg_tail_apply for a run of levels, on the host and as one device blob, and the tensors they point
    into.  `levels`: per level a dict with int32 `crow` / `col`, `val`, `dinv` (contiguous device tensors of one dtype), `dims`
    (2 or 3 entries), `max_row` and the smoother's `c0`, `c1`, `c2` (None on the last level, which has one unknown)."""

    def __init__(self, levels, degree: int, cycle: str = "V"):
        self._build(MgLevel, levels, len(levels), degree, levels[0]["val"].dtype, levels[0]["val"].device, "hipk_mg_tail_work_bytes", cycle)

    def _level(self, j, d, lev, nc) -> None:
        d.n0, d.n1, d.n2 = _grid3(lev["dims"])
        assert d.n == d.n0 * d.n1 * d.n2


def _mg_tail_call(symbol: str, tail, omega: float, scale: float, r: torch.Tensor, z: torch.Tensor, work, *last) -> torch.Tensor:
    """The call of a tail entry point `symbol`; `last` are its arguments between `scale` and `r`."""
    assert tail.cycle == ("W" if symbol.endswith("_w") else "V"), f"the tail was built for cycle {tail.cycle!r}: its workspace is another"
    n = int(tail.host[0].n)
    for v in (r, z):
        assert v.is_cuda and v.is_contiguous() and v.dtype == tail.dtype and v.device == tail.device and v.numel() == n
    work = _workspace(work, tail.device, tail.work_bytes)
    with torch.cuda.device(tail.device):
        _check(getattr(lib(), symbol)(tail.host, tail.blob.data_ptr(), tail.nlev, tail.degree, float(omega), float(scale), *last,
                                      r.data_ptr(), z.data_ptr(), _dtype_code(tail.dtype), work.data_ptr(), tail.work_bytes,
                                      _stream(tail.device)), symbol)
    return z


def mg_tail_apply(tail: MgTail, omega: float, scale: float, r: torch.Tensor, z: torch.Tensor,
                  work: Optional[torch.Tensor] = None) -> torch.Tensor:
    """z = scale * V(0, r) over the tail's levels in one launch (hipk_mg_tail_apply), on the current stream."""
    return _mg_tail_call("hipk_mg_tail_apply", tail, omega, scale, r, z, work)


MG_TAIL_W_MAX_LEVELS = 12  # the W entries' level count: the last of nlev levels is visited 2^(nlev - 2) times in the one launch


def mg_tail_apply_w(tail: MgTail, omega: float, scale: float, r: torch.Tensor, z: torch.Tensor,
                    work: Optional[torch.Tensor] = None) -> torch.Tensor:
    """z = scale * W(0, r) over the levels of a tail built with cycle="W", in one launch (hipk_mg_tail_apply_w)."""
    return _mg_tail_call("hipk_mg_tail_apply_w", tail, omega, scale, r, z, work)


def mg_add(e2: torch.Tensor, e: torch.Tensor) -> torch.Tensor:
    """e = e + e2 in place (hipk_mg_add): the sum of the W-cycle's two coarse corrections."""
    assert e.is_cuda and e.is_contiguous() and e2.is_contiguous() and e2.dtype == e.dtype and e2.device == e.device and e2.numel() == e.numel()
    with torch.cuda.device(e.device):
        _check(lib().hipk_mg_add(e.numel(), e2.data_ptr(), e.data_ptr(), _dtype_code(e.dtype), _stream(e.device)), "hipk_mg_add")
    return e


def _check_index(name: str, a: torch.Tensor, numel: int, like: torch.Tensor) -> None:
    """An int32 index array of the multigrid transfers: dtype, length, device and alignment (its contents are the caller's)."""
    assert a.is_cuda and a.is_contiguous() and a.dtype == torch.int32 and a.device == like.device, f"{name}: a contiguous int32 device tensor"
    assert a.numel() == numel, f"{name}: {a.numel()} entries, {numel} expected"
    assert a.data_ptr() % 16 == 0, f"{name} must be 16-byte aligned"


def mg_restrict_agg(aptr: torch.Tensor, amem: torch.Tensor, t: torch.Tensor, rc: torch.Tensor) -> torch.Tensor:
    """rc[I] = the sum of t over amem[aptr[I] : aptr[I + 1]], left to right from the first member (hipk_mg_restrict_agg)."""
    assert t.is_cuda and t.is_contiguous() and rc.is_contiguous() and rc.dtype == t.dtype and rc.device == t.device
    assert t.data_ptr() % 16 == 0 and rc.data_ptr() % 16 == 0
    _check_index("aptr", aptr, rc.numel() + 1, t)
    _check_index("amem", amem, t.numel(), t)
    with torch.cuda.device(t.device):
        _check(lib().hipk_mg_restrict_agg(t.numel(), rc.numel(), aptr.data_ptr(), amem.data_ptr(), t.data_ptr(), rc.data_ptr(),
                                          _dtype_code(t.dtype), _stream(t.device)), "hipk_mg_restrict_agg")
    return rc


def mg_prolong_add_agg(agg: torch.Tensor, omega: float, e: torch.Tensor, z: torch.Tensor) -> torch.Tensor:
    """z[i] += omega * e[agg[i]] in place (hipk_mg_prolong_add_agg)."""
    assert z.is_cuda and z.is_contiguous() and e.is_contiguous() and e.dtype == z.dtype and e.device == z.device
    assert z.data_ptr() % 16 == 0 and e.data_ptr() % 16 == 0
    _check_index("agg", agg, z.numel(), z)
    with torch.cuda.device(z.device):
        _check(lib().hipk_mg_prolong_add_agg(z.numel(), e.numel(), agg.data_ptr(), float(omega), e.data_ptr(), z.data_ptr(),
                                             _dtype_code(z.dtype), _stream(z.device)), "hipk_mg_prolong_add_agg")
    return z


MG_GTAIL_MAX_LEVELS = 32  # the envelope of hipk_mg_gtail_apply beyond MG_TAIL_MAX_N / MG_TAIL_MAX_ROW: levels


class MgGTail(_MgDescriptors):
    """`MgTail` for hipk_mg_gtail_apply: per level a dict with int32 `crow` / `col`, `val`, `dinv`, `max_row`, the smoother's `c0`,
    `c1`, `c2` and the int32 index arrays `agg`, `aptr`, `amem` to the next level (all four absent or None on the last level).

    `cinv` (with `ld`): the descriptors of hipk_mg_gtail_dense_apply instead.  The last entry of `levels` is then the dense level,
    a dict of which only `n` is read, and `cinv` its stored inverse (`mg_dense_apply`'s layout)."""

    def __init__(self, levels, degree: int, cinv: Optional[torch.Tensor] = None, ld: int = 0, cycle: str = "V"):
        self.cinv, self.ld = cinv, int(ld)
        if cinv is not None:
            _check_cinv(cinv, int(levels[-1]["n"]), self.ld)
        like = levels[0]["val"] if cinv is None else cinv
        self._build(MgGLevel, levels, len(levels) - (cinv is not None), degree, like.dtype, like.device,
                    "hipk_mg_gtail_work_bytes" if cinv is None else "hipk_mg_gtail_dense_work_bytes", cycle)

    def _level(self, j, d, lev, nc) -> None:
        if nc is not None:
            assert lev.get("c0") is not None, "a level that has a next one needs the smoother's coefficients"
            for name, numel in (("agg", d.n), ("aptr", nc + 1), ("amem", d.n)):
                _check_index(name, lev[name], numel, lev["val"])
                self._keep.append(lev[name])
                setattr(d, name, lev[name].data_ptr())


def mg_gtail_apply(tail: MgGTail, omega: float, scale: float, r: torch.Tensor, z: torch.Tensor,
                   work: Optional[torch.Tensor] = None) -> torch.Tensor:
    """z = scale * V(0, r) over the tail's index-array levels in one launch (hipk_mg_gtail_apply), on the current stream."""
    assert tail.cinv is None, "the tail was built with a dense level: mg_gtail_dense_apply"
    return _mg_tail_call("hipk_mg_gtail_apply", tail, omega, scale, r, z, work)


def mg_gtail_apply_w(tail: MgGTail, omega: float, scale: float, r: torch.Tensor, z: torch.Tensor,
                     work: Optional[torch.Tensor] = None) -> torch.Tensor:
    """z = scale * W(0, r) over the index-array levels of a tail built with cycle="W", in one launch (hipk_mg_gtail_apply_w)."""
    assert tail.cinv is None, "the tail was built with a dense level: mg_gtail_dense_apply_w"
    return _mg_tail_call("hipk_mg_gtail_apply_w", tail, omega, scale, r, z, work)


MG_DENSE_MAX_N = 2048     # the envelope of hipk_mg_dense_apply: unknowns of the dense level ...
MG_DENSE_TAIL_N = 512     # ... and of hipk_mg_gtail_dense_apply's last level


def _check_cinv(cinv: torch.Tensor, n: int, ld: int) -> None:
    """The stored inverse of a dense level: n columns of ld elements, element (i, j) at j * ld + i."""
    assert cinv.is_cuda and cinv.is_contiguous() and cinv.data_ptr() % 16 == 0, "cinv: a contiguous 16-byte aligned device tensor"
    assert ld >= n and ld % 4 == 0 and cinv.numel() == n * ld, f"cinv: {cinv.numel()} elements for n = {n}, ld = {ld}"


def mg_dense_apply(cinv: torch.Tensor, ld: int, scale: float, r: torch.Tensor, z: torch.Tensor) -> torch.Tensor:
    """z = scale * (cinv r) for the column-by-column inverse of a dense level, summed in segments of 64 columns (hipk_mg_dense_apply)."""
    n = z.numel()
    for v in (r, z):
        assert v.is_cuda and v.is_contiguous() and v.dtype == cinv.dtype and v.device == cinv.device and v.numel() == n
    _check_cinv(cinv, n, int(ld))
    with torch.cuda.device(z.device):
        _check(lib().hipk_mg_dense_apply(n, int(ld), cinv.data_ptr(), float(scale), r.data_ptr(), z.data_ptr(), _dtype_code(z.dtype),
                                         _stream(z.device)), "hipk_mg_dense_apply")
    return z


def mg_gtail_dense_apply(tail: MgGTail, omega: float, scale: float, r: torch.Tensor, z: torch.Tensor,
                         work: Optional[torch.Tensor] = None) -> torch.Tensor:
    """z = scale * V(0, r) over the tail's index-array levels and its dense last level in one launch (hipk_mg_gtail_dense_apply)."""
    assert tail.cinv is not None, "the tail was built without a dense level"
    return _mg_tail_call("hipk_mg_gtail_dense_apply", tail, omega, scale, r, z, work, tail.cinv.data_ptr(), tail.ld)


def mg_gtail_dense_apply_w(tail: MgGTail, omega: float, scale: float, r: torch.Tensor, z: torch.Tensor,
                           work: Optional[torch.Tensor] = None) -> torch.Tensor:
    """z = scale * W(0, r) over a tail built with cycle="W" and a dense last level, in one launch (hipk_mg_gtail_dense_apply_w)."""
    assert tail.cinv is not None, "the tail was built without a dense level"
    return _mg_tail_call("hipk_mg_gtail_dense_apply_w", tail, omega, scale, r, z, work, tail.cinv.data_ptr(), tail.ld)


def mg_level_scan_work_bytes(n: int) -> int:
    """The workspace of `mg_level_scan` for a level of n rows (hipk_mg_level_scan_work_bytes; 0 for n out of range)."""
    return int(lib().hipk_mg_level_scan_work_bytes(int(n)))


def mg_level_scan(crow: torch.Tensor, col: torch.Tensor, val: torch.Tensor, want_lmax: bool, dinv: torch.Tensor, out: torch.Tensor,
                  work: torch.Tensor) -> torch.Tensor:
    """One level of a hierarchy's refresh (hipk_mg_level_scan), on the current stream without synchronisation: from int32 `crow` /
    `col` and `val`, dinv[i] = 1 / (the stored diagonal of row i summed in stored order), out[0] = max_i sum_j |a_ij| / d_i in
    fp64 (0 when `want_lmax` is False) and out[1] = the number of rows with d_i <= 0.  `out`: two fp64 device elements, `work`: at
    least `mg_level_scan_work_bytes(n)` bytes; both 16-byte aligned."""
    n = dinv.numel()
    assert val.is_cuda and val.is_contiguous() and dinv.is_contiguous() and dinv.dtype == val.dtype and dinv.device == val.device
    assert out.is_contiguous() and out.dtype == torch.float64 and out.numel() == 2 and out.device == val.device
    assert work.is_contiguous() and work.dtype == torch.uint8 and work.device == val.device
    _check_index("crow", crow, n + 1, val)
    _check_index("col", col, val.numel(), val)
    with torch.cuda.device(val.device):
        _check(lib().hipk_mg_level_scan(n, crow.data_ptr(), col.data_ptr(), val.data_ptr(), _dtype_code(val.dtype), 1 if want_lmax else 0,
                                        dinv.data_ptr(), out.data_ptr(), work.data_ptr(), work.numel(), _stream(val.device)),
               "hipk_mg_level_scan")
    return out


# -------------------------------------------------------------------- whole solves
# Systems whose vectors live in HBM (a vector beyond the 256 MiB Infinity Cache): the CG vector kernels run at one of two discrete
# speeds depending on where r, p and x landed PHYSICALLY -- vectors in separate allocations were at the slow level every time,
# vectors in ONE allocation at the fast one in about half of the draws (profiles/r02_axpy_realloc_64m.txt).  So x joins the work
# buffer's allocation, a probe with the direction step's memory shape (hipk_placement_probe, ~0.5 ms per pass at N = 64 M) reads the
# level, and a slow draw is replaced by a fresh allocation (the earlier ones are held until the choice is made, so that the
# allocator has to map new pages), at most HIPK_PLACEMENT_TRIES (4) in all; the best one is kept.  HIPK_PLACEMENT_PROBE=0: off.
_PLACEMENT_MIN_VECTOR_BYTES = 256 << 20
_PLACEMENT_FAST_GBPS = 5400.0   # between the two levels (5.85 and 4.9 TB/s on the 40 n bytes of a pass)


def _placed_cg_work(h, x: torch.Tensor, work_bytes: int):
    """(buffer, work view, x view, probe GB/s, tries) for a large CG solve, or None when the system is small / probing is off."""
    item = x.element_size()
    n = x.numel()
    if n * item <= _PLACEMENT_MIN_VECTOR_BYTES or os.environ.get("HIPK_PLACEMENT_PROBE", "1") == "0" or hasattr(h, "regions"):
        return None
    L = lib()
    vec = (n * item + 255) // 256 * 256
    tries = max(1, int(os.environ.get("HIPK_PLACEMENT_TRIES", "4")))
    r_off = 256 + int(L.hipk_scratch_bytes())          # hipk_cg_solve's layout: header, partials, r, p, Ap (csrc/hipk_cg.hip)
    held, best = [], None
    us = ctypes.c_double()
    for t in range(tries):
        buf = torch.empty(work_bytes + vec, dtype=torch.uint8, device=x.device)
        held.append(buf)
        xin = buf[work_bytes:work_bytes + n * item].view(x.dtype)
        xin.copy_(x)
        _check(L.hipk_placement_probe(n, buf.data_ptr() + r_off, buf.data_ptr() + r_off + vec, xin.data_ptr(), _dtype_code(x.dtype),
                                      3, ctypes.byref(us), _stream(x.device)), "hipk_placement_probe")
        rate = 5 * n * item / us.value / 1e3
        if best is None or rate > best[3]:
            best = (buf, buf[:work_bytes], xin, rate, t + 1)
        if rate >= _PLACEMENT_FAST_GBPS:
            break
    return best[0], best[1], best[2], best[3], len(held)


def _workspace(work: Optional[torch.Tensor], device, nbytes: int, align: int = 256) -> torch.Tensor:
    """The workspace of a call: a fresh allocation, or the caller's `work` after checking it (contiguous uint8 on `device`,
    `align`-byte aligned, at least the library's `nbytes`).  The call is given `nbytes`, not work.numel()."""
    if work is None:
        return torch.empty(nbytes, dtype=torch.uint8, device=device)
    if not isinstance(work, torch.Tensor) or work.dtype != torch.uint8 or not work.is_contiguous() or work.dim() != 1:
        raise HipkError("work must be a contiguous one-dimensional uint8 tensor")
    if work.device != torch.device(device):
        raise HipkError(f"work is on {work.device}, the handle on {device}")
    if work.data_ptr() % align:
        raise HipkError(f"work must be {align}-byte aligned")
    if work.numel() < nbytes:
        raise HipkError(f"work holds {work.numel()} bytes, the call needs {nbytes}")
    return work


def _solve(method: str, h: CsrHandle, b: torch.Tensor, x: torch.Tensor, prm: Params, work_bytes: int,
           work: Optional[torch.Tensor] = None) -> SolveStats:
    L = lib()
    placed = None
    with torch.cuda.device(h.device):
        if method == "cg" and work is None:   # a caller's workspace stays where it is: no placement probe
            placed = _placed_cg_work(h, x, work_bytes)
    if placed is not None:
        _buf, work, x_run, probe_gbps, probe_tries = placed
    else:
        work, x_run, probe_gbps, probe_tries = _workspace(work, h.device, work_bytes), x, 0.0, 0
    if hasattr(h, "regions"):   # OpHandle: the operator callback resolves raw pointers against these tensors
        h.regions.append(work)
    st = Stats()
    fn = getattr(L, f"hipk_{method}_solve")
    with h._lock, torch.cuda.device(h.device):
        rc = fn(h.ptr, b.data_ptr(), x_run.data_ptr(), work.data_ptr(), work_bytes, ctypes.byref(prm), ctypes.byref(st),
                _stream(h.device))
    _check(rc, f"hipk_{method}_solve")
    if x_run is not x:
        x.copy_(x_run)
    return SolveStats(placement_GBps=probe_gbps, placement_tries=probe_tries, method=method, iterations=st.iterations, matvecs=st.matvecs, info=st.info,
                      breakdown=st.breakdown, b_norm=st.b_norm, residual_norm=st.residual_norm, x_norm=st.x_norm,
                      threshold=st.threshold, recurrence_rs=st.recurrence_rs, solve_ms=st.solve_ms,
                      spmv_ms_avg=st.spmv_ms_avg, spmv_profiled=st.spmv_profiled,
                      dispatch_span_ms_avg=st.dispatch_span_ms_avg)


def solve(method: str, h: CsrHandle, b: torch.Tensor, x: torch.Tensor, *, tol: float, atol: float,
          maxiter: Optional[int], restart: int = 20, solve_method: str = "batched", check_every: int = 0,
          profile: bool = False, work: Optional[torch.Tensor] = None) -> SolveStats:
    """Run hipk_{cg,bicgstab,gmres}_solve. `x` holds x0 on entry and the solution on return.  `work`: None (allocated here) or
    the caller's workspace, a contiguous uint8 tensor on the handle's device, 256-byte aligned, of at least the library's
    *_work_bytes; the solve is given the library's figure, and the placement probe of large CG systems is skipped."""
    if h.shape[0] != h.shape[1]:
        raise ValueError(f"linear operator must be a square matrix, but has shape: {h.shape}")
    assert b.is_contiguous() and x.is_contiguous() and b.dtype == h.dtype and x.dtype == h.dtype
    assert b.numel() == h.n and x.numel() == h.n and b.device == h.device and x.device == h.device
    prm = Params()
    prm.tol, prm.atol = float(tol), float(atol)
    prm.maxiter = -1 if maxiter is None else int(maxiter)
    prm.restart = int(restart)
    prm.gmres_method = {"batched": GMRES_BATCHED, "incremental": GMRES_INCREMENTAL}[solve_method]
    prm.check_every = int(check_every)
    prm.gpu_tolerances = 1  # device.type == 'cuda' on ROCm as well (TSL:737)
    prm.profile = int(profile)   # True/1: SpMV launches; CG only: 2 update kernel, 3 direction kernel
    L = lib()
    code = _dtype_code(h.dtype)
    if method == "gmres":
        wb = L.hipk_gmres_work_bytes(h.n, int(restart), code)
    else:
        wb = getattr(L, f"hipk_{method}_work_bytes")(h.n, code)
    return _solve(method, h, b, x, prm, int(wb), work)


def solve_pcg(h: CsrHandle, dinv: torch.Tensor, b: torch.Tensor, x: torch.Tensor, *, tol: float, atol: float,
              maxiter: Optional[int], check_every: int = 0, method: str = "cg",
              work: Optional[torch.Tensor] = None) -> SolveStats:
    """hipk_pcg_solve / hipk_pbicgstab_solve (method "cg" / "bicgstab") with M = diag(dinv).
    `x` holds x0 on entry and the solution on return.  `work`: as in `solve`."""
    if h.shape[0] != h.shape[1]:
        raise ValueError(f"linear operator must be a square matrix, but has shape: {h.shape}")
    for t in (dinv, b, x):
        assert t.is_contiguous() and t.dtype == h.dtype and t.numel() == h.n and t.device == h.device
    prm = Params()
    prm.tol, prm.atol = float(tol), float(atol)
    prm.maxiter = -1 if maxiter is None else int(maxiter)
    prm.check_every = int(check_every)
    prm.gpu_tolerances = 1
    L = lib()
    name = {"cg": "pcg", "bicgstab": "pbicgstab"}[method]
    wb = int(getattr(L, f"hipk_{name}_work_bytes")(h.n, _dtype_code(h.dtype)))
    work = _workspace(work, h.device, wb)
    if hasattr(h, "regions"):   # OpHandle: the operator callback resolves raw pointers against these tensors
        h.regions.append(work)
    st = Stats()
    with h._lock, torch.cuda.device(h.device):
        rc = getattr(L, f"hipk_{name}_solve")(h.ptr, dinv.data_ptr(), b.data_ptr(), x.data_ptr(), work.data_ptr(), wb,
                                              ctypes.byref(prm), ctypes.byref(st), _stream(h.device))
    _check(rc, f"hipk_{name}_solve")
    return SolveStats(method=f"{name}_jacobi", iterations=st.iterations, matvecs=st.matvecs, info=st.info,
                      breakdown=st.breakdown, b_norm=st.b_norm, residual_norm=st.residual_norm, x_norm=st.x_norm,
                      threshold=st.threshold, recurrence_rs=st.recurrence_rs, solve_ms=st.solve_ms,
                      spmv_ms_avg=st.spmv_ms_avg, spmv_profiled=st.spmv_profiled,
                      dispatch_span_ms_avg=st.dispatch_span_ms_avg)


@dataclass
class MultiSolveStats:
    """Side channel of cg_multi / bicgstab_multi: one SolveStats per column, the block-SpMV launches that did work (summed over
    the blocks of at most 16 columns; 0 when the columns ran one by one) and the solve time."""
    method: str
    columns: list
    block_spmvs: int
    solve_ms: float


MULTI_MAX_BLOCK = 16   # columns per block of hipk_{cg,bicgstab}_solve_multi


def multi_work_bytes(n: int, k: int, dtype: torch.dtype, method: str, precond: bool) -> int:
    return int(lib().hipk_multi_work_bytes(int(n), int(k), _dtype_code(dtype), 0 if method == "cg" else 1, 1 if precond else 0))


def solve_multi(method: str, h: CsrHandle, dinv: Optional[torch.Tensor], B: torch.Tensor, X: torch.Tensor, *, tol: float,
                atol: float, maxiter: Optional[int], check_every: int = 0, work: Optional[torch.Tensor] = None) -> MultiSolveStats:
    """hipk_{cg,bicgstab}_solve_multi: B, X row-major (n, k) of the handle's dtype; X holds X0 on entry and the solution on return.
    dinv: None (M = identity) or the Jacobi vector.  `work`: as in `solve`, of at least hipk_multi_work_bytes."""
    if h.shape[0] != h.shape[1]:
        raise ValueError(f"linear operator must be a square matrix, but has shape: {h.shape}")
    n, k = int(B.shape[0]), int(B.shape[1])
    for t in (B, X):
        assert t.is_contiguous() and t.dtype == h.dtype and t.shape == (h.n, k) and t.device == h.device
    if dinv is not None:
        assert dinv.is_contiguous() and dinv.dtype == h.dtype and dinv.numel() == h.n and dinv.device == h.device
    prm = Params()
    prm.tol, prm.atol = float(tol), float(atol)
    prm.maxiter = -1 if maxiter is None else int(maxiter)
    prm.check_every = int(check_every)
    prm.gpu_tolerances = 1
    L = lib()
    wb = multi_work_bytes(n, k, h.dtype, method, dinv is not None)
    work = _workspace(work, h.device, wb)
    st = (Stats * k)()
    spmvs = ctypes.c_int64(0)
    with h._lock, torch.cuda.device(h.device):
        rc = getattr(L, f"hipk_{method}_solve_multi")(h.ptr, None if dinv is None else dinv.data_ptr(), k, B.data_ptr(), k,
                                                      X.data_ptr(), k, work.data_ptr(), wb, ctypes.byref(prm), st,
                                                      ctypes.byref(spmvs), _stream(h.device))
    _check(rc, f"hipk_{method}_solve_multi")
    name = method if dinv is None else {"cg": "pcg_jacobi", "bicgstab": "pbicgstab_jacobi"}[method]
    cols = [SolveStats(method=name, iterations=c.iterations, matvecs=c.matvecs, info=c.info, breakdown=c.breakdown,
                       b_norm=c.b_norm, residual_norm=c.residual_norm, x_norm=c.x_norm, threshold=c.threshold,
                       recurrence_rs=c.recurrence_rs, solve_ms=c.solve_ms, spmv_ms_avg=0.0, spmv_profiled=0) for c in st]
    ms = sum(st[j].solve_ms for j in range(0, k, MULTI_MAX_BLOCK))
    return MultiSolveStats(method=f"{method}_multi", columns=cols, block_spmvs=int(spmvs.value), solve_ms=ms)


@dataclass
class BatchSolveStats:
    """Side channel of cg_batch / bicgstab_batch / gmres_batch: per-system lists (one entry per system), the path that ran
    (`hipk_last_solve_path` of the batch kernel, or "loop"), the kernel launches the solve took (0 on the loop route) and its time."""
    method: str
    iterations: list
    matvecs: list
    info: list
    breakdown: list
    b_norm: list
    residual_norm: list
    x_norm: list
    threshold: list
    recurrence_rs: list
    path: str
    launches: int
    solve_ms: float


BATCH_MAX_N = 4096      # the envelope of hipk_{cg,bicgstab,gmres}_solve_batch: rows per system ...
BATCH_MAX_ROW = 32      # ... and stored entries per row
GMRES_BATCH_MAX_RESTART = 31   # ... and, for hipk_gmres_solve_batch, the restart (HIPK_GM_MAXM)


def batch_work_bytes(n: int, nnz: int, batch: int, dtype: torch.dtype, method: str, precond: bool) -> int:
    """hipk_batch_work_bytes (pure host code: callable without a GPU)."""
    return int(lib().hipk_batch_work_bytes(int(n), int(nnz), int(batch), _dtype_code(dtype), 0 if method == "cg" else 1,
                                           1 if precond else 0))


def gmres_batch_work_bytes(n: int, nnz: int, batch: int, dtype: torch.dtype, restart: int, precond: bool) -> int:
    """hipk_gmres_batch_work_bytes (pure host code: callable without a GPU); 0 for a restart outside 1 .. 31."""
    return int(lib().hipk_gmres_batch_work_bytes(int(n), int(nnz), int(batch), _dtype_code(dtype), int(restart), 1 if precond else 0))


def solve_batch(method: str, n: int, nnz: int, crow: torch.Tensor, col: torch.Tensor, vals: torch.Tensor, dinv: Optional[torch.Tensor],
                B: torch.Tensor, X: torch.Tensor, *, tol: float, atol: float, maxiter: Optional[int],
                work: Optional[torch.Tensor] = None, restart: int = 20, solve_method: str = "batched") -> BatchSolveStats:
    """hipk_{cg,bicgstab,gmres}_solve_batch (restart and solve_method: gmres only): crow (n + 1,), col (nnz,) int32; vals (S, ldv), B (S, ldb), X (S, ldx), dinv None or
    (S, ldd), row-major with unit inner stride, of one dtype on one device; X holds X0 on entry and the solutions on return."""
    S = int(B.shape[0])
    dev = B.device
    for t in (vals, B, X) + (() if dinv is None else (dinv,)):
        assert t.dim() == 2 and t.shape[0] == S and t.stride(1) == 1 and t.dtype == B.dtype and t.device == dev
    assert crow.dtype == torch.int32 and col.dtype == torch.int32 and crow.is_contiguous() and col.is_contiguous()
    assert crow.numel() == n + 1 and col.numel() == nnz and crow.device == dev and col.device == dev
    prm = Params()
    prm.tol, prm.atol = float(tol), float(atol)
    prm.maxiter = -1 if maxiter is None else int(maxiter)
    prm.gpu_tolerances = 1
    L = lib()
    if method == "gmres":
        prm.restart = int(restart)
        prm.gmres_method = {"batched": GMRES_BATCHED, "incremental": GMRES_INCREMENTAL}[solve_method]
        wb = gmres_batch_work_bytes(n, nnz, S, B.dtype, restart, dinv is not None)
    else:
        wb = batch_work_bytes(n, nnz, S, B.dtype, method, dinv is not None)
    work = _workspace(work, dev, wb)
    st = (Stats * S)()
    ld = lambda t: int(t.stride(0))
    with torch.cuda.device(dev):
        rc = getattr(L, f"hipk_{method}_solve_batch")(n, nnz, crow.data_ptr(), col.data_ptr(), vals.data_ptr(), ld(vals),
                                                      None if dinv is None else dinv.data_ptr(), 0 if dinv is None else ld(dinv), S,
                                                      B.data_ptr(), ld(B), X.data_ptr(), ld(X), _dtype_code(B.dtype), work.data_ptr(),
                                                      wb, ctypes.byref(prm), st, _stream(dev))
    _check(rc, f"hipk_{method}_solve_batch")
    name = method if dinv is None else {"cg": "pcg_jacobi", "bicgstab": "pbicgstab_jacobi", "gmres": "pgmres_jacobi"}[method]
    col_of = lambda f: [getattr(c, f) for c in st]
    return BatchSolveStats(method=f"{name}_batch", iterations=col_of("iterations"), matvecs=col_of("matvecs"), info=col_of("info"),
                           breakdown=col_of("breakdown"), b_norm=col_of("b_norm"), residual_norm=col_of("residual_norm"),
                           x_norm=col_of("x_norm"), threshold=col_of("threshold"), recurrence_rs=col_of("recurrence_rs"),
                           path=last_solve_path(), launches=int(L.hipk_last_batch_launches()), solve_ms=float(st[0].solve_ms))


def bj_batch_work_bytes(n: int, nnz: int, batch: int, dtype: torch.dtype, method: str, block_size: int) -> int:
    """hipk_bj_batch_work_bytes (pure host code: callable without a GPU)."""
    return int(lib().hipk_bj_batch_work_bytes(int(n), int(nnz), int(batch), _dtype_code(dtype), 0 if method == "cg" else 1,
                                              int(block_size)))


def solve_batch_bj(method: str, n: int, nnz: int, crow: torch.Tensor, col: torch.Tensor, vals: torch.Tensor, binv: torch.Tensor,
                   block_size: int, B: torch.Tensor, X: torch.Tensor, *, tol: float, atol: float, maxiter: Optional[int],
                   work: Optional[torch.Tensor] = None) -> BatchSolveStats:
    """hipk_{cg,bicgstab}_solve_batch_bj: the operands of `solve_batch`, and binv (S, ceil(n / bs), bs, bs) contiguous."""
    S = int(B.shape[0])
    dev = B.device
    bs = int(block_size)
    for t in (vals, B, X):
        assert t.dim() == 2 and t.shape[0] == S and t.stride(1) == 1 and t.dtype == B.dtype and t.device == dev
    assert tuple(binv.shape) == (S, (n + bs - 1) // bs, bs, bs) and binv.is_contiguous() and binv.dtype == B.dtype and binv.device == dev
    assert crow.dtype == torch.int32 and col.dtype == torch.int32 and crow.is_contiguous() and col.is_contiguous()
    assert crow.numel() == n + 1 and col.numel() == nnz and crow.device == dev and col.device == dev
    prm = Params()
    prm.tol, prm.atol = float(tol), float(atol)
    prm.maxiter = -1 if maxiter is None else int(maxiter)
    prm.gpu_tolerances = 1
    L = lib()
    wb = bj_batch_work_bytes(n, nnz, S, B.dtype, method, bs)
    work = _workspace(work, dev, wb)
    st = (Stats * S)()
    ld = lambda t: int(t.stride(0))
    with torch.cuda.device(dev):
        rc = getattr(L, f"hipk_{method}_solve_batch_bj")(n, nnz, crow.data_ptr(), col.data_ptr(), vals.data_ptr(), ld(vals),
                                                         binv.data_ptr(), ld(binv), bs, S, B.data_ptr(), ld(B), X.data_ptr(), ld(X),
                                                         _dtype_code(B.dtype), work.data_ptr(), wb, ctypes.byref(prm), st, _stream(dev))
    _check(rc, f"hipk_{method}_solve_batch_bj")
    name = {"cg": "pcg_blockjacobi", "bicgstab": "pbicgstab_blockjacobi"}[method]
    col_of = lambda f: [getattr(c, f) for c in st]
    return BatchSolveStats(method=f"{name}_batch", iterations=col_of("iterations"), matvecs=col_of("matvecs"), info=col_of("info"),
                           breakdown=col_of("breakdown"), b_norm=col_of("b_norm"), residual_norm=col_of("residual_norm"),
                           x_norm=col_of("x_norm"), threshold=col_of("threshold"), recurrence_rs=col_of("recurrence_rs"),
                           path=last_solve_path(), launches=int(L.hipk_last_batch_launches()), solve_ms=float(st[0].solve_ms))


def solve_pgmres(h: CsrHandle, dinv: torch.Tensor, b: torch.Tensor, x: torch.Tensor, *, tol: float, atol: float,
                 maxiter: Optional[int], restart: int = 20, solve_method: str = "batched",
                 work: Optional[torch.Tensor] = None) -> SolveStats:
    """hipk_pgmres_solve: GMRES with M = diag(dinv) applied after every A (left preconditioning).  `work`: as in `solve`."""
    if h.shape[0] != h.shape[1]:
        raise ValueError(f"linear operator must be a square matrix, but has shape: {h.shape}")
    for t in (dinv, b, x):
        assert t.is_contiguous() and t.dtype == h.dtype and t.numel() == h.n and t.device == h.device
    prm = Params()
    prm.tol, prm.atol = float(tol), float(atol)
    prm.maxiter = -1 if maxiter is None else int(maxiter)
    prm.restart = int(restart)
    prm.gmres_method = {"batched": GMRES_BATCHED, "incremental": GMRES_INCREMENTAL}[solve_method]
    prm.gpu_tolerances = 1
    L = lib()
    wb = int(L.hipk_gmres_work_bytes(h.n, int(restart), _dtype_code(h.dtype)))
    work = _workspace(work, h.device, wb)
    if hasattr(h, "regions"):   # OpHandle: the operator callback resolves raw pointers against these tensors
        h.regions.append(work)
    st = Stats()
    with h._lock, torch.cuda.device(h.device):
        rc = L.hipk_pgmres_solve(h.ptr, dinv.data_ptr(), b.data_ptr(), x.data_ptr(), work.data_ptr(), wb,
                                 ctypes.byref(prm), ctypes.byref(st), _stream(h.device))
    _check(rc, "hipk_pgmres_solve")
    return SolveStats(method="pgmres_jacobi", iterations=st.iterations, matvecs=st.matvecs, info=st.info,
                      breakdown=st.breakdown, b_norm=st.b_norm, residual_norm=st.residual_norm, x_norm=st.x_norm,
                      threshold=st.threshold, recurrence_rs=st.recurrence_rs, solve_ms=st.solve_ms,
                      spmv_ms_avg=st.spmv_ms_avg, spmv_profiled=st.spmv_profiled,
                      dispatch_span_ms_avg=st.dispatch_span_ms_avg)


def solve_cg_callable(h: CsrHandle, M, b: torch.Tensor, x: torch.Tensor, *, tol: float, atol: float,
                      maxiter: Optional[int]) -> SolveStats:
    """CG with a CALLABLE preconditioner on the fused kernels (`_cg_solve` with M, TSL:806-856):
    `solve_cg_stepwise` with the handle's SpMV.  With M = (r -> dinv * r) the result equals hipk_pcg_solve's
    bit for bit."""
    if h.shape[0] != h.shape[1]:
        raise ValueError(f"linear operator must be a square matrix, but has shape: {h.shape}")
    return solve_cg_stepwise(h, None, M, b, x, tol=tol, atol=atol, maxiter=maxiter)


def solve_cg_stepwise(h: Optional[CsrHandle], A_fn, M, b: torch.Tensor, x: torch.Tensor, *, tol: float, atol: float,
                      maxiter: Optional[int]) -> SolveStats:
    """CG driven from the host through the step API, for operands the device-resident loop cannot call itself:
    a CALLABLE preconditioner `M` (h given) and/or a MATRIX-FREE operator `A_fn` (h None) -- `_cg_solve`, TSL:806-856.

    Per iteration: Ap = A p with <p,Ap> (fused into hipk_spmv_ex, or A_fn + hipk_dot_parts) | hipk_cg_update (r, <r,r>) |
    [z = M(r), <r,z>] | hipk_cg_direction / hipk_cgm_direction.  `A_fn` / `M` are the caller's own device code,
    enqueued on the current stream; scalars and the stop word live on the device, the host looks at the stop word
    every 8, 16, 32, 64, 64, ... iterations.  `x` holds x0 on entry and the solution on return."""
    assert (h is None) != (A_fn is None)
    assert b.is_contiguous() and x.is_contiguous() and b.is_cuda and x.dtype == b.dtype and x.shape == b.shape
    assert b.dtype in (torch.float64, torch.float32)
    if h is not None:
        assert b.dtype == h.dtype and b.numel() == h.n and b.device == h.device
    L = lib()
    n, dev, dt = b.numel(), b.device, _dtype_code(b.dtype)
    ch, G = int(L.hipk_chunk_size(n)), int(L.hipk_chunk_count(n))
    maxit = 10 * n if maxiter is None else int(maxiter)
    MODE_DOT_W, MODE_DOT_YY, MODE_RESID = 1, 2, 4

    def apply(fn, v, what):
        z = fn(v)
        if not isinstance(z, torch.Tensor) or z.shape != v.shape:
            raise ValueError(f"the {what} must map a vector to a vector of the same shape")
        return aligned(z.to(device=dev, dtype=b.dtype))

    import contextlib
    with (h._lock if h is not None else contextlib.nullcontext()), torch.cuda.device(dev):
        s = _stream(dev)
        r, p, Ap = torch.empty_like(b), torch.empty_like(b), torch.empty_like(b)
        parts = torch.zeros(6 * 2048, dtype=torch.float64, device=dev)
        part_pAp, part_rr, part_rz, part_bb, spare, part_xx = (parts[i * 2048:(i + 1) * 2048] for i in range(6))
        scal = torch.zeros(int(L.hipk_cg_scal_bytes()) // 8, dtype=torch.float64, device=dev)
        stop_word = scal[6:7].view(torch.int64)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()

        def dot_parts(u, v, part):
            _check(L.hipk_dot_parts(n, ch, u.data_ptr(), v.data_ptr(), dt, part.data_ptr(), s), "hipk_dot_parts")

        def residual(out, part_yy):                                  # out = b - A x  (+ <out,out> partials)
            if h is not None:
                _check(L.hipk_spmv_ex(h.ptr, x.data_ptr(), out.data_ptr(), MODE_RESID | MODE_DOT_YY, None, b.data_ptr(),
                                      spare.data_ptr(), part_yy.data_ptr(), None, 0, s), "hipk_spmv_ex")
            else:
                torch.sub(b, apply(A_fn, x, "operator"), out=out)
                dot_parts(out, out, part_yy)

        # r0 = b - A x0, <r0,r0>; <b,b>; [z0 = M r0, <r0,z0>]; p0 = z0 (or r0)   (TSL:815-826)
        residual(r, part_rr)
        dot_parts(b, b, part_bb)
        if M is not None:
            z = apply(M, r, "preconditioner")
            dot_parts(r, z, part_rz)
            _check(L.hipk_cgm_start(n, ch, G, scal.data_ptr(), part_rz.data_ptr(), part_rr.data_ptr(), part_bb.data_ptr(),
                                    z.data_ptr(), p.data_ptr(), dt, float(tol), float(atol), maxit, s), "hipk_cgm_start")
        else:
            _check(L.hipk_cg_start(n, ch, G, scal.data_ptr(), part_rr.data_ptr(), part_bb.data_ptr(), r.data_ptr(),
                                   p.data_ptr(), dt, float(tol), float(atol), maxit, s), "hipk_cg_start")
        it, stop, batch = 0, 1 << 62, 8
        while it < maxit:
            stop = int(stop_word.item())                      # one synchronisation per batch
            if stop <= it:
                break
            end = min(maxit, it + batch)
            batch = min(64, 2 * batch)
            while it < end:
                if h is not None:
                    _check(L.hipk_spmv_ex(h.ptr, p.data_ptr(), Ap.data_ptr(), MODE_DOT_W, p.data_ptr(), None,
                                          part_pAp.data_ptr(), spare.data_ptr(), stop_word.data_ptr(), it, s),
                           "hipk_spmv_ex")
                else:
                    Ap = apply(A_fn, p, "operator")
                    dot_parts(p, Ap, part_pAp)
                _check(L.hipk_cg_update(n, ch, G, scal.data_ptr(), it, part_pAp.data_ptr(), Ap.data_ptr(), r.data_ptr(),
                                        part_rr.data_ptr(), dt, s), "hipk_cg_update")
                if M is not None:
                    z = apply(M, r, "preconditioner")          # past the stop this works on a converged r: harmless
                    dot_parts(r, z, part_rz)
                    _check(L.hipk_cgm_direction(n, ch, G, scal.data_ptr(), it, maxit, part_pAp.data_ptr(),
                                                part_rz.data_ptr(), part_rr.data_ptr(), z.data_ptr(), p.data_ptr(),
                                                x.data_ptr(), dt, s), "hipk_cgm_direction")
                else:
                    _check(L.hipk_cg_direction(n, ch, G, scal.data_ptr(), it, maxit, part_pAp.data_ptr(),
                                               part_rr.data_ptr(), r.data_ptr(), p.data_ptr(), x.data_ptr(), dt, s),
                           "hipk_cg_direction")
                it += 1
        stop = int(stop_word.item())
        iterations = min(stop, it)
        # recurrence <r,r> of the last completed iteration, before the partial slots are reused
        out = torch.empty(4, dtype=torch.float64, device=dev)
        _check(L.hipk_reduce_parts(part_rr.data_ptr(), G, out[3:4].data_ptr(), s), "hipk_reduce_parts")
        # TSL:1007-1014: ||M (b - A x)||, ||x||
        res = torch.empty_like(b)
        residual(res, part_rz)
        if M is not None:
            zr = apply(M, res, "preconditioner")
            dot_parts(zr, zr, part_rz)
        dot_parts(x, x, part_xx)
        for k, prt in enumerate((part_rz, part_xx, part_bb)):
            _check(L.hipk_reduce_parts(prt.data_ptr(), G, out[k:k + 1].data_ptr(), s), "hipk_reduce_parts")
        e1.record()
        res2, xx, bs, rs = (float(v) for v in out.cpu())
    # math.sqrt, not ** 0.5: pow(v, 0.5) is off by one ulp from the correctly rounded root for about one value in a thousand, and
    # the C loops, the batch kernels and the oracle all take sqrt
    b_norm, res_norm = math.sqrt(max(bs, 0.0)), math.sqrt(max(res2, 0.0))
    x_norm = math.sqrt(max(xx, 0.0)) if xx == xx else float("nan")
    thr = max(float(torch.tensor(tol, dtype=torch.float32)) * b_norm, float(torch.tensor(atol, dtype=torch.float32)))
    info = -1 if (x_norm != x_norm or res_norm > thr) else 0
    method = ("cg_callable_M" if M is not None else "cg") if h is not None else \
             ("cg_matrix_free_callable_M" if M is not None else "cg_matrix_free")
    return SolveStats(method=method, iterations=iterations, matvecs=iterations + 2, info=info, breakdown=0,
                      b_norm=b_norm, residual_norm=res_norm, x_norm=x_norm, threshold=thr, recurrence_rs=rs,
                      solve_ms=e0.elapsed_time(e1), spmv_ms_avg=0.0, spmv_profiled=0)


class OpHandle:
    """hipk_op_create: a handle WITHOUT a matrix -- every product of a solve is the caller's `fn(v) -> A v` (device code on
    the current stream), followed by the library's epilogue kernel (residual form, fused dots).  It quacks like a CsrHandle
    for `solve` / `solve_pcg` / `_solve_with_callback` (ptr, n, shape, dtype, device, _lock).  The C loop hands raw device
    pointers to the callback; they are resolved against the tensors registered in `regions` (the solve's workspace, b, x)."""

    def __init__(self, fn, n: int, dtype: torch.dtype, device):
        self.fn, self.n, self.shape, self.dtype, self.device = fn, int(n), (int(n), int(n)), dtype, torch.device(device)
        self.regions = []
        self.errors = []
        self.calls = 0
        self._lock = _SolveLock()
        self._nbytes = self.n * torch.empty(0, dtype=dtype).element_size()
        self._cb = OP_FN(self._call)      # keep the thunk alive as long as the handle
        self._h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _check(lib().hipk_op_create(ctypes.byref(self._h), self.n, _dtype_code(dtype), self._cb, None, _stream(self.device)),
                   "hipk_op_create")

    @property
    def ptr(self):
        return self._h

    def _view(self, ptr):
        ptr = int(ptr)
        for t in self.regions:
            off = ptr - t.data_ptr()
            if 0 <= off and off + self._nbytes <= t.numel() * t.element_size():
                flat = t.view(torch.uint8) if t.dtype != torch.uint8 else t
                return flat[off:off + self._nbytes].view(self.dtype)
        raise HipkError("operator callback: pointer outside the solve's workspace, b and x")

    def _call(self, _user, x_ptr, y_ptr):
        try:
            vin, vout = self._view(x_ptr), self._view(y_ptr)
            y = self.fn(vin)
            if not isinstance(y, torch.Tensor) or y.shape != vin.shape:
                raise ValueError("the operator must map a vector to a vector of the same shape")
            vout.copy_(y)
            self.calls += 1
            return 0
        except BaseException as e:  # never let an exception unwind through the C frames
            self.errors.append(e)
            return 1

    def close(self):
        if getattr(self, "_h", None):
            lib().hipk_csr_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def solve_matrix_free(kind: str, A_fn, b: torch.Tensor, x: torch.Tensor, *, tol: float, atol: float, maxiter: Optional[int],
                      restart: int = 20, solve_method: str = "batched", M=None, dinv: Optional[torch.Tensor] = None) -> SolveStats:
    """cg / bicgstab / gmres with a MATRIX-FREE operator (`_normalize_matvec` takes a callable for all three solvers,
    TSL:176-208) on the device-resident C loops: `A_fn` is called where the loops launch their SpMV (hipk_op_create), the fused
    vector kernels, the device stop word and the pacing are the matrix path's.  M: None, a callable (bicgstab / gmres: the
    *_solve_cb loops) or `dinv` for the Jacobi forms.  `x` holds x0 on entry and the solution on return."""
    assert b.is_cuda and b.is_contiguous() and x.is_contiguous() and x.dtype == b.dtype and x.shape == b.shape and b.ndim == 1
    h = OpHandle(A_fn, b.numel(), b.dtype, b.device)
    try:
        # what the callback's pointers may point into: b, x and the workspace (the solve functions register theirs)
        h.regions = [b, x]
        if dinv is not None:
            if kind == "gmres":
                st = solve_pgmres(h, dinv, b, x, tol=tol, atol=atol, maxiter=maxiter, restart=restart, solve_method=solve_method)
            else:
                st = solve_pcg(h, dinv, b, x, tol=tol, atol=atol, maxiter=maxiter, method=kind)
        elif M is not None:
            if kind == "cg":
                raise HipkError("solve_matrix_free: cg with a callable M runs on solve_cg_stepwise")
            st = _solve_with_callback(kind, h, M, b, x, tol=tol, atol=atol, maxiter=maxiter, restart=restart,
                                      solve_method=solve_method)
        else:
            st = solve(kind, h, b, x, tol=tol, atol=atol, maxiter=maxiter, restart=restart, solve_method=solve_method)
        if h.errors:
            torch.cuda.synchronize(b.device)
            raise h.errors[0]
        st.method = f"{kind}_matrix_free" + ("_jacobi" if dinv is not None else "_callable_M" if M is not None else "")
        return st
    except HipkError:
        if h.errors:
            torch.cuda.synchronize(b.device)
            raise h.errors[0]
        raise
    finally:
        torch.cuda.synchronize(b.device)   # nothing of the solve may still read the handle's scratch
        h.close()


def solve_bicgstab_callable(h: CsrHandle, M, b: torch.Tensor, x: torch.Tensor, *, tol: float, atol: float,
                            maxiter: Optional[int], check_every: int = 0, work: Optional[torch.Tensor] = None) -> SolveStats:
    """hipk_pbicgstab_solve_cb: the device-resident BiCGStab loop with a CALLABLE preconditioner (TSL:859-964 with M).
    `work`: as in `solve`; M is called on views of it."""
    return _solve_with_callback("bicgstab", h, M, b, x, tol=tol, atol=atol, maxiter=maxiter, check_every=check_every, work=work)


def solve_gmres_callable(h: CsrHandle, M, b: torch.Tensor, x: torch.Tensor, *, tol: float, atol: float,
                         maxiter: Optional[int], restart: int = 20, solve_method: str = "batched",
                         work: Optional[torch.Tensor] = None) -> SolveStats:
    """hipk_pgmres_solve_cb: GMRES with a CALLABLE preconditioner applied after every A (TSL:641-803 with M).
    `work`: as in `solve`; M is called on views of it."""
    return _solve_with_callback("gmres", h, M, b, x, tol=tol, atol=atol, maxiter=maxiter, restart=restart,
                                solve_method=solve_method, work=work)


def _solve_with_callback(kind: str, h: CsrHandle, M, b: torch.Tensor, x: torch.Tensor, *, tol: float, atol: float,
                         maxiter: Optional[int], check_every: int = 0, restart: int = 20,
                         solve_method: str = "batched", work: Optional[torch.Tensor] = None) -> SolveStats:
    """The C loop calls back here where the reference applies M -- BiCGStab: phat = M(p), shat = M(s), M(b - A x);
    GMRES: M(A v), M(b - A x), M b -- with pointers into the workspace; they are wrapped as views of the workspace
    tensor (no copy in), `M` runs on the current stream, its result is copied into the output slot.  No
    synchronisation inside the loop."""
    if h.shape[0] != h.shape[1]:
        raise ValueError(f"linear operator must be a square matrix, but has shape: {h.shape}")
    for t in (b, x):
        assert t.is_contiguous() and t.dtype == h.dtype and t.numel() == h.n and t.device == h.device
    L = lib()
    prm = Params()
    prm.tol, prm.atol = float(tol), float(atol)
    prm.maxiter = -1 if maxiter is None else int(maxiter)
    prm.check_every = int(check_every)
    prm.gpu_tolerances = 1
    if kind == "gmres":
        prm.restart = int(restart)
        prm.gmres_method = {"batched": GMRES_BATCHED, "incremental": GMRES_INCREMENTAL}[solve_method]
        wb = int(L.hipk_gmres_work_bytes(h.n, int(restart), _dtype_code(h.dtype)))
        fn = L.hipk_pgmres_solve_cb
    else:
        wb = int(L.hipk_pbicgstab_work_bytes(h.n, _dtype_code(h.dtype)))
        fn = L.hipk_pbicgstab_solve_cb
    work = _workspace(work, h.device, wb)
    if hasattr(h, "regions"):   # OpHandle: the operator callback resolves raw pointers against these tensors
        h.regions.append(work)
    base, nbytes = work.data_ptr(), h.n * work.new_empty(0, dtype=h.dtype).element_size()
    errors = []

    def view(ptr):
        off = int(ptr) - base
        if off < 0 or off + nbytes > wb:
            raise HipkError("preconditioner callback: pointer outside the workspace")
        return work[off:off + nbytes].view(h.dtype)

    def callback(_user, in_ptr, out_ptr):
        try:
            vin, vout = view(in_ptr), view(out_ptr)
            z = M(vin)
            if not isinstance(z, torch.Tensor) or z.shape != vin.shape:
                raise ValueError("the preconditioner must map a vector to a vector of the same shape")
            vout.copy_(z)
            return 0
        except BaseException as e:  # never let an exception unwind through the C frames
            errors.append(e)
            return 1
    cb = PRECOND_FN(callback)
    st = Stats()
    with h._lock, torch.cuda.device(h.device):
        rc = fn(h.ptr, cb, None, b.data_ptr(), x.data_ptr(), work.data_ptr(), wb, ctypes.byref(prm), ctypes.byref(st),
                _stream(h.device))
    if errors:
        torch.cuda.synchronize(h.device)
        raise errors[0]
    _check(rc, f"hipk_p{kind}_solve_cb")
    return SolveStats(method=f"{kind}_callable_M", iterations=st.iterations, matvecs=st.matvecs, info=st.info,
                      breakdown=st.breakdown, b_norm=st.b_norm, residual_norm=st.residual_norm, x_norm=st.x_norm,
                      threshold=st.threshold, recurrence_rs=st.recurrence_rs, solve_ms=st.solve_ms,
                      spmv_ms_avg=st.spmv_ms_avg, spmv_profiled=st.spmv_profiled,
                      dispatch_span_ms_avg=st.dispatch_span_ms_avg)
