/*
 * hipk.h -- C ABI of libhipk.so: MI355X (gfx950) kernels for the Module-A
 * iterative-solver hot path (CSR SpMV, deterministic dots, fused CG / BiCGStab /
 * GMRES updates, device-resident solve loops).
 *
 * The reference (Litianyu141/Pytorch-Sparse-Linalg-torch-amgx.cg.bicg.gmres) has
 * NO native boundary: its hot path is Python calling ATen.  Every entry point
 * below therefore names the reference Python construct it replaces
 * (TSL = src/pytorch_sparse_solver/module_a/torch_sparse_linalg.py).
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no torch types.
 *   - every pointer named *_dev / x / y / b / work is a DEVICE pointer
 *     (tensor.data_ptr()); vectors must be 16-byte aligned.
 *   - every function returns HIPK_OK (0) or a negative hipk_status;
 *     hipk_last_error() gives the thread-local message of the last failure.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).
 *   - the library never allocates inside a solve: the caller supplies `work`
 *     (size from hipk_*_work_bytes), so solves are graph/stream friendly.
 *   - a handle owns scratch its kernels write (per-tile sums of the fused dots):
 *     calls on ONE handle must be ordered on one stream (or by events);
 *     different handles are independent.
 *   - all reductions are atomic-free with a fixed summation tree
 *     (DESIGN.md "reduction spec"): results are bitwise run-to-run reproducible
 *     and bitwise equal to oracle/krylov_oracle.c.
 */
#ifndef HIPK_H
#define HIPK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HIPK_VERSION 300

typedef struct hipk_csr_s *hipk_csr_t;
typedef void *hipk_stream_t; /* hipStream_t */

enum hipk_dtype { HIPK_F32 = 0, HIPK_F64 = 1 };

enum hipk_status {
    HIPK_OK = 0,
    HIPK_ERR_ARG = -1,         /* bad argument (null pointer, negative size, ...) */
    HIPK_ERR_HIP = -2,         /* a HIP runtime call failed                       */
    HIPK_ERR_ALIGN = -3,       /* vector pointer not 16-byte aligned              */
    HIPK_ERR_UNSUPPORTED = -4, /* dtype / option not built                        */
    HIPK_ERR_WORKSPACE = -5,   /* work buffer too small                           */
    HIPK_ERR_NO_DEVICE = -6    /* no gfx950 device visible                        */
};

/* GMRES least-squares variants, TSL:755-760 (`solve_method`). */
enum hipk_gmres_method { HIPK_GMRES_BATCHED = 0, HIPK_GMRES_INCREMENTAL = 1 };

/* Solver parameters: the keyword arguments of cg/bicgstab/gmres
 * (TSL:1019-1021, 1091-1093, 641-644). */
typedef struct {
    double tol;            /* relative tolerance (python float, rounded through fp32 as the reference does) */
    double atol;           /* absolute tolerance                                                           */
    int64_t maxiter;       /* CG/BiCGStab: iterations; GMRES: restart cycles. <0 => 10*n (TSL:982-984)      */
    int32_t restart;       /* GMRES Krylov dimension (TSL:642)                                             */
    int32_t gmres_method;  /* hipk_gmres_method                                                            */
    int32_t check_every;   /* stream-ordered polling interval of the fallback pacing (<=0: default), see below */
    int32_t gpu_tolerances;/* 1: GMRES uses the `device.type=='cuda'` tolerance branch (TSL:737-740)       */
    int32_t profile;       /* 1: time every SpMV launch of the loop (start/stop events bound to the dispatch) and report
                              stats.spmv_ms_avg; CG only: 2 = the update kernel, 3 = the direction kernel (large systems:
                              its flat-grid launch), 4 = the scalars launch that precedes the flat-grid one           */
    int32_t reserved;
} hipk_params;

/* Side channel the reference does not have: filled on return. */
typedef struct {
    int64_t iterations;     /* CG/BiCGStab loop iterations; GMRES restart cycles                    */
    int64_t matvecs;        /* SpMV launches that did work                                          */
    int32_t info;           /* 0 converged / -1 not, decided exactly as TSL:1007-1016 / TSL:766-773 */
    int32_t breakdown;      /* BiCGStab: 0, -10 (rho), -11 (alpha/omega) as TSL:902-936; GMRES: 1 on happy breakdown */
    double b_norm;          /* ||b||                                                                */
    double residual_norm;   /* true ||b - A x|| recomputed after the loop                           */
    double x_norm;          /* ||x|| (NaN check)                                                    */
    double threshold;       /* the value residual_norm was compared against                         */
    double recurrence_rs;   /* last recurrence <r,r> (CG: gamma)                                    */
    double solve_ms;        /* device time of the whole solve, HIP events on `stream`               */
    double spmv_ms_avg;     /* average of stop - start over the launches params.profile selects (start/stop events bound to the
                               dispatch, hipExtLaunchKernel); RAW: nothing subtracted.  The start stamp is taken when the dispatch
                               is picked up, 0.6-1.5 us before its first wave when the previous kernel is still draining
                               (csrc/hipk_solve.h has the comparison with rocprofv3's averages). */
    int64_t spmv_profiled;  /* number of SpMV launches in that average                              */
    double dispatch_span_ms_avg; /* the same figure (in the diagnostic chain mode spmv_ms_avg is stop-to-stop instead; version 200:
                                    event_overhead_ms) */
} hipk_stats;

int hipk_version(void);
/* 16 hex digits: sha1 over the sources this library was compiled from (csrc/Makefile).  Counter profiles under profiles/ carry it;
 * bench.py quotes a `traffic` figure only when it was taken on the build that is running. */
const char *hipk_build_id(void);
const char *hipk_last_error(void);

/* Number of visible HIP devices whose arch is gfx950 (0 => nothing can run). */
int hipk_device_count(void);

/* ---- CSR handle --------------------------------------------------------------
 * Replaces the tensor `A` captured by `_normalize_matvec` (TSL:176-208).
 * crow/col are device arrays of idx_bytes (4 or 8) wide integers as torch stores
 * them (int64); they are narrowed once to int32 (SURVEY 7.2 "index width").
 * `val` is BORROWED: it must stay alive until hipk_csr_destroy, and unchanged unless
 * hipk_csr_update_values is called afterwards -- the one lawful way to change values.
 * A row is summed in STORED order: its products are rounded and added in the order
 * of its entries in col/val (rows of more than 32 entries: 64 lane-strided partial
 * sums of the stored sequence).  Column indices need not be sorted within a row, and
 * a column may be stored more than once (the entries add, as in A x) or with the
 * value 0: every SpMV kernel, solve form, the Chebyshev epilogue and the transpose
 * accept such rows, and the results are bitwise those of the oracle on the same
 * arrays (tests/test_gpu_entry_order.py).  The row-partitioned solves depend on
 * it: a rank's boundary rows arrive with renumbered, unsorted ghost columns. */
int hipk_csr_create(hipk_csr_t *out, int64_t n_rows, int64_t n_cols, int64_t nnz,
                    const void *crow_dev, const void *col_dev, int idx_bytes,
                    const void *val_dev, int dtype, hipk_stream_t stream);
int hipk_csr_destroy(hipk_csr_t h);
int64_t hipk_csr_rows(hipk_csr_t h);
int64_t hipk_csr_nnz(hipk_csr_t h);
/* Algorithmic bytes of one SpMV: nnz*(sizeof(val)+4)+(n+1)*4+2*n*sizeof(val). */
int64_t hipk_csr_spmv_bytes(hipk_csr_t h);

/* Which SpMV kernel family the structure analysis of hipk_csr_create selected.  All of them produce the same
 * bits (one summation spec, oracle/krylov_oracle.c).
 *   TILE_FAST : 256-row tiles, every tile fits the LDS product buffer and no row exceeds 32 entries
 *   TILE      : 256-row tiles with the general path (long rows, dense tiles, huge-row pre-pass)
 *   ROWWAVE   : row per wavefront (mean row length >= 48: dense-as-CSR, FEM blocks)
 *   CODED     : the matrix has at most 256 distinct (col - row, value) pairs and short rows (finite-difference /
 *               finite-volume stencils, e.g. matrix_utils.py:193-257 and ldc_solver_common.py:90-135): the handle
 *               keeps one byte per entry + one byte per row + the dictionary and streams those instead of
 *               col/val/crow.  The values are SNAPSHOTTED at creation and by hipk_csr_update_values.
 *   OFFSET_CODED : too many distinct values, but at most 255 distinct column OFFSETS and short rows (variable-coefficient
 *               stencils): one offset-code byte + the value per entry in coalesced planes, 9 instead of 12 bytes
 *               per entry and no row pointers.  Values snapshotted as for CODED. */
enum hipk_spmv_path { HIPK_PATH_TILE_FAST = 0, HIPK_PATH_TILE = 1, HIPK_PATH_ROWWAVE = 2, HIPK_PATH_CODED = 3,
                      HIPK_PATH_OFFSET_CODED = 4 };
int hipk_csr_spmv_path(hipk_csr_t h);
/* Name of the kernel instantiation the calling thread's most recent SpMV launch selected (stand-alone or inside a solver),
 * as the profiler prints it, e.g. "hipk_spmv_sell_wide_kernel<5,1>"; "" before the first launch.  Measurement scripts label
 * their per-kernel figures with it instead of guessing the dispatch. */
const char *hipk_last_spmv_kernel(void);
/* The loop that finished the calling thread's most recent hipk_{cg,pcg,bicgstab,pbicgstab,gmres,pgmres}_solve (also the _cb
 * forms): the one-launch instantiation of mid-size systems, e.g. "hipk_cg_mid_kernel<double,9,1,false>" or
 * "hipk_gm_mid_kernel<float,7,true>"; the whole-loop kernel of small systems, e.g. "hipk_cg_solve_lds_kernel"; or
 * "launch sequence" (kernels launched per iteration, also when the loop ran no iteration).  When a one-launch kernel handed
 * the solve back (its workgroups were not all resident), the chain shows it: "hipk_cg_mid_kernel<double,5,1,false> ->
 * launch sequence".  "" before the first solve. */
const char *hipk_last_solve_path(void);
/* The FORM that solve finished in: which variant of the path's kind, at the resolution of the dispatch.  A one-launch kernel
 * reports the instantiation of its last launch, e.g. "hipk_cg_solve_lds_kernel<double,true,false>" (T, LOCAL, PRE; LOCAL false
 * also after the kernel asked for agent-scope hand-offs), "hipk_gm_solve_lds_kernel<float,false>", "hipk_gm_cycle_small_kernel<double>"
 * or the mid kernel's name as the path gives it.  A launch sequence reports which one, e.g. "cg two-launch: hipk_cg2_spmv_kernel<double,1280>
 * + hipk_cg2_update_kernel", "cg three-launch, small", "bicgstab five-launch, Jacobi", "gmres restart > 31" (DESIGN.md 8b lists
 * them) -- also when the loop ran no iteration.  hipk_{cg,bicgstab}_solve_multi and hipk_dist_* report their path string.
 * hipk_solve_form_name(i), 0 <= i < hipk_solve_form_count(), enumerates every form of the single-device solvers (no GPU
 * needed); NULL outside that range. */
const char *hipk_last_solve_form(void);
/* The iterations of the calling thread's last hipk_cg_solve whose direction step (beta, p = r + beta p, the stop test) ran as the
 * tail of the fused SpMV + update launch (hipk_cg_fuse_update_kernel) instead of a launch of its own; 0 when none did.  The note,
 * path and form of such a solve are those of the fused sequence it is a variant of. */
int hipk_last_cg_fused_directions(void);
/* ... and those of them whose launch kept p of its uniform tiles in registers between the SpMV walk and the direction tail
 * instead of loading it again (0 with HIPK_CG_FUSE_KEEP_P=0). */
int hipk_last_cg_fused_kept_p(void);
int hipk_solve_form_count(void);
const char *hipk_solve_form_name(int i);
/* mode 0: automatic (default); 1: never use the coded forms (A/B measurements, parity tests).
 * Environment: HIPK_SPMV_CODED=0 at creation time skips building the coded forms altogether,
 * HIPK_SPMV_OFFSET_CODED=0 only the offset-coded one. */
int hipk_csr_set_path(hipk_csr_t h, int mode);
/* Bytes one SpMV has to move in the format the selected path streams (= hipk_csr_spmv_bytes unless CODED). */
int64_t hipk_csr_format_bytes(hipk_csr_t h);
/* New values on the same pattern.  After HIPK_OK the handle is the one hipk_csr_create_ex would have built from the same crow,
 * col, chunk_rows and `val_dev` under the same HIPK_* switches: the same hipk_csr_spmv_path, hipk_csr_format_bytes, coded layout
 * and uniform-tile decision, so every hipk_spmv_ex mode and every solve selects the same kernel and solve form and produces the
 * same bits as on a fresh handle (dictionary numbering may differ; no result depends on it).  Creation and update run ONE
 * decision function (hipk_decide_coded, csrc/hipk_api.hip).  `val_dev` (nnz values of the handle's dtype, 16-byte aligned) is
 * BORROWED from then on; it may be the pointer the handle already holds, after an in-place change.  Everything that follows from
 * crow / col alone is kept -- the int32 copies, the row / tile maxima, the huge-row list, the scratch, the tile widths and plane
 * offsets, the offset dictionary and code planes of the OFFSET_CODED form, the window plan of the one-launch loops,
 * hipk_csr_set_path's mode -- and what follows from the numbers is recomputed into the buffers the handle owns: the pair dictionary
 * attempt, the code bytes and uniform-tile words of the CODED form, the value planes of the OFFSET_CODED form (hipk_csr_revalue_*
 * kernels).  While the form stays the same nothing is allocated or freed; a form the handle leaves has its buffers freed.  The host
 * waits only for the dictionary verdicts: 0 for a matrix with a row of more than 32 entries, else 1 - 3.
 * Every transition between CODED, OFFSET_CODED and the plain kernels is allowed.
 * hipk_last_csr_update_kind(): of the calling thread's last successful update -- 1 values only (plain stayed plain, or OFFSET_CODED
 * stayed and its value planes were rewritten), 2 re-encoded in place (CODED stayed in its layout), 3 the form changed; 0 before
 * the first update.
 * A null val_dev: HIPK_ERR_ARG; a misaligned one: HIPK_ERR_ALIGN; a matrix-free handle (hipk_op_create): HIPK_ERR_UNSUPPORTED; each
 * leaves the handle exactly as it was.  A HIP error part-way leaves a valid handle on the plain kernels with the new values.
 * NOT safe against a solve or product running on the same handle: the caller serialises. */
int hipk_csr_update_values(hipk_csr_t h, const void *val_dev, hipk_stream_t stream);
int hipk_last_csr_update_kind(void);
/* Host synchronisations the calling thread's last successful update took (measurement: tools/handle_update_probe.py). */
int hipk_last_csr_update_syncs(void);
/* Measurement hook: one launch of the value-plane rewrite of an OFFSET_CODED handle from the values it holds, in the given
 * form -- 1: one row per lane from global memory, 2: the tile's CSR value range staged through LDS with 16-byte loads (the
 * library's choice where the range fits 64 KB).  Both write the same elements.  Another handle: HIPK_ERR_UNSUPPORTED. */
int hipk_csr_revalue_probe(hipk_csr_t h, int form, hipk_stream_t stream);

/* ---- transpose (adjoint solves) ------------------------------------------------
 * The implicit-diff backward of the reference solves with A^T (`ImplicitAdjointFunction.backward`, TSL:1237-1248; `A.T`,
 * TSL:1245).  hipk_csr_transpose writes the CSR arrays of A^T -- int32 row pointers [n_cols + 1], int32 columns [nnz]
 * sorted within each row, values [nnz] of the handle's dtype -- into caller-owned device buffers, from which a handle
 * for A^T is created with hipk_csr_create (idx_bytes 4).  Device-side stable sort by column; `work` >=
 * hipk_csr_transpose_work_bytes(h), 256-byte aligned.  Setup step, not on the per-iteration path. */
size_t hipk_csr_transpose_work_bytes(hipk_csr_t h);
int hipk_csr_transpose(hipk_csr_t h, int32_t *crow_t_dev, int32_t *col_t_dev, void *val_t_dev, void *work,
                       size_t work_bytes, hipk_stream_t stream);

/* ---- matrix gradient of a solve (csrc/hipk_vgrad.hip) -----------------------------
 * With x = A^-1 b, g = dL/dx and lam = A^-T g, the gradient of L with respect to the stored entry k of A, in row row(k) and
 * column col(k), is  G[k] = -(lam[row(k)] * x[col(k)]):  one multiplication in T, then a negation.  A column stored twice in a
 * row gives both entries the same value, a stored zero gets a gradient like any other entry, rows may have any length.
 *   hipk_batch_grad_values : G[s ldg + k] = -(L[s ldl + row(k)] * X[s ldx + col(k)]),  k < nnz, s < batch, for `batch` systems
 *                            of n rows with ONE pattern (int32 crow [n + 1] / col [nnz] on the device).  No n or row-length
 *                            envelope.
 *   hipk_csr_grad_values   : the same for one matrix through its handle (the handle's int32 index copies; rectangular handles:
 *                            lam has n_rows, x n_cols elements, gvals nnz).
 * One launch of hipk_csr_vgrad_kernel<T> either way; every element G[s ldg + k], k < nnz, is written exactly once and elements
 * of a row at and beyond nnz are never written.  Neither entry synchronises or reads crow on the host.  nnz == 0 or batch == 0:
 * HIPK_OK without a launch.  A null pointer, a negative size, n or nnz >= 2^31, an ld shorter than its row (ldl, ldx < n,
 * ldg < nnz) or g equal to lam or x: HIPK_ERR_ARG; a dtype other than HIPK_F32 / HIPK_F64: HIPK_ERR_UNSUPPORTED; a pointer that
 * is not 16-byte aligned or, with batch > 1, an ld * sizeof(T) that is no multiple of 16: HIPK_ERR_ALIGN.  A call that returns
 * an error has launched nothing.  hipk_last_grad_values_launches(): the launches the calling thread's last call of either
 * entry took (0 or 1). */
int hipk_batch_grad_values(int64_t n, int64_t nnz, const int32_t *crow_dev, const int32_t *col_dev, int batch,
                           const void *lam, int64_t ldl, const void *x, int64_t ldx, void *g, int64_t ldg,
                           int dtype, hipk_stream_t stream);
int hipk_csr_grad_values(hipk_csr_t h, const void *lam, const void *x, void *gvals, hipk_stream_t stream);
int hipk_last_grad_values_launches(void);

/* ---- reduction geometry ------------------------------------------------------
 * Every dot/norm is a two-level fixed tree: the vector is cut in `count` chunks
 * of `chunk` elements (chunk = 2048 * 2^k, count <= 2048); see DESIGN.md. */
int hipk_chunk_size(int64_t n);
int hipk_chunk_count(int64_t n);

/* ---- primitives --------------------------------------------------------------
 * scratch_dev: device buffer of hipk_scratch_bytes() bytes (partial sums).      */
size_t hipk_scratch_bytes(void);

/* y = A x  (torch.matmul(A, v), TSL:191). */
int hipk_spmv(hipk_csr_t h, const void *x, void *y, hipk_stream_t stream);
/* y = A x and out_dev[0] = <w, y>  (TSL:845-846 fused). */
int hipk_spmv_dot(hipk_csr_t h, const void *x, void *y, const void *w,
                  double *out_dev, void *scratch_dev, hipk_stream_t stream);
/* out_dev[0] = <x, y>  (`_vdot_real_tree`, TSL:130-139). Accumulates in fp64. */
int hipk_dot(int64_t n, const void *x, const void *y, int dtype, double *out_dev,
             void *scratch_dev, hipk_stream_t stream);
/* y = a*x + y with mul-then-add rounding (`_add(y, _mul(a, x))`, TSL:847). */
int hipk_axpy(int64_t n, double a, const void *x, void *y, int dtype, hipk_stream_t stream);
/* y = x + b*y  (`_add(z, _mul(beta, p))`, TSL:852). */
int hipk_xpby(int64_t n, const void *x, double b, void *y, int dtype, hipk_stream_t stream);

/* ---- whole solves (device-resident loops) ------------------------------------
 * x: in = x0, out = solution.  b is not modified.  `work` >= *_work_bytes.
 * The workspace contract (every entry point that takes `work`; tests/_arena.py):
 *   - `work` need not be initialised: the result does not depend on what it
 *     holds on entry, and what it holds after a call is unspecified;
 *   - a call writes no byte outside [work, work + work_bytes) -- work_bytes the
 *     figure of *_work_bytes, whatever larger size is passed --, x[0..n) and
 *     the handle's own scratch; dinv and the matrix are read-only like b;
 *   - one workspace may be reused, without clearing it, across solvers, sizes
 *     and handles, by calls ordered on one stream.
 * The loop stops at exactly the iteration the reference stops at (device-side
 * stop word: launches past it are no-ops).  The host follows the loop through a
 * pinned word the deciding kernel stores to and keeps a few iterations queued
 * ahead; HIPK_HOST_SIGNAL=0 (or a word that stops moving) selects stream-ordered
 * reads of the stop word every check_every iterations instead.
 * A handle owns scratch that its solves and fused-dot products share (per-tile
 * partial sums, the pinned signal words): run ONE whole solve / hipk_spmv_ex
 * with dot modes per handle at a time; plain hipk_spmv calls may overlap.      */
size_t hipk_cg_work_bytes(int64_t n, int dtype);
/* `_isolve(_cg_solve)`: TSL:806-856 + 968-1016. */
int hipk_cg_solve(hipk_csr_t A, const void *b, void *x, void *work, size_t work_bytes,
                  const hipk_params *prm, hipk_stats *st, hipk_stream_t stream);

size_t hipk_bicgstab_work_bytes(int64_t n, int dtype);
/* `_isolve(_bicgstab_solve)`: TSL:859-964 + 968-1016. */
int hipk_bicgstab_solve(hipk_csr_t A, const void *b, void *x, void *work, size_t work_bytes,
                        const hipk_params *prm, hipk_stats *st, hipk_stream_t stream);

size_t hipk_gmres_work_bytes(int64_t n, int restart, int dtype);
/* `gmres`: TSL:641-803 with `_gmres_batched` (TSL:431-493) or
 * `_gmres_incremental` (TSL:557-638). */
int hipk_gmres_solve(hipk_csr_t A, const void *b, void *x, void *work, size_t work_bytes,
                     const hipk_params *prm, hipk_stats *st, hipk_stream_t stream);

/* ---- CG with a Jacobi preconditioner ---------------------------------
 * `cg(A, b, M=...)` of the reference (TSL:1019-1021) with M(v) = dinv .* v, the iteration of TSL:806-856 for a
 * non-identity M: gamma = <r, M r>, stop test on <r,r>, `info` from ||M (b - A x)|| (TSL:1007).  `dinv` is a
 * device vector of the matrix' dtype (the reciprocal diagonal); the scaling is fused into the update and direction
 * kernels.  Same params / stats / work-buffer conventions as hipk_cg_solve. */
size_t hipk_pcg_work_bytes(int64_t n, int dtype);
int hipk_pcg_solve(hipk_csr_t A, const void *dinv, const void *b, void *x, void *work, size_t work_bytes,
                   const hipk_params *prm, hipk_stats *st, hipk_stream_t stream);
/* GMRES with the same M (left preconditioning: the reference applies M after every A, TSL:351, 791, 766; ptol from
 * ||M b||, TSL:750).  The row scaling runs in the SpMV epilogue.  Work buffer: hipk_gmres_work_bytes. */
int hipk_pgmres_solve(hipk_csr_t A, const void *dinv, const void *b, void *x, void *work, size_t work_bytes,
                      const hipk_params *prm, hipk_stats *st, hipk_stream_t stream);
/* BiCGStab with the same M, applied BEFORE A as the reference does (phat = M p, shat = M s, TSL:908, 922; x advances
 * with phat / shat, TSL:942; `info` from ||M (b - A x)||): phat and shat are two more work vectors. */
size_t hipk_pbicgstab_work_bytes(int64_t n, int dtype);
int hipk_pbicgstab_solve(hipk_csr_t A, const void *dinv, const void *b, void *x, void *work, size_t work_bytes,
                         const hipk_params *prm, hipk_stats *st, hipk_stream_t stream);
/* ---- many right-hand sides: k systems on one matrix, the matrix read once per block iteration ------------------------
 * Column j of the result is bit for bit hipk_cg_solve / hipk_pcg_solve (solver 0) or hipk_bicgstab_solve / hipk_pbicgstab_solve
 * (solver 1) of column j: the same params, the same per-column stats (st: k entries, iterations, matvecs, info, breakdown,
 * norms), each column stopping at its own iteration.  B (n x k, leading dimension ldb >= k) and X (n x k, ldx >= k; x0 in,
 * x out) are row-major device arrays of the matrix' dtype; dinv is NULL (M = identity) or the Jacobi vector.  Columns run in
 * blocks of at most 16 with all per-column scratch in `work` (hipk_multi_work_bytes(n, k, dtype, solver, precond), 256-byte
 * aligned; the handle's own scratch is not used).  *block_spmvs = the block-SpMV launches that did work, summed over the
 * blocks.  hipk_last_solve_path() reports "hipk_cg_multi launch sequence" / "hipk_bicgstab_multi launch sequence".  CSR
 * handles only (not hipk_op_create). */
size_t hipk_multi_work_bytes(int64_t n, int k, int dtype, int solver, int precond);
int hipk_cg_solve_multi(hipk_csr_t A, const void *dinv, int k, const void *B, int64_t ldb, void *X, int64_t ldx, void *work,
                        size_t work_bytes, const hipk_params *prm, hipk_stats *st, int64_t *block_spmvs, hipk_stream_t stream);
int hipk_bicgstab_solve_multi(hipk_csr_t A, const void *dinv, int k, const void *B, int64_t ldb, void *X, int64_t ldx, void *work,
                              size_t work_bytes, const hipk_params *prm, hipk_stats *st, int64_t *block_spmvs,
                              hipk_stream_t stream);
/* ---- many small systems: S independent systems with ONE sparsity pattern, one workgroup per system (csrc/hipk_batch.hip, hipk_batch_gm.hip) ----
 * System s has the shared pattern crow_dev[n + 1] / col_dev[nnz] (int32, device), the values vals + s * ldv, the right-hand side
 * B + s * ldb and x0 / the solution in X + s * ldx (device arrays of `dtype`; ldv >= nnz, ldb, ldx >= n); dinv is NULL (M = identity)
 * or the Jacobi vectors dinv + s * ldd.  Row s of the result and st[s] (st: `batch` entries) are bit for bit hipk_cg_solve /
 * hipk_pcg_solve (hipk_bicgstab_solve / hipk_pbicgstab_solve) of system s: the same params (tol through fp32, maxiter < 0 = 10 n),
 * the same stats, every system stopping -- or breaking down -- at its own iteration.  One launch of hipk_cg_batch_kernel<T, PRE> /
 * hipk_bi_batch_kernel<T, PRE> runs every system's whole solve including the true residual and `info`; a launch runs at most
 * HIPK_BATCH_LAUNCH_ITS iterations per system and the next one resumes the unfinished systems (same bits for any budget).
 * Envelope: n <= 4096 and at most 32 stored entries per row, else HIPK_ERR_UNSUPPORTED.  Row starts must be 16-byte aligned
 * (vals, B, X, dinv aligned and ld * sizeof(T) a multiple of 16), else HIPK_ERR_ALIGN; elements of a row beyond nnz or n are
 * never read or written.  A call that returns an error has written nothing, `work` included (the row bound is checked on the
 * host from a copy of crow_dev).  `work`: hipk_batch_work_bytes, 256-byte aligned, the workspace contract above.  No handle is needed
 * and no handle scratch is used.  hipk_last_solve_path() and hipk_last_solve_form() report the kernel, e.g.
 * "hipk_cg_batch_kernel<double,false>"; hipk_last_batch_launches() the launches the calling thread's last batch solve took. */
size_t hipk_batch_work_bytes(int64_t n, int64_t nnz, int batch, int dtype, int solver /* 0 cg, 1 bicgstab */, int precond);
int hipk_cg_solve_batch(int64_t n, int64_t nnz, const int32_t *crow_dev, const int32_t *col_dev, const void *vals, int64_t ldv,
                        const void *dinv /* NULL: M = identity */, int64_t ldd, int batch, const void *B, int64_t ldb, void *X,
                        int64_t ldx, int dtype, void *work, size_t work_bytes, const hipk_params *prm, hipk_stats *st /* batch entries */,
                        hipk_stream_t stream);
int hipk_bicgstab_solve_batch(int64_t n, int64_t nnz, const int32_t *crow_dev, const int32_t *col_dev, const void *vals, int64_t ldv,
                              const void *dinv, int64_t ldd, int batch, const void *B, int64_t ldb, void *X, int64_t ldx, int dtype,
                              void *work, size_t work_bytes, const hipk_params *prm, hipk_stats *st, hipk_stream_t stream);
int hipk_last_batch_launches(void);
/* Restarted GMRES for the same batches (csrc/hipk_batch_gm.hip): row s of the result and st[s] are bit for bit hipk_gmres_solve /
 * hipk_pgmres_solve of system s with the same params -- prm->restart (1 .. 31, else HIPK_ERR_UNSUPPORTED), prm->gmres_method and
 * prm->gpu_tolerances are read; iterations = restart cycles, breakdown = 1 on happy breakdown -- every system stopping at its own
 * cycle and, with HIPK_GMRES_INCREMENTAL, at its own Arnoldi step inside a cycle.  One launch of hipk_gm_batch_kernel<T, PRE> runs
 * every system's whole solve; the basis (restart + 1 vectors per system) lives in `work`.  A non-positive pivot of the normal
 * equations' Cholesky factorisation is followed by the partial-pivot elimination on the device.  A launch ends a system's work at
 * the first cycle boundary at or after HIPK_BATCH_LAUNCH_ITS Arnoldi steps and the next one resumes it (same bits for any budget).
 * Arguments, envelope, alignment, error codes and the workspace contract as hipk_cg_solve_batch; `work`:
 * hipk_gmres_batch_work_bytes (pure host code; 0 for a restart outside 1 .. 31).  hipk_last_solve_path() reports e.g.
 * "hipk_gm_batch_kernel<double,false>". */
size_t hipk_gmres_batch_work_bytes(int64_t n, int64_t nnz, int batch, int dtype, int restart, int precond);
int hipk_gmres_solve_batch(int64_t n, int64_t nnz, const int32_t *crow_dev, const int32_t *col_dev, const void *vals, int64_t ldv,
                           const void *dinv /* NULL: M = identity */, int64_t ldd, int batch, const void *B, int64_t ldb, void *X,
                           int64_t ldx, int dtype, void *work, size_t work_bytes, const hipk_params *prm, hipk_stats *st /* batch entries */,
                           hipk_stream_t stream);
/* Block-Jacobi forms of hipk_cg_solve_batch / hipk_bicgstab_solve_batch (csrc/hipk_batch_bj.hip): M_s = blockdiag(binv_s), binv_s =
 * binv + s * ldbinv the ceil(n / block_size) inverted diagonal blocks of system s, block_size x block_size each, row-major per
 * block (the layout of hipk_block_jacobi_apply; a ragged last block completed with identity); ldbinv, in elements, is at least
 * ceil(n / block_size) * block_size^2.  Row s of the result and st[s] are bit for bit the single solve of system s with that M as
 * its callable: hipk_cgm_start / hipk_cgm_direction between the fused kernels (orc_pcg_blockjacobi) resp. hipk_pbicgstab_solve_cb
 * (final test: the plain dot of z = M (b - A x) with itself).  One launch of hipk_cg_bjbatch_kernel<T> / hipk_bi_bjbatch_kernel<T>
 * runs every system's whole solve; HIPK_BATCH_LAUNCH_ITS bounds a launch as above.  Envelope: that of hipk_cg_solve_batch and
 * 1 <= block_size <= 32, else HIPK_ERR_UNSUPPORTED; a null binv, one not aligned to its element size or a short ldbinv is
 * HIPK_ERR_ARG (rows of a block need no 16-byte alignment: binv is read element by element); the other operands, error codes, the
 * write-nothing-on-error rule and the workspace contract as hipk_cg_solve_batch, `work`: hipk_bj_batch_work_bytes.
 * hipk_last_solve_path() reports e.g. "hipk_cg_bjbatch_kernel<double>". */
size_t hipk_bj_batch_work_bytes(int64_t n, int64_t nnz, int batch, int dtype, int solver /* 0 cg, 1 bicgstab */, int block_size);
int hipk_cg_solve_batch_bj(int64_t n, int64_t nnz, const int32_t *crow_dev, const int32_t *col_dev, const void *vals, int64_t ldv,
                           const void *binv, int64_t ldbinv /* elements between systems */, int block_size, int batch, const void *B,
                           int64_t ldb, void *X, int64_t ldx, int dtype, void *work, size_t work_bytes, const hipk_params *prm,
                           hipk_stats *st /* batch entries */, hipk_stream_t stream);
int hipk_bicgstab_solve_batch_bj(int64_t n, int64_t nnz, const int32_t *crow_dev, const int32_t *col_dev, const void *vals, int64_t ldv,
                                 const void *binv, int64_t ldbinv, int block_size, int batch, const void *B, int64_t ldb, void *X,
                                 int64_t ldx, int dtype, void *work, size_t work_bytes, const hipk_params *prm, hipk_stats *st,
                                 hipk_stream_t stream);
/* Placement probe for systems whose vectors live in HBM (N >> 8 M rows): the memory shape of the CG direction step (reads r, p, x;
 * writes p, x) on the three vectors, storing back the bits it loaded (safe on live data); *us_out = the fastest of `reps` (<= 16)
 * timed passes in microseconds.  40 n bytes (fp64) per pass.  On MI355X such a step runs at one of two discrete speeds depending on
 * where the allocation landed physically; the Python host re-draws the work allocation when it reads the slow one (_hipk.py). */
int hipk_placement_probe(int64_t n, const void *r, void *p, void *x, int dtype, int reps, double *us_out, hipk_stream_t stream);

/* ---- MATRIX-FREE operators (the reference's `_normalize_matvec` takes a callable for all three solvers, TSL:176-208).
 * hipk_op_create makes a handle WITHOUT a matrix: every product y = A x of a solve is `op(user, x_dev, y_dev)`, which enqueues
 * y = A(x) (vectors of `dtype`, n elements) on the solve's stream and returns 0.  The residual form b - A x, the row scaling of
 * the Jacobi forms and the fused dots of the SpMV kernels follow in one epilogue kernel with the SAME reduction spec ("tiled dot"),
 * so hipk_cg_solve / hipk_bicgstab_solve / hipk_gmres_solve (and the hipk_p* forms) run unchanged on such a handle -- device
 * stop word, one host synchronisation per GMRES cycle and none inside CG / BiCGStab -- and, when `op` computes this library's
 * SpMV of a matrix, return that matrix's solve bit for bit.  The host calls `op` when it ENQUEUES an iteration (a few ahead of the
 * device): it must not synchronise, and it may be called for a few iterations past the stop (their results are never read).
 * The one-launch small-system kernels need the matrix and are not taken.  Destroy with hipk_csr_destroy. */
typedef int (*hipk_op_fn)(void *user, const void *x_dev, void *y_dev);
int hipk_op_create(hipk_csr_t *out, int64_t n, int dtype, hipk_op_fn op, void *user, hipk_stream_t stream);

/* BiCGStab with the CALLER's preconditioner: M(user, in_dev, out_dev) enqueues out = M(in) (vectors of the handle's
 * dtype, n elements) on `stream` and returns 0; it is called for p and s of every iteration (TSL:908, 922) and once
 * for the final residual (TSL:1007).  Workspace as hipk_pbicgstab_work_bytes.  With M = diag(dinv) the iterates equal
 * hipk_pbicgstab_solve's bit for bit. */
typedef int (*hipk_precond_fn)(void *user, const void *in_dev, void *out_dev);
int hipk_pbicgstab_solve_cb(hipk_csr_t A, hipk_precond_fn M, void *user, const void *b, void *x, void *work,
                            size_t work_bytes, const hipk_params *prm, hipk_stats *st, hipk_stream_t stream);
/* GMRES with the CALLER's preconditioner, applied after every A (left preconditioning: v = M(A v) TSL:351,
 * M(b - A x) TSL:791/766, ptol from ||M b|| TSL:750).  M is called in place (in_dev == out_dev) on workspace
 * vectors.  Workspace as hipk_gmres_work_bytes. */
int hipk_pgmres_solve_cb(hipk_csr_t A, hipk_precond_fn M, void *user, const void *b, void *x, void *work,
                         size_t work_bytes, const hipk_params *prm, hipk_stats *st, hipk_stream_t stream);

/* ---- block-Jacobi preconditioner ------------------------------------------
 * out = M in with M = blockdiag(A)^-1: `binv_dev` holds the inverted block_size x block_size diagonal blocks, row-major
 * per block, ceil(n / block_size) of them (a ragged last block is padded with identity rows/columns).  The device kernel
 * behind `BlockJacobiPreconditioner`, a callable for the reference's `M` hook (TSL:849, 908, 922, 351) that cg / bicgstab /
 * gmres run between their fused kernels.  z_i is an fma chain over the block's columns in ascending order. */
int hipk_block_jacobi_apply(int64_t n, int block_size, const void *binv_dev, const void *in, void *out, int dtype,
                            hipk_stream_t stream);

/* ---- Chebyshev polynomial preconditioner ---------------------------------------------------
 * z = p_m(D^-1 A) D^-1 r, m = degree SpMVs (1 .. 32), enqueued on `stream`; never synchronises.  `dinv` is the reciprocal
 * diagonal (device, the handle's dtype), `coef_host` holds 2 m + 2 doubles on the HOST: c0, c1[1..m], c2[1..m], scale (fp32
 * handles round them to float once).  Every step is a separate rounding, no fma:
 *     step 0      d = c0 * (dinv * r),  z = d
 *     step k      res = dinv * (r - A z)  (the SpMV's residual form and row scaling, its one summation order)
 *                 d = (c1[k] * d) + (c2[k] * res),  z = z + d;  the last step stores scale * (z + d)
 * A step is ONE launch where the handle's SpMV family has the Chebyshev epilogue (res never reaches memory, z ping-pongs
 * between `z` and `work`), else the SpMV into `work` followed by a vector kernel; HIPK_CHEB_FUSED=0 forces the latter.  Same
 * bits either way.  `work`: 2 * ((n + 3) & ~3) elements (two vectors, each 16-byte aligned); r, z, work, dinv 16-byte aligned and
 * distinct.  CSR handles only (a handle from
 * hipk_op_create is refused).  May be called from inside a preconditioner callback of a solve on the same handle: it uses
 * none of the handle's reduction scratch and does not touch hipk_last_solve_path. */
int hipk_cheb_apply(hipk_csr_t A, int degree, const void *dinv, const double *coef_host, const void *r, void *z, void *work,
                    hipk_stream_t stream);

/* ---- aggregation multigrid on a grid: the transfer steps (csrc/hipk_mg.hip) ----------------------------
 * The device steps of `AggregationMultigridPreconditioner` that are not an SpMV or a Chebyshev apply.  A level is a box of
 * n0 x n1 x n2 points (each >= 1; a two-dimensional grid passes n0 = 1), row index (i0 n1 + i1) n2 + i2; the next level has
 * ceil(n_d / 2) points per dimension and the aggregate of fine point (i0, i1, i2) is coarse point (i0 / 2, i1 / 2, i2 / 2).
 * Indices are computed from the dimensions, there are no index arrays.  Every call is one streaming launch enqueued on `stream`
 * and never synchronises; vectors are of `dtype`, 16-byte aligned (else HIPK_ERR_ALIGN) and distinct; elements at and beyond
 * the vector's length are never read or written.  Every operation is a separate rounding, no fma; `omega` / `scale` are rounded
 * to `dtype` once.
 *   hipk_mg_restrict    : rc[I] = the sum of t (n0 n1 n2 elements) over the members of aggregate I in ascending fine index, left
 *                         to right, the first member starting the sum; rc has prod(ceil(n_d / 2)) elements.
 *   hipk_mg_prolong_add : z[i] = z[i] + (omega * e[agg(i)]), z of n0 n1 n2 elements, e of the coarse level's.
 *   hipk_mg_correct     : z[i] = scale * (z[i] + d[i]), i < n (the last step of a level; scale = 1 except on the finest).
 *   hipk_mg_diag        : z[i] = scale * (dinv[i] * r[i]), i < n (the level with one unknown). */
int hipk_mg_restrict(int64_t n0, int64_t n1, int64_t n2, const void *t, void *rc, int dtype, hipk_stream_t stream);
int hipk_mg_prolong_add(int64_t n0, int64_t n1, int64_t n2, double omega, const void *e, void *z, int dtype, hipk_stream_t stream);
int hipk_mg_correct(int64_t n, double scale, const void *d, void *z, int dtype, hipk_stream_t stream);
int hipk_mg_diag(int64_t n, double scale, const void *dinv, const void *r, void *z, int dtype, hipk_stream_t stream);
/* The tail of the V-cycle in ONE launch of one 256-thread workgroup (hipk_mg_tail_kernel<T>): for the run of levels
 * levels[0 .. nlev), each the ceil(d / 2) coarsening of the one before and the last with one unknown,
 *     z = scale * V(0, r),   V(j, r) = steps 1 - 6 of the class's docstring with S_j the Chebyshev recurrence of hipk_cheb_apply
 *                            (degree steps, coefficients c0, c1[k], c2[k] of the level, scale 1), V(nlev - 1, r) = dinv r,
 * bit for bit what hipk_cheb_apply, hipk_spmv_ex (mode 4), hipk_mg_restrict, hipk_mg_prolong_add, hipk_mg_correct and
 * hipk_mg_diag give on the same levels, launch by launch.  A level is described by int32 CSR arrays, values and the reciprocal
 * diagonal of `dtype` (device pointers, read only), its dimensions, n = n0 n1 n2 and `max_row`, the largest number of stored
 * entries in a row (it decides nothing but the envelope: the kernel sums a row in stored order).  The descriptors are passed
 * twice: `levels_host` for the checks and the workspace layout, `levels_dev` the same bytes in device memory (built once by the
 * caller, 16-byte aligned) for the kernel.  Envelope: n <= 4096 and max_row <= 32 on every level, else HIPK_ERR_UNSUPPORTED;
 * 1 <= nlev <= 16, 1 <= degree <= 32, consistent dimensions, else HIPK_ERR_ARG; r, z 16-byte and `work` 256-byte aligned, else
 * HIPK_ERR_ALIGN; `work` >= hipk_mg_tail_work_bytes (pure host code; 0 for bad arguments), else HIPK_ERR_WORKSPACE.  A call that
 * returns an error has launched nothing and written nothing.  The workspace contract above holds: every element of `work` the
 * kernel reads it has written before.  r: levels[0].n elements, read only; z likewise, written.  Never synchronises. */
typedef struct {
    const int32_t *crow, *col; /* device: n + 1 row pointers, the columns                          */
    const void *val, *dinv;    /* device, `dtype`: the values, the n reciprocal diagonal entries   */
    int32_t n0, n1, n2, n;     /* the level's box (a two-dimensional grid has n0 = 1), n = n0 n1 n2 */
    int32_t max_row, reserved;
    double c0, c1[32], c2[32]; /* the smoother's coefficients, c1[k - 1], c2[k - 1] for step k       */
} hipk_mg_level;
size_t hipk_mg_tail_work_bytes(const hipk_mg_level *levels_host, int nlev, int dtype);
int hipk_mg_tail_apply(const hipk_mg_level *levels_host, const void *levels_dev, int nlev, int degree, double omega, double scale,
                       const void *r, void *z, int dtype, void *work, size_t work_bytes, hipk_stream_t stream);

/* ---- aggregation multigrid on a matrix graph: the transfer steps by index arrays (csrc/hipk_mg_graph.hip) ----
 * The same steps for `AggregationMultigridPreconditioner.from_graph`, whose aggregates are not boxes.  A fine level of n rows and
 * a coarse one of nc (1 <= nc <= n < 2^31) are linked by int32 device arrays, read only:
 *   agg  : n entries, the aggregate of every fine row, in [0, nc);
 *   aptr : nc + 1 entries, aptr[0] = 0, aptr[nc] = n, strictly ascending (an aggregate has at least one member, any number);
 *   amem : n entries, amem[aptr[I] .. aptr[I + 1]) the members of aggregate I in ascending fine index.
 * The CONTENTS of the index arrays are the caller's responsibility: they are not checked.  Every call is one streaming launch
 * enqueued on `stream` and never synchronises; the kernel walks the vector it writes in the library's chunk form, 16-byte
 * groups; vectors are of `dtype`, vectors and index arrays 16-byte aligned (else HIPK_ERR_ALIGN) and distinct; elements at and
 * beyond a vector's length are never read or written.  One rounding per operation, no fma, no atomics; `omega` is rounded to
 * `dtype` once.  n or nc out of range, a null pointer or t == rc / e == z: HIPK_ERR_ARG; another dtype: HIPK_ERR_UNSUPPORTED.
 *   hipk_mg_restrict_agg    : rc[I] = t[amem[aptr[I]]], then rc[I] = rc[I] + t[amem[k]] for k = aptr[I] + 1 .. aptr[I + 1] - 1.
 *   hipk_mg_prolong_add_agg : z[i] = z[i] + (omega * e[agg[i]]), i < n. */
int hipk_mg_restrict_agg(int64_t n, int64_t nc, const int32_t *aptr, const int32_t *amem, const void *t, void *rc, int dtype,
                         hipk_stream_t stream);
int hipk_mg_prolong_add_agg(int64_t n, int64_t nc, const int32_t *agg, double omega, const void *e, void *z, int dtype,
                            hipk_stream_t stream);
/* hipk_mg_tail_apply for index-array levels (hipk_mg_gtail_kernel<T>, one launch of one 256-thread workgroup): levels[0 .. nlev),
 * level j + 1 the aggregation of level j by its agg / aptr / amem (as above, with n = levels[j].n and nc = levels[j + 1].n),
 *     z = scale * V(0, r),   V(j, r) = steps 1 - 6 with the transfers above,   V(nlev - 1, r) = dinv r  (any n >= 1 there),
 * bit for bit what hipk_cheb_apply, hipk_spmv_ex (mode 4), hipk_mg_restrict_agg, hipk_mg_prolong_add_agg, hipk_mg_correct and
 * hipk_mg_diag give on the same levels, launch by launch.  The last level's agg / aptr / amem and coefficients are not read.
 * Envelope: n <= 4096 and max_row <= 32 on every level and nlev <= 32, else HIPK_ERR_UNSUPPORTED; nlev >= 1, 1 <= degree <= 32,
 * 1 <= levels[j + 1].n <= levels[j].n, no null pointer, else HIPK_ERR_ARG.  Alignment, workspace (hipk_mg_gtail_work_bytes: pure
 * host code, 0 for bad arguments), the error contract -- an erroring call launches and writes nothing -- and the workspace
 * contract -- every byte of `work` the kernel reads it has written before -- are hipk_mg_tail_apply's. */
typedef struct {
    const int32_t *crow, *col;         /* device: n + 1 row pointers, the columns                         */
    const void *val, *dinv;            /* device, `dtype`: the values, the n reciprocal diagonal entries  */
    const int32_t *agg, *aptr, *amem;  /* device: the link to the next level (not read on the last level) */
    int32_t n, max_row;
    double c0, c1[32], c2[32];         /* the smoother's coefficients, c1[k - 1], c2[k - 1] for step k      */
} hipk_mg_glevel;
size_t hipk_mg_gtail_work_bytes(const hipk_mg_glevel *levels_host, int nlev, int dtype);
int hipk_mg_gtail_apply(const hipk_mg_glevel *levels_host, const void *levels_dev, int nlev, int degree, double omega, double scale,
                        const void *r, void *z, int dtype, void *work, size_t work_bytes, hipk_stream_t stream);

/* ---- aggregation multigrid: a dense coarsest level (csrc/hipk_mg_dense.hip) ----------------------------
 * `from_graph(coarse_rows=K)` ends the hierarchy at a level of n <= K unknowns that is solved with the stored inverse of its
 * matrix instead of being coarsened further.  cinv: n x n of `dtype` on the device, read only, column by column -- element
 * (i, j) at cinv[j ld + i], ld >= n a multiple of 4 (else HIPK_ERR_ARG / HIPK_ERR_ALIGN), 16-byte aligned; rows n .. ld - 1
 * of a column are padding and never read.  z = cinv r under this rounding spec, in segments of 64 columns:
 *     p_q = 0;  p_q = p_q + (cinv[i, j] * r[j])   for j = 64 q .. min(64 q + 64, n) - 1 ascending
 *     s   = 0;  s   = s + p_q                     for q ascending
 *     z[i] = scale * s
 * one rounding per operation, no fma, everything in `dtype`, `scale` rounded to it once.  The p_q are computed in parallel and
 * meet in LDS behind a barrier, where the thread of row i adds them in ascending q: no atomics, no hand-off between workgroups,
 * the same bits whatever the launch shape.
 *   hipk_mg_dense_apply : one launch of ceil(n / 16) (fp64; 32 rows per workgroup in fp32) workgroups of 256 threads, each on 128
 *                         bytes of every column; r is staged in LDS.  1 <= n <= 2048 (n < 1: HIPK_ERR_ARG, n > 2048:
 *                         HIPK_ERR_UNSUPPORTED); r, z of n elements, 16-byte aligned, distinct; elements at and beyond n are
 *                         never read or written.  Enqueued on `stream`, never synchronises.
 *   hipk_mg_gtail_dense_apply : hipk_mg_gtail_apply whose LAST level is dense: levels[0 .. nlev - 1) are its sparse levels under its
 *                         envelope (n <= 4096, max_row <= 32, nlev <= 32) and V(nlev - 1, r) = cinv r by the spec above, with
 *                         all 256 threads on rows x segments (scale applies there only when nlev == 1).  Of levels[nlev - 1]
 *                         only n is read, 1 <= n <= 512 (above: HIPK_ERR_UNSUPPORTED) and n <= levels[nlev - 2].n.  One launch
 *                         of one workgroup, bit for bit the launch sequence that ends in hipk_mg_dense_apply.  Workspace
 *                         (hipk_mg_gtail_dense_work_bytes: pure host code, 0 for bad arguments), alignment and the error
 *                         contract -- an erroring call launches and writes nothing -- are hipk_mg_gtail_apply's. */
int hipk_mg_dense_apply(int64_t n, int64_t ld, const void *cinv, double scale, const void *r, void *z, int dtype, hipk_stream_t stream);
size_t hipk_mg_gtail_dense_work_bytes(const hipk_mg_glevel *levels_host, int nlev, int dtype);
int hipk_mg_gtail_dense_apply(const hipk_mg_glevel *levels_host, const void *levels_dev, int nlev, int degree, double omega, double scale,
                              const void *cinv, int64_t ld, const void *r, void *z, int dtype, void *work, size_t work_bytes,
                              hipk_stream_t stream);

/* ---- aggregation multigrid: the W-cycle (csrc/hipk_mg_w.hip) -------------------------------------------
 * `AggregationMultigridPreconditioner(cycle="W")`: W(l, r) is V(l, r) whose step 4 reads, where level l + 1 is smoothed (it is
 * not the last level),
 *     e = W(l + 1, rc);  rc2 = rc - A_{l+1} e;  e2 = W(l + 1, rc2);  e = e + e2
 * every step one rounding, no fma; the last level is visited once per visit of the level above it.
 *   hipk_mg_add : e[i] = e[i] + e2[i], i < n (the last line above), in hipk_mg_correct's form: 16-byte groups, one ragged group,
 *                 nothing at or beyond n touched.  n >= 1 and two distinct non-null vectors, else HIPK_ERR_ARG; 16-byte aligned,
 *                 else HIPK_ERR_ALIGN; another dtype: HIPK_ERR_UNSUPPORTED.
 *   hipk_mg_tail_apply_w, hipk_mg_gtail_apply_w, hipk_mg_gtail_dense_apply_w : hipk_mg_tail_apply, hipk_mg_gtail_apply and
 *                 hipk_mg_gtail_dense_apply with the W-cycle: the same descriptors, arguments, checks and error codes, ONE launch
 *                 of one 256-thread workgroup that runs the whole W walk over its levels (level j >= 1 of nlev is visited
 *                 2^min(j, nlev - 2) times), bit for bit the W launch sequence.  nlev <= 2 is the V entry's result bit for bit.
 *                 More than 12 levels: HIPK_ERR_UNSUPPORTED.  The slab holds SIX vectors per level, r | z | t | d | w | e: `work`
 *                 >= the entry's *_work_bytes_w (pure host code; 0 for bad arguments or more than 12 levels), else
 *                 HIPK_ERR_WORKSPACE.  A call that returns an error has launched nothing and written nothing. */
int hipk_mg_add(int64_t n, const void *e2, void *e, int dtype, hipk_stream_t stream);
size_t hipk_mg_tail_work_bytes_w(const hipk_mg_level *levels_host, int nlev, int dtype);
int hipk_mg_tail_apply_w(const hipk_mg_level *levels_host, const void *levels_dev, int nlev, int degree, double omega, double scale,
                         const void *r, void *z, int dtype, void *work, size_t work_bytes, hipk_stream_t stream);
size_t hipk_mg_gtail_work_bytes_w(const hipk_mg_glevel *levels_host, int nlev, int dtype);
int hipk_mg_gtail_apply_w(const hipk_mg_glevel *levels_host, const void *levels_dev, int nlev, int degree, double omega, double scale,
                          const void *r, void *z, int dtype, void *work, size_t work_bytes, hipk_stream_t stream);
size_t hipk_mg_gtail_dense_work_bytes_w(const hipk_mg_glevel *levels_host, int nlev, int dtype);
int hipk_mg_gtail_dense_apply_w(const hipk_mg_glevel *levels_host, const void *levels_dev, int nlev, int degree, double omega, double scale,
                                const void *cinv, int64_t ld, const void *r, void *z, int dtype, void *work, size_t work_bytes,
                                hipk_stream_t stream);

/* ---- aggregation multigrid: the refresh of a hierarchy (csrc/hipk_mg_refresh.hip) ----------------------
 * `AggregationMultigridPreconditioner.update(A_new)` keeps the aggregates and every index array of a hierarchy and recomputes
 * its numbers.  The Galerkin values of the next level are hipk_mg_restrict_agg over the stored sort order of the entries
 * ((n, nc, aptr, amem, t, rc) = (nnz_l, nnz_{l+1}, gptr, gsrc, val_l, val_{l+1})); what a level then needs from its values is
 *   hipk_mg_level_scan : for a level of n rows (1 <= n < 2^31, else HIPK_ERR_ARG) given by int32 crow (n + 1 entries) / col and
 *                        val of `dtype` (device, read only; their CONTENTS are the caller's responsibility), for every row i
 *                            d_i = 0;  d_i = d_i + a    over the stored entries with col == i, in stored order
 *                            s_i = 0;  s_i = s_i + |a|  over all stored entries of the row, in stored order
 *                            dinv[i] = 1 / d_i          the correctly rounded quotient (inf for d_i = 0)
 *                            q_i = (double)s_i / (double)d_i
 *                        one rounding per operation in `dtype`, no fma, a row of any length; dinv has n elements and nothing at or
 *                        beyond n is written.  out (device, two doubles): out[0] = max_i q_i, NaN when a q_i is NaN (torch.max);
 *                        out[1] = the number of rows with d_i <= 0.  want_lmax = 0 forms neither s_i nor q_i and writes
 *                        out[0] = 0 (the level that only needs dinv); another value than 0 / 1 is HIPK_ERR_ARG.
 * Two launches enqueued on `stream`: the scan walks dinv in the library's chunk form, 16-byte groups, and leaves one pair of
 * doubles per workgroup in `work`; one workgroup folds them into `out`.  No atomics, no hand-off between workgroups, every byte
 * of `work` read has been written by the launch before, the same bits whatever `work` held.  crow, col, val, dinv, out, work
 * 16-byte aligned, else HIPK_ERR_ALIGN; a null pointer or val == dinv: HIPK_ERR_ARG; another dtype: HIPK_ERR_UNSUPPORTED;
 * `work` >= hipk_mg_level_scan_work_bytes(n) (pure host code; 0 for n out of range), else HIPK_ERR_WORKSPACE.  A call that
 * returns an error has launched nothing and written nothing.  Never synchronises. */
size_t hipk_mg_level_scan_work_bytes(int64_t n);
int hipk_mg_level_scan(int64_t n, const int32_t *crow, const int32_t *col, const void *val, int dtype, int want_lmax, void *dinv,
                       double *out, void *work, size_t work_bytes, hipk_stream_t stream);

/* ---- step API: externally driven loops (row-partitioned multi-GPU CG) ------------
 * The reference is single-device; the row-partitioned solver (north_star) drives the
 * SAME fused kernels from the host side of each rank and exchanges (a) the x-vector
 * halo and (b) the chunk partial sums between launches.  Rows are partitioned on
 * reduction-chunk boundaries of the GLOBAL problem, so every rank reduces the
 * all-gathered partials in the same fixed order: results are bitwise identical to the
 * single-GPU solve for any rank count.
 *   chunk_rows : chunk size of the GLOBAL row count (hipk_chunk_size(n_global))
 *   g_red      : number of partials of ALL ranks (hipk_chunk_count(n_global))
 * Kernels index partial OUTPUTS by local chunk and read partial INPUTS from the
 * gathered (global) arrays.
 * The vector operands of hipk_cg_* / hipk_cgm_* (r, p, x, Ap, z) must be 16-byte
 * aligned, as those of hipk_dot_parts and hipk_spmv_ex: HIPK_ERR_ALIGN otherwise,
 * checked before any launch (tests/test_gpu_step_api.py pins every entry point
 * call by call against tests/_step_mirror.py). */
int hipk_csr_create_ex(hipk_csr_t *out, int64_t n_rows, int64_t n_cols, int64_t nnz,
                       const void *crow_dev, const void *col_dev, int idx_bytes,
                       const void *val_dev, int dtype, int chunk_rows, hipk_stream_t stream);
/* mode bits: 1 part0[c] = <w, out>; 2 part1[c] = <out, out>; 4 out = bsub - A x */
int hipk_spmv_ex(hipk_csr_t h, const void *x, void *y, int mode, const void *w, const void *bsub,
                 double *part0, double *part1, const int64_t *stop_dev, int64_t it,
                 hipk_stream_t stream);
int hipk_dot_parts(int64_t n, int chunk_rows, const void *x, const void *y, int dtype,
                   double *part, hipk_stream_t stream);
/* out_dev[0] = fixed-order sum of part[0..g)  (the second level of every dot) */
int hipk_reduce_parts(const double *part_dev, int g, double *out_dev, hipk_stream_t stream);
/* dst[i] = src[idx[i]], i < m  (halo pack) */
int hipk_gather(int64_t m, const int32_t *idx_dev, const void *src, void *dst, int dtype,
                hipk_stream_t stream);
size_t hipk_cg_scal_bytes(void); /* device scalar block: {gamma[2], atol2, bs, res2, xx, stop_it(int64), host signal ptr (null here)} */
int hipk_cg_start(int64_t n_local, int chunk_rows, int g_red, void *scal_dev, const double *part_rr,
                  const double *part_bb, const void *r, void *p, int dtype, double tol, double atol,
                  int64_t maxiter, hipk_stream_t stream);
/* r -= alpha Ap, partials of <r,r>   (alpha = gamma / sum(part_pAp)) */
int hipk_cg_update(int64_t n_local, int chunk_rows, int g_red, const void *scal_dev, int64_t it,
                   const double *part_pAp, const void *Ap, void *r, double *part_rr_out, int dtype,
                   hipk_stream_t stream);
/* x += alpha p alone (alpha = gamma / sum(part_pAp), the bits hipk_cg_update / hipk_cg_direction derive): for a caller that
 * runs it on a side stream while a collective is in flight and then calls hipk_cg_direction with x = NULL */
int hipk_cg_xupdate(int64_t n_local, int chunk_rows, int g_red, const void *scal_dev, int64_t it, const double *part_pAp,
                    const void *p, void *x, int dtype, hipk_stream_t stream);
/* x += alpha p; p = r + beta p; gamma <- <r,r>; stop test   (the x update rides on the pass over p; x = NULL: p only) */
int hipk_cg_direction(int64_t n_local, int chunk_rows, int g_red, void *scal_dev, int64_t it,
                      int64_t maxiter, const double *part_pAp, const double *part_rr, const void *r, void *p,
                      void *x, int dtype, hipk_stream_t stream);

/* CG with a CALLABLE preconditioner (`M` of cg(), TSL:821, 849): the host runs
 *   hipk_spmv_ex(p -> Ap, <p,Ap>) | hipk_cg_update | z = M(r) (the caller's own device code, same stream) |
 *   hipk_dot_parts(r, z) | hipk_cgm_direction
 * gamma = <r,z> steers alpha / beta, the stop test uses <r,r> (TSL:835-841). */
int hipk_cgm_start(int64_t n_local, int chunk_rows, int g_red, void *scal_dev, const double *part_rz,
                   const double *part_rr, const double *part_bb, const void *z, void *p, int dtype,
                   double tol, double atol, int64_t maxiter, hipk_stream_t stream);
/* x += alpha p; p = z + beta p; gamma <- <r,z>; stop test on <r,r> */
int hipk_cgm_direction(int64_t n_local, int chunk_rows, int g_red, void *scal_dev, int64_t it, int64_t maxiter,
                       const double *part_pAp, const double *part_rz, const double *part_rr, const void *z,
                       void *p, void *x, int dtype, hipk_stream_t stream);

/* ---- row-partitioned CG, the whole loop of one rank driven from C (north_star: "the SpMV shards row-blocks across the
 * GPUs with an RCCL allgather of the x-vector halo and an allreduce for the global dot") ----------------------------------
 * The collectives are called through function pointers the caller resolves from the librccl that created `comm`
 * (signatures of ncclGroupStart / ncclGroupEnd / ncclAllGather / ncclSend / ncclRecv; datatype 8 = ncclFloat64), on the
 * solver's stream.  Tests plug in host-staged stand-ins. */
typedef struct {
    int (*group_start)(void);
    int (*group_end)(void);
    int (*all_gather)(const void *send, void *recv, size_t count, int datatype, void *comm, void *stream);
    int (*send)(const void *buf, size_t count, int datatype, int peer, void *comm, void *stream);
    int (*recv)(void *buf, size_t count, int datatype, int peer, void *comm, void *stream);
    void *comm;
    void *fused;   /* NULL, or a hipk_p2p_t created with a fused area (hipk_p2p_create2): hipk_dist_cg_solve then folds the two
                      exchanges of an iteration into its update / direction kernels (csrc/hipk_fx.h) -- no collective launch inside
                      the loop; the entry points above still serve the set-up and the final residual */
} hipk_rccl;

/* One rank's view of the partition (pytorch_sparse_solver/distributed.py: RowPartition + HaloPlan). */
typedef struct {
    int32_t rank, world;
    int64_t n_local;   /* rows this rank owns (> 0 on every rank)                                        */
    int64_t n_ext;     /* n_local + number of halo entries: length of x, p, r                            */
    int64_t n_global;
    int32_t chunk_rows; /* reduction chunk of the GLOBAL problem (hipk_chunk_size(n_global))              */
    int32_t g_red;      /* partials of all ranks (hipk_chunk_count(n_global))                             */
    int32_t per;        /* chunks per rank, the all-gather count (per * world >= g_red)                   */
    int32_t halo_mode;  /* 1: neighbour send/recv pairs; 0: all-gather of slabs padded to `slab` entries  */
    int32_t n_send;     /* owned entries other ranks need, grouped by destination rank                    */
    int32_t n_ghost;    /* = n_ext - n_local                                                              */
    int32_t slab;       /* halo_mode 0: padded slab length                                                */
    int32_t reserved;
    const int32_t *send_idx_dev;  /* [n_send] local row of each packed entry                              */
    const int32_t *ghost_src_dev; /* [n_ghost] halo_mode 0: position of each halo entry in the gathered slabs */
    const int32_t *send_off_dev;  /* device, [world + 1] or NULL: bounds of each destination's group in send_idx_dev (fused exchanges) */
    const int64_t *dest_off_dev;  /* device, [world] or NULL: where this rank's group starts in each destination's ghost tail     */
    const int32_t *send_counts;   /* host, [world]: entries sent to each rank                             */
    const int32_t *recv_counts;   /* host, [world]: halo entries received from each rank (in rank order)  */
    const int64_t *send_first;    /* host, [world] or NULL: halo_mode 1, >= 0 where the entries for that rank are the
                                     CONTIGUOUS local rows send_first[p] .. + send_counts[p] (row blocks of a stencil):
                                     they are sent straight from the vector, and when that holds for every peer the pack
                                     kernel is not launched at all                                       */
} hipk_dist_plan;

size_t hipk_dist_cg_work_bytes(const hipk_dist_plan *plan);
/* `A_local`: this rank's row block with columns renumbered to [0, n_ext) (hipk_csr_create_ex with the global chunk size).
 * x_ext: n_ext doubles, x0 in the first n_local on entry, the solution there on return.  params.check_every = batch
 * size of the loop (default 16).  Same `info` rule and, bit for bit, the same iterates as hipk_cg_solve on the whole
 * system (TSL:806-856, 968-1016). */
int hipk_dist_cg_solve(hipk_csr_t A_local, const hipk_dist_plan *plan, const hipk_rccl *coll, const void *b_local,
                       void *x_ext, void *work, size_t work_bytes, const hipk_params *prm, hipk_stats *st,
                       hipk_stream_t stream);

/* Row-partitioned BiCGStab (TSL:859-964 via `_isolve`): the same conventions and the same plan / collective structs; x_ext carries
 * x0 / the solution in its first n_local entries.  Bit for bit the iterates, counts and breakdown codes of hipk_bicgstab_solve on
 * the whole system.  Five collective launches per iteration (the all-gathers of the six dots' partials, the halos of p and s). */
size_t hipk_dist_bicgstab_work_bytes(const hipk_dist_plan *plan);
int hipk_dist_bicgstab_solve(hipk_csr_t A_local, const hipk_dist_plan *plan, const hipk_rccl *coll, const void *b_local,
                             void *x_ext, void *work, size_t work_bytes, const hipk_params *prm, hipk_stats *st,
                             hipk_stream_t stream);

/* Row-partitioned GMRES (TSL:641-803; params.restart <= 31 -- 32 .. 255: hipk_dist_gmres_wide_solve below --, params.gmres_method,
 * params.gpu_tolerances as hipk_gmres_solve): the
 * kernels of the large-system path with in-place all-gathers of their chunk partials and the halo of v_k before each SpMV; bit for
 * bit the iterates, cycle and operator-application counts of hipk_gmres_solve on the whole system.  per * world <= 2048. */
size_t hipk_dist_gmres_work_bytes(const hipk_dist_plan *plan, int restart);
int hipk_dist_gmres_solve(hipk_csr_t A_local, const hipk_dist_plan *plan, const hipk_rccl *coll, const void *b_local,
                          void *x_ext, void *work, size_t work_bytes, const hipk_params *prm, hipk_stats *st,
                          hipk_stream_t stream);

/* Row-partitioned GMRES at params.restart 32 .. 255 (any other restart: HIPK_ERR_ARG "restart must be in [32, 255]", and the
 * work-bytes functions return 0).  Arguments, plan / collective structs and the bitwise contract of hipk_dist_gmres_solve; H, R
 * and the Givens pairs live in the workspace as in hipk_gmres_solve beyond restart 31.  The multi-dot partials of an Arnoldi
 * step travel in ONE in-place all-gather of (k + 1) * per doubles per CGS pass, whatever k: per step the halo of v_k, then
 * all-gathers of per, (k + 1) per, per, (k + 1) per, per doubles.  hipk_dist_pgmres_wide_solve: the Jacobi form, arguments of
 * hipk_dist_pgmres_solve. */
size_t hipk_dist_gmres_wide_work_bytes(const hipk_dist_plan *plan, int restart);
int hipk_dist_gmres_wide_solve(hipk_csr_t A_local, const hipk_dist_plan *plan, const hipk_rccl *coll, const void *b_local,
                               void *x_ext, void *work, size_t work_bytes, const hipk_params *prm, hipk_stats *st,
                               hipk_stream_t stream);

/* The three row-partitioned loops with the Jacobi preconditioner M = diag(dinv): the same plan / collective structs and
 * conventions as above, bit for bit the iterates, counts and `info` of hipk_pcg_solve / hipk_pbicgstab_solve / hipk_pgmres_solve
 * on the whole system.  `dinv_ext`: device, n_ext doubles -- the reciprocal diagonal of this rank's rows, then its entries at
 * the halo positions (the owners' values, in the plan's ghost order).  CG reads the halo tail (it forms z = dinv .* r on the
 * ghost rows); BiCGStab and GMRES read the first n_local entries.
 *   CG       : two collective launches per iteration, as hipk_dist_cg_solve; the second carries the <r,r> and <r,z> partials
 *              and the halo of r in one group.  The fused exchanges of hipk_rccl.fused are not taken.
 *   BiCGStab : the halos of phat = M p and shat = M s instead of p and s; five collective launches per iteration.
 *   GMRES    : left preconditioning, w = M (A v_k); restart <= 31 (32 .. 255: hipk_dist_pgmres_wide_solve). */
size_t hipk_dist_pcg_work_bytes(const hipk_dist_plan *plan);
int hipk_dist_pcg_solve(hipk_csr_t A_local, const hipk_dist_plan *plan, const hipk_rccl *coll, const void *dinv_ext,
                        const void *b_local, void *x_ext, void *work, size_t work_bytes, const hipk_params *prm,
                        hipk_stats *st, hipk_stream_t stream);
size_t hipk_dist_pbicgstab_work_bytes(const hipk_dist_plan *plan);
int hipk_dist_pbicgstab_solve(hipk_csr_t A_local, const hipk_dist_plan *plan, const hipk_rccl *coll, const void *dinv_ext,
                              const void *b_local, void *x_ext, void *work, size_t work_bytes, const hipk_params *prm,
                              hipk_stats *st, hipk_stream_t stream);
size_t hipk_dist_pgmres_work_bytes(const hipk_dist_plan *plan, int restart);
int hipk_dist_pgmres_solve(hipk_csr_t A_local, const hipk_dist_plan *plan, const hipk_rccl *coll, const void *dinv_ext,
                           const void *b_local, void *x_ext, void *work, size_t work_bytes, const hipk_params *prm,
                           hipk_stats *st, hipk_stream_t stream);
/* ... and at restart 32 .. 255 (see hipk_dist_gmres_wide_solve). */
size_t hipk_dist_pgmres_wide_work_bytes(const hipk_dist_plan *plan, int restart);
int hipk_dist_pgmres_wide_solve(hipk_csr_t A_local, const hipk_dist_plan *plan, const hipk_rccl *coll, const void *dinv_ext,
                                const void *b_local, void *x_ext, void *work, size_t work_bytes, const hipk_params *prm,
                                hipk_stats *st, hipk_stream_t stream);

/* The Chebyshev polynomial preconditioner of the GLOBAL system on a row block, and the row-partitioned CG that runs it (csrc/
 * hipk_dist_cheb.h).  `degree`, `coef_host` as hipk_cheb_apply (2 m + 2 doubles on the host); `dinv_ext` as in the Jacobi loops
 * above: n_ext doubles, the rank's reciprocal diagonal and then the owners' entries at the halo positions.  degree outside [1, 32]:
 * HIPK_ERR_ARG.  fp64; the fused exchanges of hipk_rccl.fused are not taken.
 *   hipk_dist_cheb_apply : z_ext[0 .. n_local) = this rank's rows of M r, r_ext[0 .. n_local) this rank's rows of r (n_ext doubles
 *              each; both ghost tails are overwritten).  The recurrence and rounding spec of hipk_cheb_apply on the rectangular
 *              block handle: step k gathers z_{k-1} over own and ghost columns, a halo exchange fills the ghost tail of z_k before
 *              step k + 1 -- m halo exchanges (r, z_1 .. z_{m-1}), no reduction.  One launch per step where the block handle's SpMV
 *              has the Chebyshev epilogue (z ping-pongs between z_ext and the workspace, z_m landing in z_ext), else SpMV +
 *              hipk_cheb_step_kernel (also with HIPK_CHEB_FUSED=0); hipk_last_spmv_kernel() tells which.  Concatenated over the
 *              ranks: bit for bit hipk_cheb_apply on the whole matrix.  Every rank calls it; never synchronises.
 *   hipk_dist_chebcg_solve : CG with that M, arguments and conventions of hipk_dist_pcg_solve; bit for bit the iterates, counts and
 *              `info` of the single-device cg with M = the Chebyshev preconditioner of the whole matrix (gamma = <r,z>, stop test
 *              on <r,r>, info from ||M (b - A x)||).  Per iteration m + 2 collective launches: all-gather <p,Ap> | update + step 0
 *              in one kernel | ONE group: all-gather <r,r> + halo of r | steps 1 .. m with a stand-alone halo of z_k before step
 *              k + 1 | ONE group: all-gather <r,z> + halo of z_m | direction over n_ext.  hipk_last_solve_path() reports
 *              "hipk_dist_chebcg launch sequence". */
size_t hipk_dist_cheb_work_bytes(const hipk_dist_plan *plan);
int hipk_dist_cheb_apply(hipk_csr_t A_local, const hipk_dist_plan *plan, const hipk_rccl *coll, int degree, const void *dinv_ext,
                         const double *coef_host, void *r_ext, void *z_ext, void *work, size_t work_bytes, hipk_stream_t stream);
size_t hipk_dist_chebcg_work_bytes(const hipk_dist_plan *plan);
int hipk_dist_chebcg_solve(hipk_csr_t A_local, const hipk_dist_plan *plan, const hipk_rccl *coll, int degree, const void *dinv_ext,
                           const double *coef_host, const void *b_local, void *x_ext, void *work, size_t work_bytes,
                           const hipk_params *prm, hipk_stats *st, hipk_stream_t stream);

/* ---- EXPERIMENTAL peer-to-peer exchange provider for the loop above (csrc/hipk_p2p.hip) ---------------------------------
 * Each rank owns a device mailbox that every peer maps through HIP IPC; an all-gather is ONE small kernel per rank (publish
 * blocks store into the peers' mailboxes, collect blocks wait on per-source sequence flags).  No reference counterpart.
 * Protocol: create on every rank -> export the 64-byte handle -> exchange the handles out of band (rank order) -> connect.
 * hipk_p2p_group_start/_group_end/_all_gather have the signatures of the hipk_rccl members (comm = the hipk_p2p_t);
 * leave hipk_rccl.send/.recv NULL and hipk_dist_plan.halo_mode 0.  max_count = the largest `count` of any call. */
typedef struct hipk_p2p_s *hipk_p2p_t;
int hipk_p2p_create(hipk_p2p_t *out, int rank, int world, size_t max_count);
/* ... with a FUSED AREA for a partition of fx_per chunks per rank and at most fx_ghost_cap ghost entries on any rank (the same two
 * numbers on every rank): per-source sequence flags, the gathered partial arrays and the ghost tail of both exchanges of a CG
 * iteration, written by the peers' update / direction kernels themselves (csrc/hipk_fx.h; hipk_rccl.fused). */
int hipk_p2p_create2(hipk_p2p_t *out, int rank, int world, size_t max_count, int fx_per, int fx_ghost_cap);
int hipk_p2p_export(hipk_p2p_t c, void *handle64);
int hipk_p2p_connect(hipk_p2p_t c, const void *handles /* world x 64 bytes */);
int hipk_p2p_destroy(hipk_p2p_t c);
int hipk_p2p_error(hipk_p2p_t c); /* 1: a wait gave up (a peer never published) since the last query -- the results of the calls in
                                     between are void; the query clears the flag */
int hipk_p2p_group_start(void);
int hipk_p2p_group_end(void);
int hipk_p2p_all_gather(const void *send, void *recv, size_t count, int datatype, void *comm, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HIPK_H */
