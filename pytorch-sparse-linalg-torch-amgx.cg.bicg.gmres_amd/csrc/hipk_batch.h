// hipk_batch.h -- what the one-workgroup-per-system kernels share (hipk_batch.hip: CG and BiCGStab; hipk_batch_gm.hip: GMRES):
// the record and the argument block of a launch, the LDS carve, 16-byte loads and stores in the virtual-thread layout, the folds of
// the plain and the tiled dot, the SpMV with fused dots, and what a launch does on entry and when its budget is used up.
#pragma once

#include <cstdint>
#include <cstring>
#include <vector>

#include "hipk_common.h"
#include "hipk_solve.h"
#include "hipk_switch.h"

#define HIPK_BATCH_MAX_N 4096
#define HIPK_BATCH_MAX_ROW 32
#define HIPK_BATCH_EPS64 2.220446049250313e-16   // torch.finfo(torch.float64).eps
#define HIPK_BATCH_EPS32 1.1920928955078125e-07  // torch.finfo(torch.float32).eps

// slots of the scalar block (doubles) ...
enum {
    BS_BS, BS_ATOL2, BS_GAMMA, BS_RS, BS_ALPHA, BS_BETA, BS_OMEGA, BS_RHO, BS_RS_NEXT, BS_RHO_NEXT, BS_RHO_NEW, BS_ALPHA_NEW,
    BS_OMEGA_NEW, BS_RES2, BS_XX, BS_ND
};
// ... and its words (int64)
enum { BI_K, BI_MATVECS, BI_CODE, BI_ITS, BI_EXIT_EARLY, BI_GO, BI_NI };
// BI_GO: what the workgroup does next
enum { GO_ITERATE = 1, GO_FINISH = 2, GO_SAVE = 3 };
enum { BATCH_RUNNING = 0x52554e, BATCH_DONE = 0x444f4e45 };

// one system's record in `work`: the stats the host copies out, then the state a launch leaves for the next one
struct hipk_batch_rec {
    int64_t iterations, matvecs;
    int32_t info, breakdown;
    double b_norm, residual_norm, x_norm, threshold, recurrence_rs;
    int32_t status, launches;
    double sd[BS_ND];
    int64_t si[BI_NI];
};
static_assert(sizeof(hipk_batch_rec) <= 256, "a record is 256 bytes");
#define HIPK_BATCH_REC 256
#define HIPK_BATCH_HEAD 256   // int unfinished

struct hipk_batch_args {
    int n, g, ntile, resume;
    const int *crow, *col;
    const void *vals, *dinv, *B;
    void *X;
    int64_t ldv, ldd, ldb, ldx;
    char *recs, *slabs;
    size_t slab_bytes, vec_bytes;
    int *unfinished;
    double tol2, atol_sq, tol_f, atol_f;   // tol, atol rounded through fp32; their fp32 squares
    int64_t maxiter, budget;
    int nvp;   // n rounded up to a multiple of 4: the stride of the LDS vectors (16-byte aligned starts)
};

// LDS: red[4][256] | sw[2][64] | sd[BS_ND (<= 16)] | si[BI_NI (<= 8)] | vectors
#define HIPK_BATCH_LDS_FIXED ((4 * 256 + 2 * 64 + 16 + 8) * 8)

// ---------------------------------------------------------------------------------------------------------------- device helpers
template <typename T>
struct hipk_beps;
template <>
struct hipk_beps<double> {
    static constexpr double v = HIPK_BATCH_EPS64;
};
template <>
struct hipk_beps<float> {
    static constexpr double v = HIPK_BATCH_EPS32;
};

// the VEC elements at `base` (a multiple of VEC) of a vector of n: one 16-byte access when they all exist
template <typename T>
__device__ __forceinline__ void hipk_bld(const T *p, int base, int n, T (&v)[hipk_vec<T>::VEC]) {
    constexpr int VEC = hipk_vec<T>::VEC;
    typedef T vt __attribute__((ext_vector_type(VEC)));
    if (base + VEC <= n) {
        const vt q = *(const vt *)(p + base);
#pragma unroll
        for (int i = 0; i < VEC; ++i) v[i] = q[i];
    } else {
#pragma unroll
        for (int i = 0; i < VEC; ++i) v[i] = (base + i < n) ? p[base + i] : (T)0;
    }
}
template <typename T>
__device__ __forceinline__ void hipk_bst(T *p, int base, int n, const T (&v)[hipk_vec<T>::VEC]) {
    constexpr int VEC = hipk_vec<T>::VEC;
    typedef T vt __attribute__((ext_vector_type(VEC)));
    if (base + VEC <= n) {
        vt q;
#pragma unroll
        for (int i = 0; i < VEC; ++i) q[i] = v[i];
        *(vt *)(p + base) = q;
    } else {
#pragma unroll
        for (int i = 0; i < VEC; ++i)
            if (base + i < n) p[base + i] = v[i];
    }
}

// the elements thread t owns in the virtual-thread layout: chunk c, then blocks of 256 VEC elements, VEC at `base`
#define HIPK_B_FOR_OWN(T, c, base)                                                                          \
    _Pragma("unroll") for (int c = 0; c < 2; ++c)                                                           \
        if (c < g)                                                                                          \
            for (int base = c * HIPK_BASE_CHUNK + hipk_vec<T>::VEC * (int)threadIdx.x,                      \
                     _end = ((c + 1) * HIPK_BASE_CHUNK < n ? (c + 1) * HIPK_BASE_CHUNK : n);                \
                 base < _end; base += HIPK_THREADS * hipk_vec<T>::VEC)

// reduce_parts of the oracle over at most 8 partials: thread t of 256 holds 0.0 + part[t], the tree folds v[t] += v[t + s],
// s = 128 .. 1; beyond the partials every operand is +0.0, which changes nothing
__device__ __forceinline__ double hipk_bfold8(const double (&p)[8], int cnt) {
    double v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (i < cnt) ? 0.0 + p[i] : 0.0;
    return ((v[0] + v[4]) + (v[2] + v[6])) + ((v[1] + v[5]) + (v[3] + v[7]));
}
__device__ __forceinline__ double hipk_bfold2(double p0, double p1, int g) {
    const double a = 0.0 + p0, b = (g > 1) ? 0.0 + p1 : 0.0;
    return a + b;
}

// K plain sums at once: v[k] of the 256 threads with the spec's tree (v[t] += v[t+128], v[t] += v[t+64], the wavefront tree).
// Result in v[k] of THREAD 0 only.  red: K x 256 doubles.  The caller's next barrier makes red reusable.
template <int K>
__device__ __forceinline__ void hipk_bsums_t0(double (&v)[K], double *red) {
    const int t = threadIdx.x;
#pragma unroll
    for (int k = 0; k < K; ++k) red[k * 256 + t] = v[k];
    __syncthreads();
    if (t < 64) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const double *r = red + k * 256;
            v[k] = hipk_wave_sum((r[t] + r[t + 128]) + (r[t + 64] + r[t + 192]));
        }
    }
}

// the tiled dot's second and third level (thread 0): tile partial (sw0 + sw1) + (sw2 + sw3), the tiles of a chunk folded like chunk
// partials, then the chunks.  sw: [tile][wavefront]
__device__ __forceinline__ double hipk_btiled_t0(const double *sw, int ntile, int g) {
    double part[2] = {0.0, 0.0};
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        if (c < g) {
            double tp[8];
            const int cnt = ntile - 8 * c < 8 ? ntile - 8 * c : 8;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const double *q = sw + (8 * c + i) * 4;
                tp[i] = (i < cnt) ? (q[0] + q[1]) + (q[2] + q[3]) : 0.0;
            }
            part[c] = hipk_bfold8(tp, cnt);
        }
    }
    return hipk_bfold2(part[0], part[1], g);
}

// y = A x over the workgroup's rows, x in LDS: row t + 256 k of tile k, summed in stored order.  f(row, sum, pr) stores what the
// caller wants of the row and returns the ND products of the fused dots; their wavefront sums land in sw[d][tile][wavefront].
template <typename T, int ND, typename F>
__device__ __forceinline__ void hipk_bspmv(const hipk_batch_args &a, const T *__restrict__ vals, const T *xg, double *sw, F f) {
    const int t = threadIdx.x;
    for (int tile = 0; tile < a.ntile; ++tile) {
        const int row = tile * HIPK_THREADS + t;
        double pr[ND > 0 ? ND : 1];
#pragma unroll
        for (int d = 0; d < ND; ++d) pr[d] = 0.0;
        if (row < a.n) {
            const int lo = a.crow[row], hi = a.crow[row + 1];
            T s = (T)0;
            for (int j = lo; j < hi; ++j) {
                const T p = vals[j] * xg[a.col[j]];
                s = s + p;
            }
            f(row, s, pr);
        }
#pragma unroll
        for (int d = 0; d < ND; ++d) {
            const double w = hipk_wave_sum(pr[d]);
            if ((t & 63) == 0) sw[d * 64 + tile * 4 + (t >> 6)] = w;
        }
    }
}

// info as `_isolve` decides it (TSL:1007-1016), from the squares
__device__ __forceinline__ void hipk_bfinish(hipk_batch_rec *rec, const hipk_batch_args &a, const double *sd, const int64_t *si) {
    const double bs = sd[BS_BS], r2 = sd[BS_RES2], xx = sd[BS_XX];
    rec->iterations = si[BI_K];
    rec->matvecs = si[BI_MATVECS];
    rec->breakdown = (int32_t)si[BI_CODE];
    rec->b_norm = sqrt(bs < 0.0 ? 0.0 : bs);
    rec->residual_norm = sqrt(r2 < 0.0 ? 0.0 : r2);
    rec->x_norm = sqrt(xx < 0.0 ? 0.0 : xx);
    const double u = a.tol_f * rec->b_norm, w = a.atol_f;
    rec->threshold = (u != u || w != w) ? __builtin_nan("") : (u > w ? u : w);   // torch.maximum: NaN wins
    rec->info = (rec->x_norm != rec->x_norm || rec->residual_norm > rec->threshold) ? -1 : 0;
    rec->recurrence_rs = sd[BS_RS];
    rec->status = BATCH_DONE;
}

struct hipk_batch_lds {
    double *red, *sw, *sd;
    int64_t *si;
    unsigned char *vec;
};
__device__ __forceinline__ hipk_batch_lds hipk_batch_carve(unsigned char *raw) {
    hipk_batch_lds l;
    l.red = (double *)raw;
    l.sw = l.red + 4 * 256;
    l.sd = l.sw + 2 * 64;
    l.si = (int64_t *)(l.sd + 16);
    l.vec = (unsigned char *)(l.si + 8);
    return l;
}

// what every launch does first: a finished system leaves, a fresh one clears its scalar block, an unfinished one reloads it
// (thread 0; the caller's next barrier publishes).  Returns false when the workgroup has nothing to do.
__device__ __forceinline__ bool hipk_batch_enter(const hipk_batch_args &a, hipk_batch_rec *rec, const hipk_batch_lds &l) {
    const int t = threadIdx.x;
    if (t == 0) {
        const bool done = a.resume && rec->status == BATCH_DONE;
        if (a.resume && !done) {
            for (int i = 0; i < BS_ND; ++i) l.sd[i] = rec->sd[i];
            for (int i = 0; i < BI_NI; ++i) l.si[i] = rec->si[i];
        }
        if (!a.resume) {
            for (int i = 0; i < BS_ND; ++i) l.sd[i] = 0.0;
            for (int i = 0; i < BI_NI; ++i) l.si[i] = 0;
            rec->launches = 0;
        }
        l.si[BI_ITS] = 0;
        l.si[BI_GO] = done ? 0 : GO_ITERATE;
    }
    __syncthreads();
    return l.si[BI_GO] != 0;
}

// thread 0, when the budget of this launch is used up: the scalar block goes to the record
__device__ __forceinline__ void hipk_batch_save(const hipk_batch_args &a, hipk_batch_rec *rec, const hipk_batch_lds &l) {
    for (int i = 0; i < BS_ND; ++i) rec->sd[i] = l.sd[i];
    for (int i = 0; i < BI_NI; ++i) rec->si[i] = l.si[i];
    rec->status = BATCH_RUNNING;
    rec->launches += 1;
    atomicAdd(a.unfinished, 1);
}

// ---- block-Jacobi (hipk_batch_bj.hip): the launch's argument block, and one row of the apply
struct hipk_bjbatch_args {
    hipk_batch_args a;
    const void *binv;   // system s: binv + s * ldbinv, ceil(n / bs) blocks of bs x bs, row-major per block
    int64_t ldbinv;
    int bs;
};

// z_i of z = blockdiag(binv) v, the expression of hipk_block_jacobi_kernel (orc_block_jacobi_apply): the fma chain over the block's
// columns in ascending order.  `in` must be complete (LDS, behind a barrier): a block's columns belong to other threads.  Rows of a
// block are not 16-byte aligned in general (bs = 3), so binv is read element by element.
template <typename T>
__device__ __forceinline__ T hipk_bbj_row(const T *__restrict__ binv, const T *in, int i, int n, int bs) {
    const int b0 = (i / bs) * bs;
    const T *__restrict__ row = binv + (size_t)i * bs;   // block b, local row i - b0: (b * bs + (i - b0)) * bs = i * bs
    const int cols = (n - b0 < bs) ? n - b0 : bs;
    T acc = (T)0;
    // eight columns at a time: their loads are issued together, so a lane takes the 64 bytes (fp64) of its row while the cache
    // line is there (lanes are bs elements apart: one load per column left every line to be fetched again for the next column).
    // The chain itself is unchanged: a column that does not exist adds no link (fma(0, 0, -0.0) would turn the sign).
    for (int j0 = 0; j0 < cols; j0 += 8) {
        T a[8], v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const bool ok = j0 + u < cols;
            a[u] = ok ? row[j0 + u] : (T)0;
            v[u] = ok ? in[b0 + j0 + u] : (T)0;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (j0 + u < cols) acc = fma(a[u], v[u], acc);
        }
    }
    return acc;
}

// ---------------------------------------------------------------------------------------------------------------- host
// what hipk_last_batch_launches() reports for the calling thread (hipk_batch.hip)
void hipk_batch_note_launches(int launches);

// the argument checks of a batch entry point; `need`: its work bytes.  Nothing is written before the arguments are known to be good.
static int hipk_batch_check(int dtype, int64_t n, int64_t nnz, const int32_t *crow, const int32_t *col, const void *vals, int64_t ldv,
                            const void *dinv, int64_t ldd, int batch, const void *B, int64_t ldb, void *X, int64_t ldx, void *work,
                            size_t work_bytes, size_t need, const hipk_params *prm, hipk_stats *st, hipStream_t s) {
    HIPK_REQUIRE(crow && col && vals && B && X && work && prm && st, HIPK_ERR_ARG, "null argument");
    HIPK_REQUIRE(dtype == HIPK_F64 || dtype == HIPK_F32, HIPK_ERR_ARG, "dtype must be HIPK_F32 or HIPK_F64");
    HIPK_REQUIRE(n >= 1 && nnz >= 0 && batch >= 1, HIPK_ERR_ARG, "n and batch must be at least 1");
    HIPK_REQUIRE(n <= HIPK_BATCH_MAX_N, HIPK_ERR_UNSUPPORTED, "the batch kernels take systems of at most 4096 rows");
    HIPK_REQUIRE(ldv >= nnz && ldb >= n && ldx >= n && (!dinv || ldd >= n), HIPK_ERR_ARG, "a leading dimension is shorter than its row");
    HIPK_REQUIRE(B != X, HIPK_ERR_ARG, "B and X must not alias");
    const size_t sv = dtype == HIPK_F64 ? 8 : 4;
    HIPK_REQUIRE(hipk_aligned16(vals) && hipk_aligned16(B) && hipk_aligned16(X) && hipk_aligned16(dinv), HIPK_ERR_ALIGN,
                 "vals, B, X and dinv must be 16-byte aligned");
    HIPK_REQUIRE((ldv * sv) % 16 == 0 && (ldb * sv) % 16 == 0 && (ldx * sv) % 16 == 0 && (!dinv || (ldd * sv) % 16 == 0), HIPK_ERR_ALIGN,
                 "every row of vals, B, X and dinv must start 16-byte aligned (ld * sizeof(T) a multiple of 16)");
    HIPK_REQUIRE((((uintptr_t)work) & 255u) == 0, HIPK_ERR_ALIGN, "work must be 256-byte aligned");
    HIPK_REQUIRE(work_bytes >= need, HIPK_ERR_WORKSPACE, "work too small");
    // the row bound of the envelope, from the pattern, on the host
    std::vector<int32_t> hc((size_t)n + 1);
    HIPK_CHECK_HIP(hipMemcpyAsync(hc.data(), crow, hc.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPK_CHECK_HIP(hipStreamSynchronize(s));
    bool bad = hc[0] < 0 || (int64_t)hc[n] > nnz, longrow = false;
    for (int64_t i = 0; i < n; ++i) {
        bad = bad || hc[i + 1] < hc[i];
        longrow = longrow || hc[i + 1] - hc[i] > HIPK_BATCH_MAX_ROW;
    }
    HIPK_REQUIRE(!bad, HIPK_ERR_ARG, "crow is not a row pointer array of at most nnz entries");
    HIPK_REQUIRE(!longrow, HIPK_ERR_UNSUPPORTED, "the batch kernels take rows of at most 32 stored entries");
    return HIPK_OK;
}

// the argument block of a launch; work = head | records | slabs of `nvec` vectors per system
static void hipk_batch_fill(hipk_batch_args &a, int dtype, int64_t n, const int32_t *crow, const int32_t *col, const void *vals, int64_t ldv,
                            const void *dinv, int64_t ldd, int batch, const void *B, int64_t ldb, void *X, int64_t ldx, void *work, int nvec,
                            const hipk_params *prm) {
    const size_t sv = dtype == HIPK_F64 ? 8 : 4;
    char *w = (char *)work;
    memset(&a, 0, sizeof(a));
    const hipk_geom gm = hipk_make_geom(n);
    a.n = (int)n;
    a.g = gm.g;
    a.ntile = (int)((n + HIPK_THREADS - 1) / HIPK_THREADS);
    a.crow = crow;
    a.col = col;
    a.vals = vals;
    a.dinv = dinv;
    a.B = B;
    a.X = X;
    a.ldv = ldv;
    a.ldd = ldd;
    a.ldb = ldb;
    a.ldx = ldx;
    a.vec_bytes = hipk_align_up((size_t)n * sv, 256);
    a.slab_bytes = (size_t)nvec * a.vec_bytes;
    a.recs = w + HIPK_BATCH_HEAD;
    a.slabs = a.recs + (size_t)batch * HIPK_BATCH_REC;
    a.unfinished = (int *)w;
    const hipk_tol_sq tq(prm);
    a.tol2 = tq.tol2;
    a.atol_sq = tq.atol_sq;
    a.tol_f = (double)(float)prm->tol;
    a.atol_f = (double)(float)prm->atol;
    a.maxiter = hipk_default_maxiter(prm, n);
    a.budget = hipk_sw_int("HIPK_BATCH_LAUNCH_ITS", 16384, 1);
    a.nvp = (int)((n + 3) & ~(int64_t)3);
}

// launches until no system is unfinished (launch() reads a.resume), then copies the records' stats out
template <typename F>
static int hipk_batch_drive(hipk_batch_args &a, int batch, hipk_stats *st, hipStream_t s, F launch) {
    int *head = a.unfinished;
    HIPK_CHECK_HIP(hipMemsetAsync(head, 0, HIPK_BATCH_HEAD, s));
    hipk_event_pair whole;
    HIPK_CHECK_HIP(whole.create());
    HIPK_CHECK_HIP(hipEventRecord(whole.a, s));
    int launches = 0, unfinished = 0;
    do {
        a.resume = launches > 0;
        if (launches > 0) HIPK_CHECK_HIP(hipMemsetAsync(head, 0, sizeof(int), s));
        const int rc = launch();
        if (rc != HIPK_OK) return rc;
        ++launches;
        HIPK_CHECK_HIP(hipMemcpyAsync(&unfinished, head, sizeof(int), hipMemcpyDeviceToHost, s));
        HIPK_CHECK_HIP(hipStreamSynchronize(s));
    } while (unfinished > 0);
    HIPK_CHECK_HIP(hipEventRecord(whole.b, s));
    std::vector<unsigned char> host((size_t)batch * HIPK_BATCH_REC);
    HIPK_CHECK_HIP(hipMemcpyAsync(host.data(), a.recs, host.size(), hipMemcpyDeviceToHost, s));
    HIPK_CHECK_HIP(hipStreamSynchronize(s));
    float ms = 0.f;
    HIPK_CHECK_HIP(hipEventElapsedTime(&ms, whole.a, whole.b));
    for (int i = 0; i < batch; ++i) {
        const hipk_batch_rec *h = (const hipk_batch_rec *)(host.data() + (size_t)i * HIPK_BATCH_REC);
        hipk_stats *o = st + i;
        memset(o, 0, sizeof(*o));
        o->iterations = h->iterations;
        o->matvecs = h->matvecs;
        o->info = h->info;
        o->breakdown = h->breakdown;
        o->b_norm = h->b_norm;
        o->residual_norm = h->residual_norm;
        o->x_norm = h->x_norm;
        o->threshold = h->threshold;
        o->recurrence_rs = h->recurrence_rs;
        o->solve_ms = ms;
    }
    hipk_batch_note_launches(launches);
    return HIPK_OK;
}
