// hipk_batch.hip -- cg_batch / bicgstab_batch: S independent small systems with ONE sparsity pattern, one workgroup per system.
//
// hipk_cg_batch_kernel<T, PRE> and hipk_bi_batch_kernel<T, PRE> run the whole solve of system s = blockIdx.x in one 256-thread
// workgroup: initial residual, loop, true residual, info.  No workgroup reads anything another workgroup of the launch writes
// (the one exception is an atomic count of unfinished systems that only the host reads), so there is no flag, no grid barrier and
// no spin in this file.  The arithmetic is oracle/krylov_oracle.c per system, bit for bit (DESIGN.md 7c says which dot is which).
//
// Envelope: 1 <= n <= 4096 (at most two reduction chunks of 2048), every row at most 32 stored entries (the straight-order row sum).
//
// Layout.  Dynamic LDS: the reduction buffers, the scalar block, the gather operand(s) of the SpMV (CG: p; BiCGStab: phat and shat,
// which ARE p and s without a preconditioner) and the SpMV's output.  The other vectors live in the system's slab of `work` and are
// read and written in the virtual-thread layout of the plain dot (thread t owns elements VEC t .. VEC t + VEC - 1 of every block of
// 256 VEC elements, 16-byte accesses), x in the caller's X.  Matrix values stream from memory every iteration.
//
// Scalars and decisions.  Thread 0 alone forms every scalar of the recurrence and every decision (stop test, breakdown tests,
// exit_early, launch budget) and stores them to the LDS scalar block; after a barrier all threads read the SAME words, so every
// barrier of the kernel is reached by all 256 threads or by none.
//
// Bounded launches.  A launch runs at most `budget` iterations per system (HIPK_BATCH_LAUNCH_ITS).  A system that has not finished
// then stores its LDS-resident vector and its scalar block to its record and slab and counts itself in `unfinished`; the next launch
// resumes it from exactly that state (a finished system's workgroup returns at once), so the bits do not depend on the budget.
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
static inline size_t hipk_batch_lds_bytes(int n, size_t sv, int solver) {
    const size_t nvp = ((size_t)n + 3) & ~(size_t)3;
    return HIPK_BATCH_LDS_FIXED + (size_t)(solver == 0 ? 2 : 3) * nvp * sv;
}
static inline int hipk_batch_nvec(int solver, int precond) { return solver == 0 ? 2 : (precond ? 5 : 4); }

extern "C" size_t hipk_batch_work_bytes(int64_t n, int64_t nnz, int batch, int dtype, int solver, int precond) {
    (void)nnz;
    const size_t sv = (dtype == HIPK_F64) ? 8 : 4;
    const size_t vec = hipk_align_up((size_t)(n > 0 ? n : 1) * sv, 256);
    const size_t s = (size_t)(batch > 0 ? batch : 1);
    return HIPK_BATCH_HEAD + s * HIPK_BATCH_REC + s * (size_t)hipk_batch_nvec(solver ? 1 : 0, precond ? 1 : 0) * vec;
}

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

// ---------------------------------------------------------------------------------------------------------------- CG / Jacobi PCG
// orc_cg / orc_pcg_jacobi.  Slab: r | p (saved between launches only).  LDS vectors: p (x while a residual is formed) | Ap.
template <typename T, bool PRE>
__global__ __launch_bounds__(HIPK_THREADS) HIPK_SGPR80 void hipk_cg_batch_kernel(hipk_batch_args a) {
    constexpr int VEC = hipk_vec<T>::VEC;
    extern __shared__ __align__(16) unsigned char hipk_batch_raw[];
    const hipk_batch_lds l = hipk_batch_carve(hipk_batch_raw);
    const int t = threadIdx.x, n = a.n, g = a.g;
    const size_t s = blockIdx.x;
    hipk_batch_rec *rec = (hipk_batch_rec *)(a.recs + s * HIPK_BATCH_REC);
    T *pl = (T *)l.vec, *yl = pl + a.nvp;
    T *r = (T *)(a.slabs + s * a.slab_bytes), *psave = (T *)((char *)r + a.vec_bytes);
    const T *vals = (const T *)a.vals + s * a.ldv, *b = (const T *)a.B + s * a.ldb;
    const T *dinv = PRE ? (const T *)a.dinv + s * a.ldd : nullptr;
    T *x = (T *)a.X + s * a.ldx;
    double *sd = l.sd;
    int64_t *si = l.si;

    if (!hipk_batch_enter(a, rec, l)) return;

    // thread 0: the loop condition of orc_cg at the top of iteration k, and this launch's budget
    auto decide = [&]() {
        const bool stop = si[BI_K] >= a.maxiter || sd[BS_RS] <= sd[BS_ATOL2];
        si[BI_GO] = stop ? GO_FINISH : (si[BI_ITS] >= a.budget ? GO_SAVE : GO_ITERATE);
    };

    if (!a.resume) {
        // <b,b> (plain) while x0 moves to LDS; r0 = b - A x0 with the tiled <r0,r0>
        double acc[2] = {0.0, 0.0};
        HIPK_B_FOR_OWN(T, c, base) {
            T bv[VEC], xv[VEC];
            hipk_bld(b, base, n, bv);
            hipk_bld(x, base, n, xv);
#pragma unroll
            for (int e = 0; e < VEC; ++e)
                if (base + e < n) acc[c] = fma((double)bv[e], (double)bv[e], acc[c]);
            hipk_bst(pl, base, n, xv);
        }
        hipk_bsums_t0<2>(acc, l.red);   // (its barrier also completes x in LDS)
        if (t == 0) sd[BS_BS] = hipk_bfold2(acc[0], acc[1], g);
        hipk_bspmv<T, 1>(a, vals, pl, l.sw, [&](int row, T sum, double(&pr)[1]) {
            const T rv = b[row] - sum;
            r[row] = rv;
            pr[0] = (double)rv * (double)rv;
        });
        __syncthreads();
        if (t == 0) {
            const double bs = sd[BS_BS];
            const double a2 = a.tol2 * bs;
            sd[BS_ATOL2] = a2 > a.atol_sq ? a2 : a.atol_sq;
            sd[BS_RS] = hipk_btiled_t0(l.sw, a.ntile, g);
            sd[BS_GAMMA] = sd[BS_RS];
            si[BI_MATVECS] = 1;
        }
        // p = r0 (PRE: z0 = dinv r0, gamma = <r0, z0> plain)
        double az[2] = {0.0, 0.0};
        HIPK_B_FOR_OWN(T, c, base) {
            T rv[VEC];
            hipk_bld(r, base, n, rv);
            if (PRE) {
                T dv[VEC];
                hipk_bld(dinv, base, n, dv);
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    const T z = dv[e] * rv[e];
                    if (base + e < n) az[c] = fma((double)rv[e], (double)z, az[c]);
                    rv[e] = z;
                }
            }
            hipk_bst(pl, base, n, rv);
        }
        if (PRE) {
            hipk_bsums_t0<2>(az, l.red);
            if (t == 0) sd[BS_GAMMA] = hipk_bfold2(az[0], az[1], g);
        }
        if (t == 0) decide();
        __syncthreads();
    } else {
        HIPK_B_FOR_OWN(T, c, base) {
            T pv[VEC];
            hipk_bld(psave, base, n, pv);
            hipk_bst(pl, base, n, pv);
        }
        if (t == 0) decide();
        __syncthreads();
    }

    while (si[BI_GO] == GO_ITERATE) {
        // Ap, <p,Ap> tiled
        hipk_bspmv<T, 1>(a, vals, pl, l.sw, [&](int row, T sum, double(&pr)[1]) {
            yl[row] = sum;
            pr[0] = (double)pl[row] * (double)sum;
        });
        __syncthreads();
        if (t == 0) {
            const double pAp = hipk_btiled_t0(l.sw, a.ntile, g);
            sd[BS_ALPHA] = sd[BS_GAMMA] / pAp;
            si[BI_MATVECS] += 1;
        }
        __syncthreads();
        // x += alpha p, r -= alpha Ap, <r,r> (PRE: and <r, dinv r>) plain
        const T alpha = (T)sd[BS_ALPHA];
        double acc[PRE ? 4 : 2];
#pragma unroll
        for (int k = 0; k < (PRE ? 4 : 2); ++k) acc[k] = 0.0;
        HIPK_B_FOR_OWN(T, c, base) {
            T rv[VEC], xv[VEC], pv[VEC], yv[VEC], dv[VEC];
            hipk_bld(r, base, n, rv);
            hipk_bld(x, base, n, xv);
            hipk_bld(pl, base, n, pv);
            hipk_bld(yl, base, n, yv);
            if (PRE) hipk_bld(dinv, base, n, dv);
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const T m0 = alpha * pv[e];
                xv[e] = xv[e] + m0;
                const T m1 = alpha * yv[e];
                rv[e] = rv[e] - m1;
                if (base + e < n) {
                    acc[c] = fma((double)rv[e], (double)rv[e], acc[c]);
                    if (PRE) {
                        const T z = dv[e] * rv[e];
                        acc[2 + c] = fma((double)rv[e], (double)z, acc[2 + c]);
                    }
                }
            }
            hipk_bst(r, base, n, rv);
            hipk_bst(x, base, n, xv);
        }
        hipk_bsums_t0<(PRE ? 4 : 2)>(acc, l.red);
        if (t == 0) {
            const double rr = hipk_bfold2(acc[0], acc[1], g);
            const double num = PRE ? hipk_bfold2(acc[PRE ? 2 : 0], acc[PRE ? 3 : 1], g) : rr;
            sd[BS_BETA] = num / sd[BS_GAMMA];
            sd[BS_GAMMA] = num;
            sd[BS_RS] = rr;
            si[BI_K] += 1;
            si[BI_ITS] += 1;
            decide();
        }
        __syncthreads();
        // p = r + beta p (PRE: z + beta p)
        const T beta = (T)sd[BS_BETA];
        HIPK_B_FOR_OWN(T, c, base) {
            T rv[VEC], pv[VEC];
            hipk_bld(r, base, n, rv);
            hipk_bld(pl, base, n, pv);
            if (PRE) {
                T dv[VEC];
                hipk_bld(dinv, base, n, dv);
#pragma unroll
                for (int e = 0; e < VEC; ++e) rv[e] = dv[e] * rv[e];
            }
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const T m = beta * pv[e];
                pv[e] = rv[e] + m;
            }
            hipk_bst(pl, base, n, pv);
        }
        __syncthreads();
    }

    if (si[BI_GO] == GO_SAVE) {
        HIPK_B_FOR_OWN(T, c, base) {
            T pv[VEC];
            hipk_bld(pl, base, n, pv);
            hipk_bst(psave, base, n, pv);
        }
        if (t == 0) hipk_batch_save(a, rec, l);
        return;
    }

    // TSL:1007-1016: b - A x (PRE: ||M (b - A x)|| as a plain dot of the scaled residual), <x,x> plain
    double ax[4] = {0.0, 0.0, 0.0, 0.0};
    HIPK_B_FOR_OWN(T, c, base) {
        T xv[VEC];
        hipk_bld(x, base, n, xv);
#pragma unroll
        for (int e = 0; e < VEC; ++e)
            if (base + e < n) ax[c] = fma((double)xv[e], (double)xv[e], ax[c]);
        hipk_bst(pl, base, n, xv);
    }
    __syncthreads();
    hipk_bspmv<T, 1>(a, vals, pl, l.sw, [&](int row, T sum, double(&pr)[1]) {
        const T rv = b[row] - sum;
        if (PRE) yl[row] = rv;
        pr[0] = (double)rv * (double)rv;
    });
    __syncthreads();
    if (PRE) {
        HIPK_B_FOR_OWN(T, c, base) {
            T yv[VEC], dv[VEC];
            hipk_bld(yl, base, n, yv);
            hipk_bld(dinv, base, n, dv);
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const T m = dv[e] * yv[e];
                if (base + e < n) ax[2 + c] = fma((double)m, (double)m, ax[2 + c]);
            }
        }
    }
    hipk_bsums_t0<4>(ax, l.red);
    if (t == 0) {
        sd[BS_XX] = hipk_bfold2(ax[0], ax[1], g);
        sd[BS_RES2] = PRE ? hipk_bfold2(ax[2], ax[3], g) : hipk_btiled_t0(l.sw, a.ntile, g);
        si[BI_MATVECS] += 1;
        hipk_bfinish(rec, a, sd, si);
    }
}

// ---------------------------------------------------------------------------------------------------------------- BiCGStab
// bicgstab_impl with and without dinv.  Slab: r | rhat | q | p (PRE: always; else saved between launches only) | s (PRE).
// LDS vectors: ga = phat (p without PRE; x while a residual is formed) | gb = shat (s without PRE) | yl = q, then t.
template <typename T, bool PRE>
__global__ __launch_bounds__(HIPK_THREADS) HIPK_SGPR80 void hipk_bi_batch_kernel(hipk_batch_args a) {
    constexpr int VEC = hipk_vec<T>::VEC;
    constexpr double EPS = hipk_beps<T>::v;
    extern __shared__ __align__(16) unsigned char hipk_batch_raw[];
    const hipk_batch_lds l = hipk_batch_carve(hipk_batch_raw);
    const int t = threadIdx.x, n = a.n, g = a.g;
    const size_t s = blockIdx.x;
    hipk_batch_rec *rec = (hipk_batch_rec *)(a.recs + s * HIPK_BATCH_REC);
    T *ga = (T *)l.vec, *gb = ga + a.nvp, *yl = gb + a.nvp;
    char *slab = a.slabs + s * a.slab_bytes;
    T *r = (T *)slab, *rhat = (T *)(slab + a.vec_bytes), *q = (T *)(slab + 2 * a.vec_bytes), *pg = (T *)(slab + 3 * a.vec_bytes);
    T *sg = PRE ? (T *)(slab + 4 * a.vec_bytes) : nullptr;
    const T *vals = (const T *)a.vals + s * a.ldv, *b = (const T *)a.B + s * a.ldb;
    const T *dinv = PRE ? (const T *)a.dinv + s * a.ldd : nullptr;
    T *x = (T *)a.X + s * a.ldx;
    double *sd = l.sd;
    int64_t *si = l.si;

    if (!hipk_batch_enter(a, rec, l)) return;

    // thread 0: the top of the oracle's loop (TSL:895-906) for iteration k, and this launch's budget.  Nothing it changes is part of
    // the saved state unless the iteration goes ahead (rs is only ever set to rs_next, beta is formed again).
    auto decide = [&]() {
        if (si[BI_K] >= a.maxiter) {
            si[BI_GO] = GO_FINISH;
            return;
        }
        if (si[BI_ITS] >= a.budget && !(sd[BS_RS_NEXT] <= sd[BS_ATOL2]) &&
            !(fabs(sd[BS_RHO_NEXT]) < EPS * fabs(sd[BS_RHO]))) {
            si[BI_GO] = GO_SAVE;
            return;
        }
        sd[BS_RS] = sd[BS_RS_NEXT];
        if (sd[BS_RS] <= sd[BS_ATOL2]) {
            si[BI_GO] = GO_FINISH;
            return;
        }
        const double rho_new = sd[BS_RHO_NEXT];
        if (fabs(rho_new) < EPS * fabs(sd[BS_RHO])) {
            si[BI_CODE] = -10;
            si[BI_GO] = GO_FINISH;
            return;
        }
        sd[BS_RHO_NEW] = rho_new;
        sd[BS_BETA] = rho_new / sd[BS_RHO] * sd[BS_ALPHA] / sd[BS_OMEGA];   // left to right, TSL:906
        si[BI_GO] = GO_ITERATE;
    };

    if (!a.resume) {
        double acc[2] = {0.0, 0.0};
        HIPK_B_FOR_OWN(T, c, base) {
            T bv[VEC], xv[VEC];
            hipk_bld(b, base, n, bv);
            hipk_bld(x, base, n, xv);
#pragma unroll
            for (int e = 0; e < VEC; ++e)
                if (base + e < n) acc[c] = fma((double)bv[e], (double)bv[e], acc[c]);
            hipk_bst(ga, base, n, xv);
        }
        hipk_bsums_t0<2>(acc, l.red);
        if (t == 0) sd[BS_BS] = hipk_bfold2(acc[0], acc[1], g);
        hipk_bspmv<T, 1>(a, vals, ga, l.sw, [&](int row, T sum, double(&pr)[1]) {
            const T rv = b[row] - sum;
            r[row] = rv;
            pr[0] = (double)rv * (double)rv;
        });
        __syncthreads();
        if (t == 0) {
            const double bs = sd[BS_BS];
            const double a2 = a.tol2 * bs;
            sd[BS_ATOL2] = a2 > a.atol_sq ? a2 : a.atol_sq;
            sd[BS_RS_NEXT] = hipk_btiled_t0(l.sw, a.ntile, g);
            sd[BS_RHO_NEXT] = sd[BS_RS_NEXT];
            sd[BS_ALPHA] = sd[BS_OMEGA] = sd[BS_RHO] = 1.0;
            sd[BS_RS] = 0.0;
            si[BI_MATVECS] = 1;
            decide();
        }
        // rhat = p = q = r0
        HIPK_B_FOR_OWN(T, c, base) {
            T rv[VEC];
            hipk_bld(r, base, n, rv);
            hipk_bst(rhat, base, n, rv);
            hipk_bst(q, base, n, rv);
            hipk_bst(PRE ? pg : ga, base, n, rv);
        }
        __syncthreads();
    } else {
        if (!PRE) {
            HIPK_B_FOR_OWN(T, c, base) {
                T pv[VEC];
                hipk_bld(pg, base, n, pv);
                hipk_bst(ga, base, n, pv);
            }
        }
        if (t == 0) decide();
        __syncthreads();
    }

    while (si[BI_GO] == GO_ITERATE) {
        // p = r + beta (p - omega q); phat = dinv p
        {
            const T beta = (T)sd[BS_BETA], omega = (T)sd[BS_OMEGA];
            T *pp = PRE ? pg : ga;
            HIPK_B_FOR_OWN(T, c, base) {
                T rv[VEC], pv[VEC], qv[VEC];
                hipk_bld(r, base, n, rv);
                hipk_bld(pp, base, n, pv);
                hipk_bld(q, base, n, qv);
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    const T t1 = omega * qv[e];
                    const T t2 = pv[e] - t1;
                    const T t3 = beta * t2;
                    pv[e] = rv[e] + t3;
                }
                hipk_bst(pp, base, n, pv);
                if (PRE) {
                    T dv[VEC];
                    hipk_bld(dinv, base, n, dv);
#pragma unroll
                    for (int e = 0; e < VEC; ++e) pv[e] = dv[e] * pv[e];
                    hipk_bst(ga, base, n, pv);
                }
            }
        }
        __syncthreads();
        // q = A phat, <rhat,q> tiled
        hipk_bspmv<T, 1>(a, vals, ga, l.sw, [&](int row, T sum, double(&pr)[1]) {
            yl[row] = sum;
            q[row] = sum;
            pr[0] = (double)rhat[row] * (double)sum;
        });
        __syncthreads();
        if (t == 0) {
            const double alpha_new = sd[BS_RHO_NEW] / hipk_btiled_t0(l.sw, a.ntile, g);
            sd[BS_ALPHA_NEW] = alpha_new;
            si[BI_MATVECS] += 1;
            if (fabs(alpha_new) < EPS) {   // TSL:913-915
                si[BI_CODE] = -11;
                si[BI_GO] = GO_FINISH;
            }
        }
        __syncthreads();
        if (si[BI_GO] != GO_ITERATE) break;
        // s = r - alpha q; shat = dinv s; <s,s> plain
        {
            const T alpha = (T)sd[BS_ALPHA_NEW];
            double acc[2] = {0.0, 0.0};
            HIPK_B_FOR_OWN(T, c, base) {
                T rv[VEC], qv[VEC];
                hipk_bld(r, base, n, rv);
                hipk_bld(yl, base, n, qv);
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    const T m = alpha * qv[e];
                    rv[e] = rv[e] - m;
                    if (base + e < n) acc[c] = fma((double)rv[e], (double)rv[e], acc[c]);
                }
                if (PRE) {
                    T dv[VEC];
                    hipk_bst(sg, base, n, rv);
                    hipk_bld(dinv, base, n, dv);
#pragma unroll
                    for (int e = 0; e < VEC; ++e) rv[e] = dv[e] * rv[e];
                }
                hipk_bst(gb, base, n, rv);
            }
            hipk_bsums_t0<2>(acc, l.red);
            if (t == 0) si[BI_EXIT_EARLY] = hipk_bfold2(acc[0], acc[1], g) < sd[BS_ATOL2] ? 1 : 0;
        }
        __syncthreads();
        // t = A shat, <t,t> and <s,t> tiled
        hipk_bspmv<T, 2>(a, vals, gb, l.sw, [&](int row, T sum, double(&pr)[2]) {
            yl[row] = sum;
            const T sv = PRE ? sg[row] : gb[row];
            pr[0] = (double)sum * (double)sum;
            pr[1] = (double)sv * (double)sum;
        });
        __syncthreads();
        if (t == 0) {
            const double tt = hipk_btiled_t0(l.sw, a.ntile, g);
            const double ts = hipk_btiled_t0(l.sw + 64, a.ntile, g);
            const double omega_new = (fabs(tt) < EPS) ? 0.0 : ts / tt;   // TSL:926-930
            sd[BS_OMEGA_NEW] = omega_new;
            si[BI_MATVECS] += 1;
            if (fabs(omega_new) < EPS && !si[BI_EXIT_EARLY]) {   // TSL:934-936
                si[BI_CODE] = -11;
                si[BI_GO] = GO_FINISH;
            }
        }
        __syncthreads();
        if (si[BI_GO] != GO_ITERATE) break;
        // x += alpha phat + omega shat, r = s - omega t (exit_early: x += alpha phat, r = s); <r,r>, <rhat,r> plain
        {
            const T alpha = (T)sd[BS_ALPHA_NEW], omega = (T)sd[BS_OMEGA_NEW];
            const bool early = si[BI_EXIT_EARLY] != 0;
            double acc[4] = {0.0, 0.0, 0.0, 0.0};
            HIPK_B_FOR_OWN(T, c, base) {
                T xv[VEC], ph[VEC], sh[VEC], sv[VEC], tv[VEC], hv[VEC];
                hipk_bld(x, base, n, xv);
                hipk_bld(ga, base, n, ph);
                hipk_bld(gb, base, n, sh);
                if (PRE)
                    hipk_bld(sg, base, n, sv);
                else {
#pragma unroll
                    for (int e = 0; e < VEC; ++e) sv[e] = sh[e];
                }
                hipk_bld(yl, base, n, tv);
                hipk_bld(rhat, base, n, hv);
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    const T m0 = alpha * ph[e];
                    if (early) {
                        xv[e] = xv[e] + m0;
                    } else {
                        const T m1 = omega * sh[e];
                        const T m2 = m0 + m1;
                        xv[e] = xv[e] + m2;
                        const T m3 = omega * tv[e];
                        sv[e] = sv[e] - m3;
                    }
                    if (base + e < n) {
                        acc[c] = fma((double)sv[e], (double)sv[e], acc[c]);
                        acc[2 + c] = fma((double)hv[e], (double)sv[e], acc[2 + c]);
                    }
                }
                hipk_bst(x, base, n, xv);
                hipk_bst(r, base, n, sv);
            }
            hipk_bsums_t0<4>(acc, l.red);
            if (t == 0) {
                sd[BS_RS_NEXT] = hipk_bfold2(acc[0], acc[1], g);
                sd[BS_RHO_NEXT] = hipk_bfold2(acc[2], acc[3], g);
                sd[BS_RHO] = sd[BS_RHO_NEW];
                sd[BS_ALPHA] = sd[BS_ALPHA_NEW];
                sd[BS_OMEGA] = sd[BS_OMEGA_NEW];
                si[BI_K] += 1;
                si[BI_ITS] += 1;
                if (early)
                    si[BI_GO] = GO_FINISH;
                else
                    decide();
            }
        }
        __syncthreads();
    }

    if (si[BI_GO] == GO_SAVE) {
        if (!PRE) {
            HIPK_B_FOR_OWN(T, c, base) {
                T pv[VEC];
                hipk_bld(ga, base, n, pv);
                hipk_bst(pg, base, n, pv);
            }
        }
        if (t == 0) hipk_batch_save(a, rec, l);
        return;
    }

    // TSL:1007-1016: b - A x, row-scaled by dinv after the product (PRE), its tiled square; <x,x> plain
    double ax[2] = {0.0, 0.0};
    HIPK_B_FOR_OWN(T, c, base) {
        T xv[VEC];
        hipk_bld(x, base, n, xv);
#pragma unroll
        for (int e = 0; e < VEC; ++e)
            if (base + e < n) ax[c] = fma((double)xv[e], (double)xv[e], ax[c]);
        hipk_bst(ga, base, n, xv);
    }
    hipk_bsums_t0<2>(ax, l.red);
    if (t == 0) sd[BS_XX] = hipk_bfold2(ax[0], ax[1], g);
    hipk_bspmv<T, 1>(a, vals, ga, l.sw, [&](int row, T sum, double(&pr)[1]) {
        T rv = b[row] - sum;
        if (PRE) rv = dinv[row] * rv;
        pr[0] = (double)rv * (double)rv;
    });
    __syncthreads();
    if (t == 0) {
        sd[BS_RES2] = hipk_btiled_t0(l.sw, a.ntile, g);
        si[BI_MATVECS] += 1;
        hipk_bfinish(rec, a, sd, si);
    }
}

// ---------------------------------------------------------------------------------------------------------------- host
static thread_local int g_batch_launches = 0;
extern "C" int hipk_last_batch_launches(void) { return g_batch_launches; }

template <typename T, bool PRE>
static int hipk_batch_launch(int solver, const hipk_batch_args &a, int batch, size_t lds, hipStream_t s) {
    void (*kern)(hipk_batch_args) = solver == 0 ? hipk_cg_batch_kernel<T, PRE> : hipk_bi_batch_kernel<T, PRE>;
    if (lds > 64 * 1024)   // beyond the default limit of dynamic LDS; per launch: the attribute belongs to the current device
        HIPK_CHECK_HIP(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    kern<<<(unsigned)batch, HIPK_THREADS, lds, s>>>(a);
    HIPK_CHECK_HIP(hipGetLastError());
    return HIPK_OK;
}

static const char *hipk_batch_name(int solver, int dtype, bool pre) {
    static const char *names[2][2][2] = {
        {{"hipk_cg_batch_kernel<float,false>", "hipk_cg_batch_kernel<float,true>"},
         {"hipk_cg_batch_kernel<double,false>", "hipk_cg_batch_kernel<double,true>"}},
        {{"hipk_bi_batch_kernel<float,false>", "hipk_bi_batch_kernel<float,true>"},
         {"hipk_bi_batch_kernel<double,false>", "hipk_bi_batch_kernel<double,true>"}}};
    return names[solver][dtype == HIPK_F64][pre];
}

static int hipk_solve_batch(int solver, int dtype, int64_t n, int64_t nnz, const int32_t *crow, const int32_t *col, const void *vals,
                            int64_t ldv, const void *dinv, int64_t ldd, int batch, const void *B, int64_t ldb, void *X, int64_t ldx,
                            void *work, size_t work_bytes, const hipk_params *prm, hipk_stats *st, hipk_stream_t stream) {
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
    const bool pre = dinv != nullptr;
    const size_t need = hipk_batch_work_bytes(n, nnz, batch, dtype, solver, pre);
    HIPK_REQUIRE(work_bytes >= need, HIPK_ERR_WORKSPACE, "work too small");
    hipStream_t s = (hipStream_t)stream;
    char *w = (char *)work;
    int *head = (int *)w;

    // the row bound of the envelope, from the pattern, on the host: nothing is written before the arguments are known to be good
    {
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
    }
    HIPK_CHECK_HIP(hipMemsetAsync(head, 0, HIPK_BATCH_HEAD, s));

    hipk_batch_args a;
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
    a.slab_bytes = (size_t)hipk_batch_nvec(solver, pre) * a.vec_bytes;
    a.recs = w + HIPK_BATCH_HEAD;
    a.slabs = a.recs + (size_t)batch * HIPK_BATCH_REC;
    a.unfinished = head;
    const hipk_tol_sq tq(prm);
    a.tol2 = tq.tol2;
    a.atol_sq = tq.atol_sq;
    a.tol_f = (double)(float)prm->tol;
    a.atol_f = (double)(float)prm->atol;
    a.maxiter = hipk_default_maxiter(prm, n);
    a.budget = hipk_sw_int("HIPK_BATCH_LAUNCH_ITS", 16384, 1);
    a.nvp = (int)((n + 3) & ~(int64_t)3);
    const size_t lds = hipk_batch_lds_bytes((int)n, sv, solver);

    hipk_set_solve_path(nullptr, hipk_batch_name(solver, dtype, pre));
    hipk_event_pair whole;
    HIPK_CHECK_HIP(whole.create());
    HIPK_CHECK_HIP(hipEventRecord(whole.a, s));
    int launches = 0, unfinished = 0;
    do {
        a.resume = launches > 0;
        if (launches > 0) HIPK_CHECK_HIP(hipMemsetAsync(head, 0, sizeof(int), s));
        int rc;
        if (dtype == HIPK_F64)
            rc = pre ? hipk_batch_launch<double, true>(solver, a, batch, lds, s) : hipk_batch_launch<double, false>(solver, a, batch, lds, s);
        else
            rc = pre ? hipk_batch_launch<float, true>(solver, a, batch, lds, s) : hipk_batch_launch<float, false>(solver, a, batch, lds, s);
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
    g_batch_launches = launches;
    return HIPK_OK;
}

extern "C" int hipk_cg_solve_batch(int64_t n, int64_t nnz, const int32_t *crow_dev, const int32_t *col_dev, const void *vals, int64_t ldv,
                                   const void *dinv, int64_t ldd, int batch, const void *B, int64_t ldb, void *X, int64_t ldx, int dtype,
                                   void *work, size_t work_bytes, const hipk_params *prm, hipk_stats *st, hipk_stream_t stream) {
    return hipk_solve_batch(0, dtype, n, nnz, crow_dev, col_dev, vals, ldv, dinv, ldd, batch, B, ldb, X, ldx, work, work_bytes, prm, st,
                            stream);
}

extern "C" int hipk_bicgstab_solve_batch(int64_t n, int64_t nnz, const int32_t *crow_dev, const int32_t *col_dev, const void *vals,
                                         int64_t ldv, const void *dinv, int64_t ldd, int batch, const void *B, int64_t ldb, void *X,
                                         int64_t ldx, int dtype, void *work, size_t work_bytes, const hipk_params *prm, hipk_stats *st,
                                         hipk_stream_t stream) {
    return hipk_solve_batch(1, dtype, n, nnz, crow_dev, col_dev, vals, ldv, dinv, ldd, batch, B, ldb, X, ldx, work, work_bytes, prm, st,
                            stream);
}
