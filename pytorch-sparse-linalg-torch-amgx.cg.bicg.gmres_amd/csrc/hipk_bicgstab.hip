// hipk_bicgstab.hip -- device-resident BiCGStab.
//
// Restates `_isolve(_bicgstab_solve)` (TSL:859-964, 968-1016) for M = identity as five
// kernels per iteration; every scalar test of the reference (convergence TSL:894-896,
// rho breakdown :902-904, alpha breakdown :913-915, early exit :920, omega guard
// :926-930, omega breakdown :934-936) is evaluated on the device, redundantly and
// identically by every workgroup, from the chunk partials of the previous kernel:
//   K1 direction  rs, rho' -> tests; beta; p = r + beta (p - omega q)          32 n bytes
//   K2 spmv+dot   q = A p, <rhat,q>                                           B_spmv + 8 n
//   K3 s-update   alpha' = rho'/<rhat,q> -> test; s = r - alpha' q; <s,s>      24 n
//   K4 spmv+dots  t = A s, <t,s>, <t,t>                                        B_spmv
//   K5 x/r-update omega' -> tests; x += alpha' p (+ omega' s); r = s (- omega' t);
//                 <r,r>, <rhat,r> for the next iteration                       56 n
// = 2 B_spmv + 120 n bytes per iteration.  The full-vector `torch.where` selects of the
// reference (TSL:944, 950) become a wave-uniform branch.
#include <math.h>
#include <stdlib.h>

#include "hipk_blas1.h"
#include "hipk_solve.h"
#include "hipk_spmv.h"
#include "hipk_handoff.h"

#define HIPK_EPS64 2.220446049250313e-16
#define HIPK_EPS32 1.1920928955078125e-07

struct hipk_bi_scal {
    double rho, alpha, omega;  // committed by K5 of the last completed iteration
    double rho_new, alpha_new; // handed from K3 to K5 of the same iteration
    double atol2, bs;
    double rs_last;
    double res2, xx;
    int64_t stop_it;
    int64_t iters;
    int32_t code;      // 0 / -10 / -11  (TSL:903, 914, 935)
    int32_t extra_mv;  // SpMVs run by an iteration that then broke down
    int64_t *host_sig; // pinned host word the loop reports to (hipk_pacer, hipk_solve.h), or null
    // hipk_bi_solve_lds_kernel (small systems: the whole loop in one launch)
    int64_t it_done;   // iterations finished when the launch returned
    int32_t redo;      // < 0: its resident workgroups did not all arrive / were spread over several XCDs (nothing was modified)
    int32_t bar;       // counter barrier of its placement check
    unsigned xcc_mask;
    unsigned pad;
};
static_assert(sizeof(hipk_bi_scal) <= 256, "the scalar block is 256 bytes");

template <typename T>
struct hipk_eps;
template <>
struct hipk_eps<double> {
    static constexpr double v = HIPK_EPS64;
};
template <>
struct hipk_eps<float> {
    static constexpr double v = HIPK_EPS32;
};

#include "hipk_bi_mid.h"   // one-launch loop for mid-size systems (uses hipk_bi_scal, HIPK_EPS64)

template <typename T>
__global__ __launch_bounds__(HIPK_THREADS) void hipk_bi_start_kernel(
    int64_t n, int ch, int g, hipk_bi_scal *__restrict__ scal, const double *__restrict__ part_rr,
    const double *__restrict__ part_bb, double *__restrict__ part_rhr, const T *__restrict__ r, T *__restrict__ rhat,
    T *__restrict__ p, T *__restrict__ q, double tol2, double atol_sq, int64_t maxiter, int64_t *host_sig) {
    __shared__ double sbuf[2 * HIPK_THREADS];
    double rr, bs;
    hipk_reduce_parts2(part_rr, part_bb, g, rr, bs, sbuf);
    const int c = blockIdx.x;
    hipk_chunk_loop<T>(n, ch, c, [&](int64_t i, int nv) {
        T rv[hipk_vec<T>::VEC];
        hipk_ld<T>(r, i, nv, rv);
        hipk_st<T>(rhat, i, nv, rv);  // TSL:876
        hipk_st<T>(p, i, nv, rv);     // TSL:890
        hipk_st<T>(q, i, nv, rv);
    });
    if (threadIdx.x == 0) {
        part_rhr[c] = part_rr[c];  // <rhat, r0> = <r0, r0>
        if (c == 0) {
            const double a2 = tol2 * bs;
            scal->rho = 1.0;
            scal->alpha = 1.0;
            scal->omega = 1.0;
            scal->atol2 = (a2 > atol_sq) ? a2 : atol_sq;
            scal->bs = bs;
            scal->rs_last = 0.0;
            scal->stop_it = (maxiter <= 0) ? 0 : INT64_MAX;
            scal->host_sig = host_sig;
            if (maxiter <= 0) hipk_signal(host_sig, HIPK_SIG_STOP);
            scal->iters = 0;
            scal->code = 0;
            scal->extra_mv = 0;
        }
    }
}

// PRE = true: Jacobi preconditioning, M = diag(dinv) applied BEFORE A (TSL:908, 922): the kernel that forms p also
// stores phat = dinv .* p (the SpMV's input), the one that forms s also stores shat, and x is advanced with phat / shat.
template <typename T, bool PRE>
__global__ __launch_bounds__(HIPK_THREADS) void hipk_bi_direction_kernel(
    int64_t n, int ch, int g, hipk_bi_scal *__restrict__ scal, int64_t it, const double *__restrict__ part_rr,
    const double *__restrict__ part_rhr, const T *__restrict__ r, const T *__restrict__ q, T *__restrict__ p,
    const T *__restrict__ dinv, T *__restrict__ phat) {
    hipk_pre<T, 2> pre;  // r and q travel while the stop word is read and the partials are folded
    pre.issue(n, ch, blockIdx.x, {r, q});
    if (it >= scal->stop_it) return;
    __shared__ double sbuf[2 * HIPK_THREADS];
    double rs, rho_new;
    hipk_reduce_parts2(part_rr, part_rhr, g, rs, rho_new, sbuf);
    const double rho = scal->rho, alpha = scal->alpha, omega = scal->omega;
    const bool lead = (blockIdx.x == 0 && threadIdx.x == 0);
    if (lead) scal->rs_last = rs;
    if (rs <= scal->atol2) {  // TSL:894-896
        if (lead) {
            scal->stop_it = it;
            hipk_signal(scal->host_sig, HIPK_SIG_STOP | it);
        }
        return;
    }
    if (fabs(rho_new) < hipk_eps<T>::v * fabs(rho)) {  // TSL:902-904
        if (lead) {
            scal->stop_it = it;
            scal->code = -10;
            hipk_signal(scal->host_sig, HIPK_SIG_STOP | it);
        }
        return;
    }
    const T beta = (T)(rho_new / rho * alpha / omega);  // TSL:906, left to right
    const T om = (T)omega;
    pre.run([&](int64_t i, int nv, T(&v)[2][hipk_vec<T>::VEC]) {
        constexpr int VEC = hipk_vec<T>::VEC;
        T pv[VEC];
        hipk_ld<T>((const T *)p, i, nv, pv);
#pragma unroll
        for (int k = 0; k < VEC; ++k) {  // TSL:907
            const T t1 = om * v[1][k];
            const T t2 = pv[k] - t1;
            const T t3 = beta * t2;
            pv[k] = v[0][k] + t3;
        }
        hipk_st<T>(p, i, nv, pv);
        if (PRE) {
            T dv[VEC];
            hipk_ld<T>(dinv, i, nv, dv);
#pragma unroll
            for (int k = 0; k < VEC; ++k) dv[k] = dv[k] * pv[k];  // TSL:908
            hipk_st<T>(phat, i, nv, dv);
        }
    });
}

template <typename T, bool PRE, bool SMALL>
__global__ __launch_bounds__(HIPK_THREADS) void hipk_bi_supdate_kernel(
    int64_t n, int ch, int g, hipk_bi_scal *__restrict__ scal, int64_t it, const double *__restrict__ part_rhr,
    const double *__restrict__ part_rq, const T *__restrict__ r, const T *__restrict__ q, T *__restrict__ s,
    double *__restrict__ part_ss, const T *__restrict__ dinv, T *__restrict__ shat, int small_ntiles) {
    hipk_pre<T, 2> pre;
    pre.issue(n, ch, blockIdx.x, {r, q});
    if (it >= scal->stop_it) return;
    __shared__ double sbuf[2 * HIPK_THREADS];
    double rho_new, rq;
    if (SMALL) {  // small systems: <rhat,q> from the SpMV's tile sums, no combine launch (hipk_fold_tiles8); a compile-time
                  // switch: the fold's registers would cost the large-system instantiation its 8 workgroups per CU
        rq = hipk_fold_tiles8(part_rq, small_ntiles, ch / HIPK_TILE, g, sbuf);
        rho_new = hipk_reduce_parts(part_rhr, g, sbuf);
    } else {
        hipk_reduce_parts2(part_rhr, part_rq, g, rho_new, rq, sbuf);
    }
    const double alpha_new = rho_new / rq;  // TSL:910
    const bool lead = (blockIdx.x == 0 && threadIdx.x == 0);
    if (fabs(alpha_new) < hipk_eps<T>::v) {  // TSL:913-915
        if (lead) {
            scal->stop_it = it;
            scal->code = -11;
            scal->extra_mv = 1;
            hipk_signal(scal->host_sig, HIPK_SIG_STOP | it);
        }
        return;
    }
    if (lead) {
        scal->rho_new = rho_new;
        scal->alpha_new = alpha_new;
    }
    const T al = (T)alpha_new;
    double acc = 0.0;
    pre.run([&](int64_t i, int nv, T(&v)[2][hipk_vec<T>::VEC]) {
        constexpr int VEC = hipk_vec<T>::VEC;
        T sv[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const T m = al * v[1][k];
            sv[k] = v[0][k] - m;  // TSL:917
            if (k < nv) acc = fma((double)sv[k], (double)sv[k], acc);
        }
        hipk_st<T>(s, i, nv, sv);
        if (PRE) {
            T dv[VEC];
            hipk_ld<T>(dinv, i, nv, dv);
#pragma unroll
            for (int k = 0; k < VEC; ++k) dv[k] = dv[k] * sv[k];  // TSL:922
            hipk_st<T>(shat, i, nv, dv);
        }
    });
    acc = hipk_block_sum(acc, sbuf);
    if (threadIdx.x == 0) part_ss[blockIdx.x] = acc;
}

template <typename T, bool PRE, bool SMALL>
__global__ __launch_bounds__(HIPK_THREADS) void hipk_bi_xupdate_kernel(
    int64_t n, int ch, int g, hipk_bi_scal *__restrict__ scal, int64_t it, int64_t maxiter,
    const double *__restrict__ part_ss, const double *__restrict__ part_ts, const double *__restrict__ part_tt,
    const T *__restrict__ p, const T *__restrict__ s, const T *__restrict__ t, const T *__restrict__ rhat,
    T *__restrict__ x, T *__restrict__ r, double *__restrict__ part_rr, double *__restrict__ part_rhr,
    const T *__restrict__ shat, int small_ntiles) {  // PRE: `p` is phat here; shat = M s
    hipk_pre<T, 1> pre;  // s up front; p, x, rhat, t follow after the fold (two early operands already cost the
    pre.issue(n, ch, blockIdx.x, {s});  // kernel its 8 workgroups per CU: 71 VGPRs)
    if (it >= scal->stop_it) return;
    __shared__ double sbuf[2 * HIPK_THREADS];
    const double ss = hipk_reduce_parts(part_ss, g, sbuf);
    double ts, tt;
    if (SMALL) {  // part_ts / part_tt point at the two tile-sum arrays of the second SpMV
        ts = hipk_fold_tiles8(part_ts, small_ntiles, ch / HIPK_TILE, g, sbuf);
        tt = hipk_fold_tiles8(part_tt, small_ntiles, ch / HIPK_TILE, g, sbuf);
    } else {
        hipk_reduce_parts2(part_ts, part_tt, g, ts, tt, sbuf);
    }
    const double atol2 = scal->atol2;
    const double alpha_new = scal->alpha_new, rho_new = scal->rho_new;
    const bool exit_early = ss < atol2;                                      // TSL:920 (strict)
    const double omega_new = (fabs(tt) < hipk_eps<T>::v) ? 0.0 : ts / tt;    // TSL:926-930
    const bool lead = (blockIdx.x == 0 && threadIdx.x == 0);
    if (fabs(omega_new) < hipk_eps<T>::v && !exit_early) {                   // TSL:934-936
        if (lead) {
            scal->stop_it = it;
            scal->code = -11;
            scal->extra_mv = 2;
            hipk_signal(scal->host_sig, HIPK_SIG_STOP | it);
        }
        return;
    }
    const T al = (T)alpha_new, om = (T)omega_new;
    double acc0 = 0.0, acc1 = 0.0;
    pre.run([&](int64_t i, int nv, T(&v)[1][hipk_vec<T>::VEC]) {
        constexpr int VEC = hipk_vec<T>::VEC;
        T(&sv)[VEC] = v[0];
        T pv[VEC], xv[VEC], hv[VEC], rv[VEC];
        hipk_ld<T>(p, i, nv, pv);
        hipk_ld<T>((const T *)x, i, nv, xv);
        hipk_ld<T>(rhat, i, nv, hv);
        if (exit_early) {  // TSL:942-950 with exit_early true
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const T m0 = al * pv[k];
                xv[k] = xv[k] + m0;
                rv[k] = sv[k];
            }
        } else {
            T tv[VEC], shv[VEC];
            hipk_ld<T>(t, i, nv, tv);
            if (PRE) hipk_ld<T>(shat, i, nv, shv);
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const T m0 = al * pv[k];
                const T m1 = om * (PRE ? shv[k] : sv[k]);  // TSL:942: omega * shat
                const T m2 = m0 + m1;
                xv[k] = xv[k] + m2;
                const T m3 = om * tv[k];
                rv[k] = sv[k] - m3;
            }
        }
#pragma unroll
        for (int k = 0; k < VEC; ++k)
            if (k < nv) {
                acc0 = fma((double)rv[k], (double)rv[k], acc0);
                acc1 = fma((double)hv[k], (double)rv[k], acc1);
            }
        hipk_st<T>(x, i, nv, xv);
        hipk_st<T>(r, i, nv, rv);
    });
    hipk_block_sum2(acc0, acc1, sbuf);
    if (threadIdx.x == 0) {
        part_rr[blockIdx.x] = acc0;
        part_rhr[blockIdx.x] = acc1;
    }
    if (lead) {
        scal->rho = rho_new;
        scal->alpha = alpha_new;
        scal->omega = omega_new;
        scal->iters = it + 1;
        const bool done = (exit_early || it + 1 >= maxiter);  // TSL:961, loop bound :892
        if (done) scal->stop_it = it + 1;
        hipk_signal(scal->host_sig, done ? (HIPK_SIG_STOP | (it + 1)) : (it + 1));
    }
}

// =====================================================================================================================
// Small systems (<= 32 reduction chunks, rows of <= 12 entries; M = identity or Jacobi): THE WHOLE BiCGStab LOOP IN ONE LAUNCH -- the scheme
// of hipk_cg_solve_lds_kernel (csrc/hipk_cg.hip) with three hand-offs per iteration instead of five launches:
//   K1 (tests, beta, p) | K2 q = A p by TILE rows, wavefront sums of rhat .* q            -> hand-off: tile sums + q
//   K3 (alpha test, s, <s,s> sub-partial) | K4 t = A s by tile rows, sums of s .* t, t .* t -> hand-off: tile sums + t + <s,s>
//   K5 (omega tests, x, r, sub-partials of <r,r> and <rhat,r>)                              -> hand-off: those + r
// The SpMV role keeps p, q, r at the columns of its tile row in registers and advances p = r + beta (p - omega q) and
// s = r - alpha q itself from the gathered r and q (the owners' formulas on the owners' operands): neither p nor s is exchanged.
// Arithmetic and every scalar test (TSL:894-936, 961) as in the five kernels above, bit for bit.
template <typename T>
struct hipk_bi_lds_args {
    int64_t n;
    int g;
    const int *crow;
    const int *col;
    const T *val;
    T *x, *r, *p, *q, *t;
    const T *rhat;
    const T *dinv;                  // PRE: Jacobi preconditioning, M = diag(dinv) applied BEFORE A (TSL:908, 922)
    hipk_bi_scal *scal;
    double *tsum0, *tsum1, *tsum2;  // [ntiles * 4] wavefront sums of <rhat,q>, <t,t>, <s,t> (three arrays: a fast workgroup writes
                                    // the sums of the second SpMV while a slow one still folds those of the first)
    double *part_rr, *part_rhr;     // it = 0: chunk partials of <r0,r0> (twice); afterwards [8 g] sub-partials
    double *part_ss;                // [8 g] sub-partials of <s,s>
    unsigned long long *flag_a, *flag_b, *flag_c;   // [64] each, zeroed before the launch
    int64_t it0, maxiter, max_its;
    int test_not_resident;   // tests (hipk_test_fail_launch): report the placement check as failed
    int spread;              // more than 64 workgroups: one per block all over the chip (then LOCAL = false)
};
static constexpr int kBiRowRegs = 12;

template <typename T, bool LOCAL, bool PRE>
__global__ __launch_bounds__(HIPK_THREADS, 2) void hipk_bi_solve_lds_kernel(hipk_bi_lds_args<T> a) {
    constexpr int VEC = hipk_vec<T>::VEC;
    constexpr double EPS = hipk_eps<T>::v;
    int wg = blockIdx.x;                             // spread (more than 64 workgroups): one per block, anywhere on the chip
    if (!a.spread) {
        if (blockIdx.x & 7) return;                  // the working blocks share an XCD (dispatch is round-robin over 8)
        wg = blockIdx.x >> 3;
    }
    const int c = wg / kGmSub, s_ = wg % kGmSub;
    const int g = a.g, nwg = g * kGmSub;
    if (c >= g) return;
    hipk_bi_scal *scal = a.scal;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int u = tid & 31, e8 = tid >> 5;
    const int64_t n = a.n;
    const int64_t base = (int64_t)c * HIPK_BASE_CHUNK;
    const int64_t row = base + (int64_t)VEC * (s_ + kGmSub * u) + (int64_t)(e8 / VEC) * (VEC * HIPK_THREADS) + (e8 % VEC);
    const bool live = row < n;
    const int ntiles = (int)((n + HIPK_TILE - 1) / HIPK_TILE);
    const int tile = c * (HIPK_BASE_CHUNK / HIPK_TILE) + s_;
    const int64_t trow = (int64_t)tile * HIPK_TILE + tid;
    const bool tlive = trow < n;

    __shared__ T wl[HIPK_THREADS], wh[HIPK_THREADS];
    __shared__ double bc[4];
    __shared__ int fail;
    __shared__ unsigned long long res_lds;
    if (tid == 0) fail = 0;

    // vector role
    T x_own = live ? a.x[row] : (T)0, r_own = live ? a.r[row] : (T)0, p_own = live ? a.p[row] : (T)0;
    T q_own = live ? a.q[row] : (T)0;
    const T h_own = live ? a.rhat[row] : (T)0;
    wh[tid] = h_own;
    // SpMV role: the tile row's entries; p and q at its columns (the launches before this one left them in memory)
    int lo = 0, len = 0;
    if (tlive) {
        lo = a.crow[trow];
        len = a.crow[trow + 1] - lo;
    }
    unsigned cj[kBiRowRegs];
    T vj[kBiRowRegs], pc[kBiRowRegs], qc[kBiRowRegs];
#pragma unroll
    for (int j = 0; j < kBiRowRegs; ++j) {
        const int cc = (j < len) ? a.col[lo + j] : 0;
        cj[j] = (unsigned)cc * (unsigned)sizeof(T);
        vj[j] = (j < len) ? a.val[lo + j] : (T)0;
        pc[j] = (j < len) ? a.p[cc] : (T)0;
        qc[j] = (j < len) ? a.q[cc] : (T)0;
    }
    const T h_t = tlive ? a.rhat[trow] : (T)0;
    T d_own = (T)1, dc[kBiRowRegs];   // PRE: the diagonal of M at the own row and at the tile row's columns
#pragma unroll
    for (int j = 0; j < kBiRowRegs; ++j) dc[j] = (T)1;
    if (PRE) {
        d_own = live ? a.dinv[row] : (T)0;
#pragma unroll
        for (int j = 0; j < kBiRowRegs; ++j) dc[j] = (j < len) ? a.dinv[a.col[lo + j]] : (T)0;
    }
    int wmax = len < kBiRowRegs ? len : kBiRowRegs;
    for (int off = 32; off > 0; off >>= 1) {
        const int o = __shfl_xor(wmax, off);
        wmax = o > wmax ? o : wmax;
    }
    wmax = __builtin_amdgcn_readfirstlane(wmax);
    double rho = scal->rho, alpha = scal->alpha, omega = scal->omega;
    const double atol2 = scal->atol2;
    const int64_t stop0 = scal->stop_it;

    // every workgroup resident (and, LOCAL, on one XCD)?  Nothing has been modified yet: a failure leaves the solve to the launches
    int epoch = 0;
    if (LOCAL && tid == 0) {
        unsigned xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        __hip_atomic_fetch_or(&scal->xcc_mask, 1u << (xcc & 15u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (!hipk_gbar(&scal->bar, nwg, epoch, &fail) || a.test_not_resident) {
        if (tid == 0) scal->redo = -1;
        return;
    }
    if (LOCAL) {
        if (tid == 0) {
            const unsigned mask = __hip_atomic_load(&scal->xcc_mask, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            fail = (__builtin_popcount(mask) == 1) ? 0 : 1;
        }
        __syncthreads();
        if (fail) {
            if (tid == 0) scal->redo = -2;
            return;
        }
    }
#define HIPK_BI_HO(flags)                                                      \
    if (hipk_ho_sync<LOCAL>(flags, wg, nwg, ++seq, 0u, &res_lds) == ~0ull) {   \
        if (tid == 0) scal->redo = -3;                                         \
        return;                                                                \
    }
    auto fold_tiles = [&](const double *tp, int i8) {   // i8 = lane of a whole wavefront
        return hipk_fold_64x8(i8, g, [&](int ci, int tt) {
            const int tl = ci * (HIPK_BASE_CHUNK / HIPK_TILE) + tt;
            if (tl >= ntiles) return 0.0;
            const double *w4 = tp + (size_t)tl * 4;
            const double w0 = hipk_peek(w4), w1 = hipk_peek(w4 + 1), w2 = hipk_peek(w4 + 2), w3 = hipk_peek(w4 + 3);
            return 0.0 + ((w0 + w1) + (w2 + w3));
        });
    };
    auto fold_subs = [&](const double *sp, int i8) {
        return hipk_fold_64x8(i8, g, [&](int ci, int ss) { return hipk_peek(sp + ci * kGmSub + ss); });
    };
    auto fold_chunks = [&](const double *cp, int i8) {   // it = 0: chunk partials of the launches before this one (hipk_reduce_parts)
        double a8 = (i8 < g) ? hipk_peek(cp + i8) : 0.0;
        a8 = 0.0 + a8;
        return hipk_wave_sum(a8);
    };
    unsigned long long seq = 0;
    int64_t it = a.it0, iters = a.it0;
    int code = 0, extra_mv = 0;
    double rs_last = scal->rs_last;
    int64_t stop_it = stop0;
    bool handed = true;   // the r / <r,r> / <rhat,r> this iteration starts from are visible (a launch or a hand-off before)
    while (it < stop_it && it - a.it0 < a.max_its) {
        if (!handed) {
            HIPK_BI_HO(a.flag_c)
            handed = true;
        }
        // ---- K1: rs = <r,r>, rho' = <rhat,r> -> tests; beta; p = r + beta (p - omega q)   (TSL:893-907)
        T rc[kBiRowRegs];
#pragma unroll
        for (int j = 0; j < kBiRowRegs; ++j)
            if (j < wmax) rc[j] = hipk_peek_off<T>(a.r, cj[j]);
        const T r_t = tlive ? hipk_peek_t<T>(a.r + trow) : (T)0;
        if (tid < 64) {
            const double v = (it == 0) ? fold_chunks(a.part_rr, tid) : fold_subs(a.part_rr, tid);
            if (tid == 0) bc[0] = v;
        } else if (tid < 128) {
            const double v = (it == 0) ? fold_chunks(a.part_rhr, tid - 64) : fold_subs(a.part_rhr, tid - 64);
            if (tid == 64) bc[1] = v;
        }
        __syncthreads();
        const double rs = bc[0], rho_new = bc[1];
        rs_last = rs;
        if (rs <= atol2) {  // TSL:894-896
            stop_it = it;
            break;
        }
        if (fabs(rho_new) < EPS * fabs(rho)) {  // TSL:902-904
            stop_it = it;
            code = -10;
            break;
        }
        const T beta = (T)(rho_new / rho * alpha / omega);  // TSL:906, left to right
        const T om = (T)omega;
        {
            const T t1 = om * q_own;
            const T t2 = p_own - t1;
            const T t3 = beta * t2;
            p_own = r_own + t3;
        }
#pragma unroll
        for (int j = 0; j < kBiRowRegs; ++j)
            if (j < wmax) {
                const T t1 = om * qc[j];
                const T t2 = pc[j] - t1;
                const T t3 = beta * t2;
                pc[j] = rc[j] + t3;
            }
        // ---- K2 (tile rows): q = A p, wavefront sums of rhat .* q   (TSL:909-910)
        T q_t;
        {
            T acc_row = (T)0;
#pragma unroll
            for (int j = 0; j < kBiRowRegs; ++j)
                if (j < wmax) {
                    const T pin = PRE ? dc[j] * pc[j] : pc[j];   // phat = M p (TSL:908)
                    const T pr = vj[j] * pin;
                    acc_row = (j < len) ? acc_row + pr : acc_row;
                }
            q_t = tlive ? acc_row : (T)0;
            double d0 = tlive ? (double)h_t * (double)q_t : 0.0;
            d0 = hipk_wave_sum(d0);
            if (lane == 0 && tile < ntiles) hipk_ho_store<LOCAL>(&a.tsum0[(size_t)tile * 4 + wave], d0);
            if (tlive) hipk_ho_store<LOCAL>(a.q + trow, q_t);
        }
        HIPK_BI_HO(a.flag_a)
        // ---- K3: alpha' = rho'/<rhat,q> -> test; s = r - alpha' q; <s,s>   (TSL:910-920)
        q_own = live ? hipk_peek_t<T>(a.q + row) : (T)0;
#pragma unroll
        for (int j = 0; j < kBiRowRegs; ++j)
            if (j < wmax) qc[j] = hipk_peek_off<T>(a.q, cj[j]);
        if (tid < 64) {
            const double v = fold_tiles(a.tsum0, tid);
            if (tid == 0) bc[2] = v;
        }
        __syncthreads();
        const double rq = bc[2];
        const double alpha_new = rho_new / rq;  // TSL:910
        if (fabs(alpha_new) < EPS) {            // TSL:913-915
            stop_it = it;
            code = -11;
            extra_mv = 1;
            break;
        }
        const T al = (T)alpha_new;
        T s_own;
        {
            const T m = al * q_own;
            s_own = r_own - m;  // TSL:917
        }
        wl[tid] = s_own;
        __syncthreads();
        if (tid < 32) {
            double acc = 0.0;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const double v = (double)wl[e * 32 + tid];
                acc = fma(v, v, acc);
            }
            acc = hipk_half_sum(acc);
            if (tid == 0) hipk_ho_store<LOCAL>(&a.part_ss[wg], acc);
        }
        // ---- K4 (tile rows): t = A s, wavefront sums of s .* t and t .* t   (TSL:923-930)
        {
            T acc_row = (T)0;
#pragma unroll
            for (int j = 0; j < kBiRowRegs; ++j)
                if (j < wmax) {
                    const T m = al * qc[j];
                    const T sc = rc[j] - m;
                    const T sin = PRE ? dc[j] * sc : sc;         // shat = M s (TSL:922)
                    const T pr = vj[j] * sin;
                    acc_row = (j < len) ? acc_row + pr : acc_row;
                }
            const T t_t = tlive ? acc_row : (T)0;
            const T mt = al * q_t;
            const T s_t = r_t - mt;
            double d0 = tlive ? (double)s_t * (double)t_t : 0.0;
            double d1 = tlive ? (double)t_t * (double)t_t : 0.0;
            d0 = hipk_wave_sum(d0);
            d1 = hipk_wave_sum(d1);
            if (lane == 0 && tile < ntiles) {
                hipk_ho_store<LOCAL>(&a.tsum2[(size_t)tile * 4 + wave], d0);
                hipk_ho_store<LOCAL>(&a.tsum1[(size_t)tile * 4 + wave], d1);
            }
            if (tlive) hipk_ho_store<LOCAL>(a.t + trow, t_t);
        }
        HIPK_BI_HO(a.flag_b)
        // ---- K5: omega' -> tests; x += alpha' p (+ omega' s); r = s (- omega' t); <r,r>, <rhat,r>   (TSL:920-961)
        const T t_own = live ? hipk_peek_t<T>(a.t + row) : (T)0;
        if (tid < 64) {
            const double v = fold_subs(a.part_ss, tid);
            if (tid == 0) bc[0] = v;
        } else if (tid < 128) {
            const double v = fold_tiles(a.tsum2, tid - 64);
            if (tid == 64) bc[1] = v;
        } else if (tid < 192) {
            const double v = fold_tiles(a.tsum1, tid - 128);
            if (tid == 128) bc[2] = v;
        }
        __syncthreads();
        const double ss = bc[0], ts = bc[1], tt = bc[2];
        const bool exit_early = ss < atol2;                                   // TSL:920 (strict)
        const double omega_new = (fabs(tt) < EPS) ? 0.0 : ts / tt;            // TSL:926-930
        if (fabs(omega_new) < EPS && !exit_early) {                           // TSL:934-936
            stop_it = it;
            code = -11;
            extra_mv = 2;
            break;
        }
        const T omn = (T)omega_new;
        const T ph_own = PRE ? d_own * p_own : p_own, sh_own = PRE ? d_own * s_own : s_own;   // x advances with phat, shat (TSL:942)
        if (exit_early) {  // TSL:942-950 with exit_early true
            const T m0 = al * ph_own;
            x_own = x_own + m0;
            r_own = s_own;
        } else {
            const T m0 = al * ph_own;
            const T m1 = omn * sh_own;
            const T m2 = m0 + m1;
            x_own = x_own + m2;
            const T m3 = omn * t_own;
            r_own = s_own - m3;
        }
        __syncthreads();   // bc and wl are free again
        wl[tid] = r_own;
        if (live) hipk_ho_store<LOCAL>(a.r + row, r_own);
        __syncthreads();
        if (tid < 32) {
            double acc0 = 0.0, acc1 = 0.0;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const double rv = (double)wl[e * 32 + tid], hv = (double)wh[e * 32 + tid];
                acc0 = fma(rv, rv, acc0);
                acc1 = fma(hv, rv, acc1);
            }
            acc0 = hipk_half_sum(acc0);
            acc1 = hipk_half_sum(acc1);
            if (tid == 0) {
                hipk_ho_store<LOCAL>(&a.part_rr[wg], acc0);
                hipk_ho_store<LOCAL>(&a.part_rhr[wg], acc1);
            }
        }
        rho = rho_new;
        alpha = alpha_new;
        omega = omega_new;
        ++it;
        iters = it;
        if (exit_early || it >= a.maxiter) {  // TSL:961, loop bound :892
            stop_it = it;
            break;
        }
        handed = false;
    }
#undef HIPK_BI_HO
    if (live) {
        a.x[row] = x_own;
        a.p[row] = p_own;
    }
    if (wg == 0 && tid == 0) {
        scal->rho = rho;
        scal->alpha = alpha;
        scal->omega = omega;
        scal->rs_last = rs_last;
        scal->iters = iters;
        scal->code = code;
        scal->extra_mv = extra_mv;
        scal->it_done = it;
        if (stop_it < stop0) scal->stop_it = stop_it;
    }
}

__global__ __launch_bounds__(HIPK_THREADS) void hipk_bi_final_kernel(hipk_bi_scal *__restrict__ scal, int g,
                                                                     const double *__restrict__ part_res,
                                                                     const double *__restrict__ part_xx) {
    __shared__ double sbuf[2 * HIPK_THREADS];
    double res2, xx;
    hipk_reduce_parts2(part_res, part_xx, g, res2, xx, sbuf);
    if (threadIdx.x == 0) {
        scal->res2 = res2;
        scal->xx = xx;
    }
}

static constexpr int kBiSlots = 8;

// ---------------------------------------------------------------- the workspace of a solve
// Byte offsets, from (n, dtype, pre) alone: hipk_bicgstab_work_bytes and hipk_pbicgstab_work_bytes return .total, the solve takes
// its pointers from the rest.  scalars (hipk_bi_scal) | kBiSlots partial arrays | r, rhat, p, q, s, t | two more vector places
// (pre: phat, shat) | mid-size systems: the flagged words and partial slots of hipk_bi_mid_kernel.
// Three loop forms use it -- the mid loop, the LDS loop, the five-launch sequence -- one after the other: a one-launch loop has
// returned (finished, or handed the solve back) before the next form's first launch is enqueued, and none runs twice.  A region
// of one form may therefore lie in bytes that another form owns.
struct hipk_bi_layout {
    size_t scal;
    // chunk partials of the five-launch sequence; part_spare: the dot slot an SpMV does not need
    size_t part_rr, part_rhr, part_rq, part_ss, part_ts, part_tt, part_bb, part_spare;
    size_t r, rhat, p, q, s, t;
    size_t phat, shat;   // the SpMV inputs (TSL:908, 922); M = identity: p and s themselves
    // The LDS loop (hipk_bi_solve_lds_kernel) in slots of the five-launch sequence, whose <t,s> and <t,t> partials are only
    // written once that sequence runs:
    size_t lds_flags;    // 3 x kHoMaxWg hand-off words, in the <t,t> slot
    size_t lds_tsum2;    // the third tile-sum array, 4 words per tile, in the <t,s> slot
    // The mid loop (hipk_bi_mid_kernel), behind the EIGHT vector places whether the solve is preconditioned or not (present iff mid):
    bool mid;
    size_t ll_bytes;     // n 16-byte flagged words, whatever the dtype
    size_t q_ll, r_ll;   // q and r as flagged words
    size_t slots;        // kBiMidSlotBytes of chunk-partial slots
    size_t total;
};
static_assert(3 * kHoMaxWg <= HIPK_MAX_PARTS, "the LDS loop's hand-off flags fit the <t,t> slot");
static_assert(4 * kHoMaxChunks * (HIPK_BASE_CHUNK / HIPK_TILE) <= HIPK_MAX_PARTS, "the LDS loop's third tile-sum array fits the <t,s> slot");

static hipk_bi_layout hipk_bi_make_layout(int64_t n, int dtype, bool pre) {
    const size_t rows = (size_t)(n > 0 ? n : 1), vec = hipk_align_up(rows * (dtype == HIPK_F64 ? 8 : 4), 256);
    const hipk_geom gm = hipk_make_geom(n > 0 ? n : 1);
    hipk_bi_layout L;
    hipk_carve take;
    L.scal = take(256);
    size_t *const parts[kBiSlots] = {&L.part_rr, &L.part_rhr, &L.part_rq, &L.part_ss, &L.part_ts, &L.part_tt, &L.part_bb, &L.part_spare};
    for (size_t *slot : parts) *slot = take(HIPK_MAX_PARTS * sizeof(double));
    L.lds_flags = L.part_tt;
    L.lds_tsum2 = L.part_ts;
    size_t *const vecs[6] = {&L.r, &L.rhat, &L.p, &L.q, &L.s, &L.t};
    for (size_t *v : vecs) *v = take(vec);
    L.mid = gm.g > kMidMinChunks && gm.g <= kBiMidMaxChunks;
    // places seven and eight: phat and shat of a preconditioned solve; a plain solve of a mid-size system leaves them unused
    const size_t v7 = (pre || L.mid) ? take(vec) : 0, v8 = (pre || L.mid) ? take(vec) : 0;
    L.phat = pre ? v7 : L.p;
    L.shat = pre ? v8 : L.s;
    L.ll_bytes = hipk_align_up(rows * 16, 256);
    L.q_ll = L.mid ? take(L.ll_bytes) : 0;
    L.r_ll = L.mid ? take(L.ll_bytes) : 0;   // (directly behind q_ll: one memset clears both)
    L.slots = L.mid ? take(kBiMidSlotBytes) : 0;
    // hipk_pbicgstab_work_bytes has always been the plain size + two vectors: at the mid sizes, where the plain size already
    // holds places seven and eight, two unused vectors end the workspace.  Callers size buffers by it; kept.
    if (pre && L.mid) take(2 * vec);
    L.total = take.o;
    return L;
}
extern "C" size_t hipk_bicgstab_work_bytes(int64_t n, int dtype) { return hipk_bi_make_layout(n, dtype, false).total; }
extern "C" size_t hipk_pbicgstab_work_bytes(int64_t n, int dtype) { return hipk_bi_make_layout(n, dtype, true).total; }   // + phat, shat

// the one-launch instantiations the dispatch below selects (hipk_mid_pick), each with the name hipk_last_solve_path reports
#define HIPK_MID_ROW(W, PRE)                                                                                               \
    {W, 1, PRE, hipk_bi_mid_kernel<T, W, PRE>,                                                                             \
     HIPK_FORM_OF_T(T, "hipk_bi_mid_kernel<", #W "," #PRE ">")}
template <typename T>
static const hipk_mid_entry<hipk_bi_mid_args> hipk_bi_mid_table[] = {
    HIPK_MID_ROW(5, false), HIPK_MID_ROW(7, false), HIPK_MID_ROW(9, false), HIPK_MID_ROW(12, false),
    HIPK_MID_ROW(5, true),  HIPK_MID_ROW(7, true),  HIPK_MID_ROW(9, true),  HIPK_MID_ROW(12, true)};
#undef HIPK_MID_ROW
// {redo, it_done, stop_it} of a host copy of the scalar block (hipk_resident_run)
static hipk_loop_state hipk_bi_loop_state(const hipk_bi_scal &h) { return {h.redo, h.it_done, h.stop_it}; }

// ---- which paths a bicgstab solve takes (PRE: Jacobi; ext: the caller's M through a callback): the only place that knows
// BiCGStab's switches and size limits.  Two steps, because a mid loop that handed the solve back changes what the LDS loop may do:
//   hipk_bi_path_begin   before the iteration loop: small and the mid loop
//   hipk_bi_path_lds     after the mid loop (mid_done: it finished the solve), at iteration `it`: the LDS loop
// What is left is the five-launch sequence (small picks its kernels).
struct hipk_bi_path {
    bool small = false;      // <= 8 reduction chunks: both SpMVs skip their combine launch, the consumers fold the tile sums
    bool mid = false;        // hipk_bi_mid_kernel: the whole loop in one launch, one workgroup per chunk (hipk_bi_mid.h)
    const hipk_mid_entry<hipk_bi_mid_args> *mid_entry = nullptr;
    hipk_mid_plan mid_plan;
    size_t mid_lds = 0;
    bool lds_loop = false;   // hipk_bi_solve_lds_kernel: the whole loop in one launch, eight workgroups per chunk
    bool spread = false;     // ... spread over the chip (more than 64 workgroups) instead of on ONE XCD
    bool local = false;      // ... hand-offs through that XCD's L2 (a -2 of the kernel: agent scope from then on)
    int64_t max_its = 0;     // iterations one launch of either loop may run
};

template <typename T, bool PRE>
static hipk_bi_path hipk_bi_path_begin(hipk_csr_s *A, const hipk_params *prm, bool ext, int64_t maxiter, bool mid_failed, hipStream_t stream) {
    const int g = A->geom.g;
    hipk_bi_path path;
    path.small = g <= 8 && !hipk_sw_present("HIPK_BICGSTAB_NO_SMALL");
    // launch-bound systems of 9 .. 256 chunks (fp64, M = identity or Jacobi, rows of <= 12 entries within a window around their
    // chunk): one workgroup per chunk, one per CU; HIPK_BICGSTAB_MID=0 leaves them to the paths below
    path.mid_entry = hipk_mid_pick(hipk_bi_mid_table<T>, A->max_row_len, 1, PRE);
    auto mid_lds = [](int slots) { return hipk_bi_mid_lds_bytes(slots * HIPK_TILE, PRE, sizeof(T)); };
    // (hipk_mid_eligible last: it builds the handle's window plan on the stream and queries occupancy)
    path.mid = !ext && g > kMidMinChunks && g <= kBiMidMaxChunks && g <= A->n_cu && A->geom.ch == HIPK_BASE_CHUNK && A->op_cb == nullptr &&
               A->crow != nullptr && A->max_row_len <= 12 && prm->profile == 0 && maxiter > 0 && !mid_failed &&
               hipk_sw_enabled("HIPK_BICGSTAB_MID") && !hipk_sw_present("HIPK_BICGSTAB_NO_LDS_LOOP") && !hipk_sw_present("HIPK_BICGSTAB_NO_SMALL") &&
               path.mid_entry && hipk_mid_eligible(A, path.mid_entry, g, mid_lds, stream, &path.mid_plan, &path.mid_lds);
    if (path.mid) path.max_its = hipk_sw_int("HIPK_BICGSTAB_LAUNCH_ITS", 8192, 1);
    return path;
}

// launch-bound systems with short rows, M = identity or Jacobi: up to 64 workgroups (8 chunks) on ONE XCD; up to 32 chunks
// (n <= 65536) spread over the chip, two workgroups per compute unit.  lds_failed: its workgroups once failed to meet (a shared
// device): do not wait for that verdict again.  it == 0: after the mid loop gave up mid-solve, part_rr / part_rhr hold CHUNK
// partials, which only the launch sequence folds
static void hipk_bi_path_lds(hipk_bi_path &path, const hipk_csr_s *A, const hipk_params *prm, bool ext, int64_t maxiter, bool mid_done,
                             int64_t it, bool lds_failed) {
    const int g = A->geom.g;
    path.spread = kGmSub * g > 64;
    path.lds_loop = g <= 32 && !hipk_sw_present("HIPK_BICGSTAB_NO_SMALL") && !ext && A->geom.ch == HIPK_BASE_CHUNK &&
                    A->max_row_len <= kBiRowRegs && prm->profile == 0 && maxiter > 0 &&
                    kGmSub * g <= (path.spread ? 2 * A->n_cu : 2 * (A->n_cu / 8)) && !lds_failed &&
                    !hipk_sw_present("HIPK_BICGSTAB_NO_LDS_LOOP") && !(path.spread && hipk_sw_present("HIPK_NO_LDS_SPREAD")) && !mid_done && it == 0;
    if (path.lds_loop) {
        path.local = !path.spread && !hipk_sw_present("HIPK_BICGSTAB_LOOP_AGENT");
        path.max_its = hipk_sw_int("HIPK_BICGSTAB_LAUNCH_ITS", 8192, 1);
    }
}

// what the five-launch sequence launches for its s and x updates, and the partials those fold (hipk_bi_steps::pick)
template <typename T, bool PRE>
struct hipk_bi_kernels {
    decltype(&hipk_bi_supdate_kernel<T, PRE, false>) supdate;
    decltype(&hipk_bi_xupdate_kernel<T, PRE, false>) xupdate;
    const double *rq, *ts, *tt;   // <rhat,q>, <t,s>, <t,t>: chunk partials, or (small) the SpMVs' tile sums
    int nt;                       // small: the tile count; else 0
};

// One single-device solve: its operands, workspace and state, and the steps hipk_bicgstab_solve_t drives it through.
// PRE: Jacobi, M = diag(dinv) applied in the kernels.  cb != null (PRE = false): the preconditioner is the CALLER's device code
// -- cb(user, in, out) enqueues out = M(in) on `stream` -- applied where the Jacobi variant scales in-kernel: phat = M(p) before
// the first SpMV, shat = M(s) before the second (TSL:908, 922), M(b - A x) for the final test (TSL:1007).  Same kernels, same
// order of operations.
template <typename T, bool PRE>
struct hipk_bi_steps {
    hipk_csr_s *A;
    const T *dinv, *b;
    T *x;
    hipk_precond_fn cb;
    void *user;
    const hipk_params *prm;
    hipStream_t stream;
    const bool ext;   // M through the callback
    const int64_t n, maxiter;
    const hipk_geom gm;
    const int nt;
    const hipk_bi_layout lay;
    char *const work;
    hipk_bi_scal *const scal = hipk_at<hipk_bi_scal>(work, lay.scal);
    double *const part_rr = hipk_at<double>(work, lay.part_rr), *const part_rhr = hipk_at<double>(work, lay.part_rhr);
    double *const part_rq = hipk_at<double>(work, lay.part_rq), *const part_ss = hipk_at<double>(work, lay.part_ss);
    double *const part_ts = hipk_at<double>(work, lay.part_ts), *const part_tt = hipk_at<double>(work, lay.part_tt);
    double *const part_bb = hipk_at<double>(work, lay.part_bb), *const part_spare = hipk_at<double>(work, lay.part_spare);
    T *const r = hipk_at<T>(work, lay.r), *const rhat = hipk_at<T>(work, lay.rhat), *const p = hipk_at<T>(work, lay.p), *const q = hipk_at<T>(work, lay.q);
    T *const s = hipk_at<T>(work, lay.s), *const t = hipk_at<T>(work, lay.t), *const phat = hipk_at<T>(work, lay.phat), *const shat = hipk_at<T>(work, lay.shat);
    hipk_event_pair whole;
    hipk_spmv_profiler prof;
    hipk_pacer pace;
    hipk_bi_path path;
    int64_t it = 0, stop = INT64_MAX;
    bool done = false;       // a one-launch loop finished the solve
    char handed[128] = "";   // the one-launch loops that handed this solve back

    hipk_bi_steps(hipk_csr_s *A_, const T *dinv_, const T *b_, T *x_, char *w, const hipk_params *prm_, hipStream_t s_, hipk_precond_fn cb_, void *user_)
        : A(A_), dinv(dinv_), b(b_), x(x_), cb(cb_), user(user_), prm(prm_), stream(s_), ext(cb_ != nullptr), n(A_->n_rows),
          maxiter(hipk_default_maxiter(prm_, A_->n_rows)), gm(A_->geom), nt((int)((A_->n_rows + HIPK_TILE - 1) / HIPK_TILE)),
          lay(hipk_bi_make_layout(A_->n_rows, A_->dtype, PRE || cb_ != nullptr)), work(w), prof(prm_->profile != 0 ? HIPK_K_SPMV : 0),
          pace(A_->host_poll, &scal->stop_it, prm_->check_every > 0 ? prm_->check_every : 32) {}

    // ext: out = M(in) by the caller
    int precondition(const T *in, T *out) const {
        if (cb(user, in, out) != 0) {
            hipk_set_error("hipk_pbicgstab_solve_cb: the preconditioner callback failed");
            return HIPK_ERR_ARG;
        }
        return HIPK_OK;
    }

    // y = b - A x (scaled: M = diag(dinv) in the SpMV epilogue), the chunk partials of its squared norm in part_yy
    int residual(T *y, double *part_yy, bool scaled) const {
        hipk_spmv_args sa = hipk_spmv_base(A);
        sa.x = x;
        sa.y = y;
        sa.mode = HIPK_SPMV_RESID | HIPK_SPMV_DOT_YY | (scaled ? HIPK_SPMV_SCALE : 0);
        sa.dscale = scaled ? dinv : nullptr;
        sa.bsub = b;
        sa.part0 = part_spare;
        sa.part1 = part_yy;
        return hipk_launch_spmv(A, sa, stream);
    }

    // r0 = b - A x0 with <r0,r0>; <b,b>; rhat = p = q = r0, the stop word and the tolerances (TSL:870-890)
    int start() {
        hipk_set_solve_path(nullptr, "");
        HIPK_CHECK_HIP(whole.create());
        HIPK_CHECK_HIP(hipEventRecord(whole.a, stream));
        HIPK_TRY(residual(r, part_rr, false));
        HIPK_TRY(hipk_launch_dot_parts(n, b, b, A->dtype, part_bb, stream));
        HIPK_CHECK_HIP(pace.create());   // zeroes the pinned signal word: before the kernel that may write it is enqueued
        const hipk_tol_sq tol(prm);
        hipk_bi_start_kernel<T><<<gm.g, HIPK_THREADS, 0, stream>>>(n, gm.ch, gm.g, scal, part_rr, part_bb, part_rhr, r, rhat, p, q, tol.tol2,
                                                                    tol.atol_sq, maxiter, pace.device_sig());
        HIPK_CHECK_HIP(hipGetLastError());
        return HIPK_OK;
    }

    // the whole loop in one launch, one workgroup per chunk (hipk_bi_mid.h), from iteration `it` -- HIPK_OK, HIPK_HANDED_BACK or
    // an error (hipk_resident_run); failed: the caller's latch
    int mid_loop(bool &failed) {
        const hipk_mid_entry<hipk_bi_mid_args> *mid = path.mid_entry;
        const size_t lds = path.mid_lds;
        hipk_bi_mid_args ca;
        ca.n = n;
        ca.g = gm.g;
        ca.win = path.mid_plan.max_slots * HIPK_TILE;
        ca.plan = path.mid_plan;
        ca.crow = A->crow;
        ca.col = A->col;
        ca.val = A->val;
        ca.x = x;
        ca.r = r;
        ca.p = p;
        ca.q = q;
        ca.rhat = rhat;
        ca.dinv = dinv;
        ca.q_ll = hipk_at<unsigned long long>(work, lay.q_ll);
        ca.r_ll = hipk_at<unsigned long long>(work, lay.r_ll);
        ca.slots = hipk_at<unsigned long long>(work, lay.slots);
        ca.part_rr = part_rr;
        ca.part_rhr = part_rhr;
        ca.scal = scal;
        ca.maxiter = maxiter;
        ca.max_its = path.max_its;
        ca.slot_stride = gm.g <= 32 ? 1 : 16;
        ca.xcd_aware = 1;
        auto launch = [&](int64_t it0, int test_not_resident, bool) -> int {
            ca.it0 = it0;
            ca.test_not_resident = test_not_resident;
            HIPK_CHECK_HIP(hipMemsetAsync(ca.q_ll, 0, 2 * lay.ll_bytes, stream));   // q_ll and r_ll
            HIPK_CHECK_HIP(hipMemsetAsync(ca.slots, 0, kBiMidSlotBytes, stream));
            HIPK_CHECK_HIP(hipMemsetAsync(&scal->it_done, 0, sizeof(hipk_bi_scal) - offsetof(hipk_bi_scal, it_done), stream));
            mid->kern<<<hipk_xcd_grid(gm.g), 1024, lds, stream>>>(ca);
            return HIPK_OK;
        };
        return hipk_resident_run(stream, scal, launch, hipk_bi_loop_state, it, maxiter, nullptr, failed, handed, mid->name, "hipk_bicgstab_solve");
    }

    // the whole loop in one launch, eight workgroups per chunk (hipk_bi_solve_lds_kernel), from iteration `it` -- as mid_loop;
    // *form: the instantiation of its last launch (hipk_last_solve_form)
    int lds_loop(bool &failed, const char **form) {
        bool local = path.local;   // a -2 (spread over several XCDs): agent-scope hand-offs
        hipk_bi_lds_args<T> ca;
        ca.n = n;
        ca.g = gm.g;
        ca.crow = A->crow;
        ca.col = A->col;
        ca.val = (const T *)A->val;
        ca.x = x;
        ca.r = r;
        ca.p = p;
        ca.q = q;
        ca.t = t;
        ca.rhat = rhat;
        ca.dinv = dinv;
        ca.scal = scal;
        ca.tsum0 = A->tile_part;
        ca.tsum1 = A->tile_part + 4 * (size_t)nt;
        ca.tsum2 = hipk_at<double>(work, lay.lds_tsum2);
        ca.part_rr = part_rr;
        ca.part_rhr = part_rhr;
        ca.part_ss = part_ss;
        ca.flag_a = hipk_at<unsigned long long>(work, lay.lds_flags);
        ca.flag_b = ca.flag_a + kHoMaxWg;
        ca.flag_c = ca.flag_a + 2 * kHoMaxWg;
        ca.spread = path.spread ? 1 : 0;
        const int lgrid = path.spread ? kGmSub * gm.g : 8 * kGmSub * gm.g;
        ca.maxiter = maxiter;
        ca.max_its = path.max_its;
        auto launch = [&](int64_t it0, int test_not_resident, bool loc) -> int {
            ca.it0 = it0;
            ca.test_not_resident = test_not_resident;
            HIPK_CHECK_HIP(hipMemsetAsync(ca.flag_a, 0, 3 * kHoMaxWg * sizeof(unsigned long long), stream));
            HIPK_CHECK_HIP(hipMemsetAsync(&scal->it_done, 0, sizeof(hipk_bi_scal) - offsetof(hipk_bi_scal, it_done), stream));
            (loc ? hipk_bi_solve_lds_kernel<T, true, PRE> : hipk_bi_solve_lds_kernel<T, false, PRE>)<<<lgrid, HIPK_THREADS, 0, stream>>>(ca);
            return HIPK_OK;
        };
        // a hand-back (not co-resident; this launch modified nothing): the launch sequence takes over
        const int run = hipk_resident_run(stream, scal, launch, hipk_bi_loop_state, it, maxiter, &local, failed, handed, "hipk_bi_solve_lds_kernel",
                                          "hipk_bicgstab_solve");
        if (run == HIPK_HANDED_BACK && it > 0) {
            // ... from iteration `it` of an EARLIER launch: the vectors and scalars are in memory, but part_rr / part_rhr hold
            // that launch's 8 g SUB-partials, not the g chunk partials the direction kernel folds.  Recompute them from r
            // and rhat (the spec's plain dot: the bits the x-update kernel of the launch sequence would have left)
            HIPK_TRY(hipk_launch_dot_parts(n, r, r, A->dtype, part_rr, stream));
            HIPK_TRY(hipk_launch_dot_parts(n, rhat, r, A->dtype, part_rhr, stream));
        }
        *form = local ? (PRE ? HIPK_FORM_OF_T(T, "hipk_bi_solve_lds_kernel<", "true,true>") : HIPK_FORM_OF_T(T, "hipk_bi_solve_lds_kernel<", "true,false>"))
                      : (PRE ? HIPK_FORM_OF_T(T, "hipk_bi_solve_lds_kernel<", "false,true>") : HIPK_FORM_OF_T(T, "hipk_bi_solve_lds_kernel<", "false,false>"));
        return run;
    }

    const char *five_launch_form() const {
        return path.small ? (ext ? HIPK_FORM("bicgstab five-launch, small, callback M") : PRE ? HIPK_FORM("bicgstab five-launch, small, Jacobi") : HIPK_FORM("bicgstab five-launch, small"))
                          : (ext ? HIPK_FORM("bicgstab five-launch, callback M") : PRE ? HIPK_FORM("bicgstab five-launch, Jacobi") : HIPK_FORM("bicgstab five-launch"));
    }

    // The one-launch section: the mid loop, else the LDS loop, from iteration `it`; `done` when one of them finished the solve, else
    // the five-launch sequence goes on from `it`.  Records the path and the form the solve reports.  The latches: a one-launch loop
    // once handed a solve back in this process
    int one_launch(bool &mid_failed, bool &lds_failed) {
        path = hipk_bi_path_begin<T, PRE>(A, prm, ext, maxiter, mid_failed, stream);
        bool mid_done = false, lds_done = false;
        const char *lds_form = "";
        if (path.mid) {
            const int run = mid_loop(mid_failed);
            if (run < 0) return run;
            mid_done = run == HIPK_OK;
        }
        hipk_bi_path_lds(path, A, prm, ext, maxiter, mid_done, it, lds_failed);
        if (path.lds_loop) {
            const int run = lds_loop(lds_failed, &lds_form);
            if (run < 0) return run;
            lds_done = run == HIPK_OK;
        }
        done = mid_done || lds_done;
        hipk_set_solve_path(handed, mid_done ? path.mid_entry->name : lds_done ? "hipk_bi_solve_lds_kernel" : "launch sequence");
        hipk_set_solve_form(mid_done ? path.mid_entry->name : lds_done ? lds_form : five_launch_form());
        return HIPK_OK;
    }

    // small (<= 8 chunks): the SpMVs skip their combine launch and the consumers fold the tile sums.  x advances with phat / shat
    // (TSL:942): the PRE form of the x update also when they come from the callback
    hipk_bi_kernels<T, PRE> pick() const {
        const bool xpre = PRE || ext;
        const double *tsum0 = A->tile_part, *tsum1 = A->tile_part + 4 * (size_t)nt;
        if (path.small)
            return {hipk_bi_supdate_kernel<T, PRE, true>, xpre ? hipk_bi_xupdate_kernel<T, true, true> : hipk_bi_xupdate_kernel<T, false, true>, tsum0,
                    tsum0, tsum1, nt};
        return {hipk_bi_supdate_kernel<T, PRE, false>, xpre ? hipk_bi_xupdate_kernel<T, true, false> : hipk_bi_xupdate_kernel<T, false, false>, part_rq,
                part_ts, part_tt, 0};
    }

    // direction, SpMV q = A phat, s update, SpMV t = A shat, x update per iteration: the host enqueues iterations a few ahead of the
    // GPU and stops when the x update reports the stop (hipk_pacer); launches past the stop are no-ops on the device
    int five_launch_sequence() {
        const hipk_bi_kernels<T, PRE> k = pick();
        hipk_spmv_args sq = hipk_spmv_base(A), stt = sq;
        sq.x = phat;
        sq.y = q;
        sq.mode = HIPK_SPMV_DOT_W;
        sq.w = rhat;
        sq.part0 = part_rq;
        sq.part1 = part_spare;
        stt.x = shat;
        stt.y = t;
        stt.mode = HIPK_SPMV_DOT_W | HIPK_SPMV_DOT_YY;
        stt.w = s;
        stt.part0 = part_ts;
        stt.part1 = part_tt;
        sq.stop_it = stt.stop_it = &scal->stop_it;
        sq.skip_combine = stt.skip_combine = path.small ? 1 : 0;
        for (; it < maxiter; ++it) {
            HIPK_CHECK_HIP(pace.gate(it, stream, &stop));
            if (stop <= it) break;
            hipk_bi_direction_kernel<T, PRE><<<gm.g, HIPK_THREADS, 0, stream>>>(n, gm.ch, gm.g, scal, it, part_rr, part_rhr, r, q, p, dinv, phat);
            if (ext) HIPK_TRY(precondition(p, phat));
            sq.it = it;
            HIPK_TRY(hipk_launch_spmv(A, sq, stream, &prof));
            k.supdate<<<gm.g, HIPK_THREADS, 0, stream>>>(n, gm.ch, gm.g, scal, it, part_rhr, k.rq, r, q, s, part_ss, dinv, shat, k.nt);
            if (ext) HIPK_TRY(precondition(s, shat));
            stt.it = it;
            HIPK_TRY(hipk_launch_spmv(A, stt, stream));
            k.xupdate<<<gm.g, HIPK_THREADS, 0, stream>>>(n, gm.ch, gm.g, scal, it, maxiter, part_ss, k.ts, k.tt, phat, s, t, rhat, x, r, part_rr, part_rhr,
                                                         shat, k.nt);
            if ((it & 31) == 31) HIPK_CHECK_HIP(hipGetLastError());
        }
        return HIPK_OK;
    }

    // TSL:1007-1014: the true residual (PRE: ||M (b - A x)||, the row scaling runs in the SpMV epilogue) and ||x|| decide info
    int finish(hipk_stats *st) {
        HIPK_CHECK_HIP(hipGetLastError());
        HIPK_TRY(residual(t, part_ss, PRE));
        if (ext) {  // ||M (b - A x)||^2 of the caller's M
            HIPK_TRY(precondition(t, phat));
            HIPK_TRY(hipk_launch_dot_parts(n, phat, phat, A->dtype, part_ss, stream));
        }
        HIPK_TRY(hipk_launch_dot_parts(n, x, x, A->dtype, part_bb, stream));
        hipk_bi_final_kernel<<<1, HIPK_THREADS, 0, stream>>>(scal, gm.g, part_ss, part_bb);
        HIPK_CHECK_HIP(hipGetLastError());
        hipk_bi_scal hs;
        HIPK_CHECK_HIP(hipEventRecord(whole.b, stream));
        HIPK_CHECK_HIP(hipMemcpyAsync(&hs, scal, sizeof(hs), hipMemcpyDeviceToHost, stream));
        HIPK_CHECK_HIP(hipStreamSynchronize(stream));

        hipk_finish_isolve_stats(st, prm, hs.bs, hs.res2, hs.xx, hs.iters, 1 + 2 * hs.iters + hs.extra_mv + 1);
        st->recurrence_rs = hs.rs_last;
        st->breakdown = hs.code;
        float ms = 0.f;
        HIPK_CHECK_HIP(hipEventElapsedTime(&ms, whole.a, whole.b));
        st->solve_ms = ms;
        HIPK_CHECK_HIP(prof.collect(st, hs.iters));
        return HIPK_OK;
    }
};

template <typename T, bool PRE>
static int hipk_bicgstab_solve_t(hipk_csr_s *A, const T *dinv, const T *b, T *x, char *work, const hipk_params *prm, hipk_stats *st,
                                 hipStream_t stream, hipk_precond_fn cb, void *user) {
    static bool mid_failed = false, lds_loop_failed = false;   // per dtype and PRE; the callback entry shares those of the plain one
    hipk_bi_steps<T, PRE> s(A, dinv, b, x, work, prm, stream, cb, user);
    HIPK_TRY(s.start());
    HIPK_TRY(s.one_launch(mid_failed, lds_loop_failed));
    if (!s.done) HIPK_TRY(s.five_launch_sequence());
    return s.finish(st);
}

// the checks and the dispatch on the operand's dtype the three entries share (have_m: the entry's dinv or M is not null)
static int hipk_bicgstab_entry(hipk_csr_t A, bool have_m, const void *dinv, hipk_precond_fn M, void *user, const void *b, void *x, void *work,
                               size_t work_bytes, const hipk_params *prm, hipk_stats *st, hipk_stream_t stream) {
    HIPK_TRY(hipk_solve_check(A, have_m, dinv, b, x, work, work_bytes, (dinv || M) ? hipk_pbicgstab_work_bytes : hipk_bicgstab_work_bytes, prm, st));
    hipStream_t s = (hipStream_t)stream;
    if (dinv)
        return A->dtype == HIPK_F64 ? hipk_bicgstab_solve_t<double, true>(A, (const double *)dinv, (const double *)b, (double *)x, (char *)work, prm, st, s, nullptr, nullptr)
                                    : hipk_bicgstab_solve_t<float, true>(A, (const float *)dinv, (const float *)b, (float *)x, (char *)work, prm, st, s, nullptr, nullptr);
    return A->dtype == HIPK_F64 ? hipk_bicgstab_solve_t<double, false>(A, nullptr, (const double *)b, (double *)x, (char *)work, prm, st, s, M, user)
                                : hipk_bicgstab_solve_t<float, false>(A, nullptr, (const float *)b, (float *)x, (char *)work, prm, st, s, M, user);
}

extern "C" int hipk_bicgstab_solve(hipk_csr_t A, const void *b, void *x, void *work, size_t work_bytes,
                                   const hipk_params *prm, hipk_stats *st, hipk_stream_t stream) {
    return hipk_bicgstab_entry(A, true, nullptr, nullptr, nullptr, b, x, work, work_bytes, prm, st, stream);
}

extern "C" int hipk_pbicgstab_solve(hipk_csr_t A, const void *dinv, const void *b, void *x, void *work, size_t work_bytes,
                                    const hipk_params *prm, hipk_stats *st, hipk_stream_t stream) {
    return hipk_bicgstab_entry(A, dinv != nullptr, dinv, nullptr, nullptr, b, x, work, work_bytes, prm, st, stream);
}

extern "C" int hipk_pbicgstab_solve_cb(hipk_csr_t A, hipk_precond_fn M, void *user, const void *b, void *x, void *work,
                                       size_t work_bytes, const hipk_params *prm, hipk_stats *st, hipk_stream_t stream) {
    return hipk_bicgstab_entry(A, M != nullptr, nullptr, M, user, b, x, work, work_bytes, prm, st, stream);
}


// =====================================================================================================================
// Row-partitioned BiCGStab, the loop of one rank in C (new against the reference, which is single-device; SURVEY 8e names CG,
// VERDICT r1 lists this as the next solver to shard).  The algorithm is `bicgstab` (TSL:859-964 via `_isolve`, TSL:968-1016) on the
// SAME five kernels as the single-GPU solve; every kernel folds the chunk partials of ALL ranks (gathered in global chunk order),
// so the iterates are bitwise those of the single-GPU solve for any rank count.  Per iteration, on the solver's stream:
//   all-gather <r,r>, <rhat,r> (one group) | K1 | halo of p | SpMV q, all-gather <rhat,q> | K3 | ONE group: all-gather <s,s> + halo
//   of s | SpMV t, all-gather <t,s>, <t,t> (one group) | K5
// -- five collective launches (CG: two).  Conventions of hipk_dist_cg_solve (csrc/hipk_dist.hip): fixed batches, the stop word
// read one batch late, identical decisions on all ranks without an agreement collective.
// PRE (hipk_dist_pbicgstab_solve, M = diag(dinv)): the PRE instances of K1 / K3 / K5 as in hipk_pbicgstab_solve; the SpMVs multiply
// phat = dinv .* p and shat = dinv .* s, so their halos are exchanged instead of those of p and s (ghost values: the owner's bits),
// and `info` comes from ||M (b - A x)|| (the scaled residual SpMV).  The same five collective launches per iteration.
#include "hipk_dist_xchg.h"

struct hipk_dbi_layout {
    size_t scal, part_a, part_b, spare, g_rr, g_rhr, g_rq, g_ss, g_ts, g_tt, g_bb, out4, send_buf, slab_loc, slab_all;
    size_t r, rhat, p, q, s, t, phat, shat, total;
};
static hipk_dbi_layout hipk_dbi_make_layout(const hipk_dist_plan *pl, bool pre) {
    hipk_dbi_layout L;
    hipk_carve take;
    const size_t per = (size_t)pl->per, W = (size_t)pl->world;
    const size_t next = (size_t)(pl->n_ext > 0 ? pl->n_ext : 1), nloc = (size_t)(pl->n_local > 0 ? pl->n_local : 1);
    L.scal = take(256);
    L.part_a = take(per * 8);
    L.part_b = take(per * 8);
    L.spare = take(per * 8);
    L.g_rr = take(W * per * 8);
    L.g_rhr = take(W * per * 8);
    L.g_rq = take(W * per * 8);
    L.g_ss = take(W * per * 8);
    L.g_ts = take(W * per * 8);
    L.g_tt = take(W * per * 8);
    L.g_bb = take(W * per * 8);
    L.out4 = take(4 * 8);
    L.send_buf = take((size_t)(pl->n_send > 0 ? pl->n_send : 1) * 8);
    L.slab_loc = take((size_t)(pl->slab > 0 ? pl->slab : 1) * 8);
    L.slab_all = take((size_t)(pl->slab > 0 ? pl->slab : 1) * W * 8);
    L.r = take(nloc * 8);
    L.rhat = take(nloc * 8);
    L.p = take(next * 8);
    L.q = take(nloc * 8);
    L.s = take(next * 8);
    L.t = take(next * 8);   // also the x-halo scratch of the residual SpMVs
    L.phat = pre ? take(next * 8) : L.p;   // PRE: the SpMV inputs, with their halo tails
    L.shat = pre ? take(next * 8) : L.s;
    L.total = take.o;
    return L;
}
extern "C" size_t hipk_dist_bicgstab_work_bytes(const hipk_dist_plan *plan) {
    if (!plan || plan->world < 1 || plan->per < 1) return 0;
    return hipk_dbi_make_layout(plan, false).total;
}
extern "C" size_t hipk_dist_pbicgstab_work_bytes(const hipk_dist_plan *plan) {
    if (!plan || plan->world < 1 || plan->per < 1) return 0;
    return hipk_dbi_make_layout(plan, true).total;
}

template <bool PRE>
static int hipk_dist_bicgstab_t(hipk_csr_t A, const hipk_dist_plan *pl, const hipk_rccl *cc, const double *dinv, const void *b_local,
                                void *x_ext, void *work, size_t work_bytes, const hipk_params *prm, hipk_stats *st, hipk_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    HIPK_TRY(hipk_dist_check(A, pl, cc, PRE, dinv, b_local, x_ext, work, prm, st));
    const hipk_dbi_layout L = hipk_dbi_make_layout(pl, PRE);
    HIPK_REQUIRE(work_bytes >= L.total, HIPK_ERR_WORKSPACE, "work too small");
    memset(st, 0, sizeof(*st));
    typedef double T;
    char *wk = (char *)work;
    hipk_bi_scal *scal = (hipk_bi_scal *)(wk + L.scal);
    double *part_a = (double *)(wk + L.part_a), *part_b = (double *)(wk + L.part_b), *spare = (double *)(wk + L.spare);
    double *g_rr = (double *)(wk + L.g_rr), *g_rhr = (double *)(wk + L.g_rhr), *g_rq = (double *)(wk + L.g_rq);
    double *g_ss = (double *)(wk + L.g_ss), *g_ts = (double *)(wk + L.g_ts), *g_tt = (double *)(wk + L.g_tt);
    double *g_bb = (double *)(wk + L.g_bb), *out4 = (double *)(wk + L.out4);
    T *r = (T *)(wk + L.r), *rhat = (T *)(wk + L.rhat), *p = (T *)(wk + L.p), *q = (T *)(wk + L.q), *s = (T *)(wk + L.s);
    T *t = (T *)(wk + L.t), *phat = (T *)(wk + L.phat), *shat = (T *)(wk + L.shat);   // (= p, s without PRE)
    T *x = (T *)x_ext;
    const T *b = (const T *)b_local;
    const int64_t n = pl->n_local, n_ext = pl->n_ext;
    const int ch = pl->chunk_rows, G = pl->g_red, per = pl->per, W = pl->world;
    const int grid = (int)((n + ch - 1) / ch);
    const int64_t maxiter = hipk_default_maxiter(prm, pl->n_global);
    const hipk_tol_sq tol(prm);
    const int64_t *stop_dev = &scal->stop_it;
    // grouped(): each exchange of the loop is one group at world > 1, whatever it carries
    const hipk_dist_xchg xc(pl, cc, stream, (double *)(wk + L.send_buf), (double *)(wk + L.slab_loc), (double *)(wk + L.slab_all),
                            PRE ? "hipk_dist_pbicgstab_solve" : "hipk_dist_bicgstab_solve");

    hipk_event_pair whole;
    HIPK_CHECK_HIP(whole.create());
    HIPK_CHECK_HIP(hipEventRecord(whole.a, stream));
    HIPK_CHECK_HIP(hipMemsetAsync(wk, 0, L.total, stream));
    if (n_ext > n) HIPK_CHECK_HIP(hipMemsetAsync(x + n, 0, (size_t)(n_ext - n) * 8, stream));

    // ---- r0 = b - A x0 with <r0,r0>; <b,b>; rhat = p = q = r0, <rhat,r0> = <r0,r0>   (TSL:870-890)
    // (x carries its halo tail for the residual forms; t doubles as nothing here: x_ext is the caller's n_ext vector)
    HIPK_TRY(xc.grouped(x, nullptr, nullptr));
    HIPK_TRY(hipk_spmv_ex(A, x, r, HIPK_SPMV_RESID | HIPK_SPMV_DOT_YY, nullptr, b, spare, part_a, nullptr, 0, stream));
    HIPK_TRY(xc.parts(part_a, g_rr));
    HIPK_TRY(hipk_dot_parts(n, ch, b, b, HIPK_F64, part_a, stream));
    HIPK_TRY(xc.parts(part_a, g_bb));
    HIPK_CHECK_HIP(hipMemcpyAsync(g_rhr, g_rr, (size_t)W * per * 8, hipMemcpyDeviceToDevice, stream));
    hipk_bi_start_kernel<T><<<grid, HIPK_THREADS, 0, stream>>>(n, ch, G, scal, g_rr, g_bb, spare, r, rhat, p, q, tol.tol2, tol.atol_sq, maxiter,
                                                                nullptr);
    HIPK_CHECK_HIP(hipGetLastError());

    // ---- the loop: fixed batches, the stop word read one batch late (hipk_dist_batches)
    int64_t it = 0, stop = INT64_MAX;
    HIPK_TRY(hipk_dist_batches(prm, A->host_poll, stop_dev, maxiter, stream, it, stop, [&](int64_t it) -> int {
        hipk_bi_direction_kernel<T, PRE><<<grid, HIPK_THREADS, 0, stream>>>(n, ch, G, scal, it, g_rr, g_rhr, r, q, p, dinv, phat);
        HIPK_TRY(xc.grouped(phat, nullptr, nullptr));
        HIPK_TRY(hipk_spmv_ex(A, phat, q, HIPK_SPMV_DOT_W, rhat, nullptr, part_a, spare, stop_dev, it, stream));
        HIPK_TRY(xc.parts(part_a, g_rq));
        hipk_bi_supdate_kernel<T, PRE, false><<<grid, HIPK_THREADS, 0, stream>>>(n, ch, G, scal, it, g_rhr, g_rq, r, q, s, part_a,
                                                                                dinv, shat, 0);
        HIPK_TRY(xc.grouped(shat, part_a, g_ss));
        HIPK_TRY(hipk_spmv_ex(A, shat, t, HIPK_SPMV_DOT_W | HIPK_SPMV_DOT_YY, s, nullptr, part_a, part_b, stop_dev, it, stream));
        HIPK_TRY(xc.grouped(nullptr, part_a, g_ts, part_b, g_tt));
        hipk_bi_xupdate_kernel<T, PRE, false><<<grid, HIPK_THREADS, 0, stream>>>(n, ch, G, scal, it, maxiter, g_ss, g_ts, g_tt, phat, s,
                                                                                t, rhat, x, r, part_a, part_b, shat, 0);
        return xc.grouped(nullptr, part_a, g_rr, part_b, g_rhr);
    }));

    // ---- TSL:1007-1014: true residual (PRE: ||M (b - A x)||, the row scaling in the SpMV epilogue) and ||x|| decide info
    HIPK_TRY(xc.grouped(x, nullptr, nullptr));
    HIPK_TRY(hipk_dist_spmv(A, x, t, HIPK_SPMV_RESID | HIPK_SPMV_DOT_YY, nullptr, b, dinv, spare, part_a, nullptr, 0, stream));
    HIPK_TRY(xc.parts(part_a, g_ss));
    HIPK_TRY(hipk_reduce_parts(g_ss, G, out4 + 0, stream));
    HIPK_TRY(hipk_dot_parts(n, ch, x, x, HIPK_F64, part_a, stream));
    HIPK_TRY(xc.parts(part_a, g_ts));
    HIPK_TRY(hipk_reduce_parts(g_ts, G, out4 + 1, stream));
    HIPK_TRY(hipk_reduce_parts(g_bb, G, out4 + 2, stream));
    double h4[4] = {0, 0, 0, 0};
    hipk_bi_scal hs;
    HIPK_CHECK_HIP(hipEventRecord(whole.b, stream));
    HIPK_CHECK_HIP(hipMemcpyAsync(h4, out4, sizeof(h4), hipMemcpyDeviceToHost, stream));
    HIPK_CHECK_HIP(hipMemcpyAsync(&hs, scal, sizeof(hs), hipMemcpyDeviceToHost, stream));
    HIPK_CHECK_HIP(hipStreamSynchronize(stream));
    hipk_finish_isolve_stats(st, prm, h4[2], h4[0], h4[1], hs.iters, 1 + 2 * hs.iters + hs.extra_mv + 1);
    st->recurrence_rs = hs.rs_last;
    st->breakdown = hs.code;
    float ms = 0.f;
    HIPK_CHECK_HIP(hipEventElapsedTime(&ms, whole.a, whole.b));
    st->solve_ms = ms;
    return HIPK_OK;
}

extern "C" int hipk_dist_bicgstab_solve(hipk_csr_t A, const hipk_dist_plan *pl, const hipk_rccl *cc, const void *b_local, void *x_ext,
                                        void *work, size_t work_bytes, const hipk_params *prm, hipk_stats *st, hipk_stream_t stream) {
    return hipk_dist_bicgstab_t<false>(A, pl, cc, nullptr, b_local, x_ext, work, work_bytes, prm, st, stream);
}

extern "C" int hipk_dist_pbicgstab_solve(hipk_csr_t A, const hipk_dist_plan *pl, const hipk_rccl *cc, const void *dinv,
                                         const void *b_local, void *x_ext, void *work, size_t work_bytes, const hipk_params *prm,
                                         hipk_stats *st, hipk_stream_t stream) {
    return hipk_dist_bicgstab_t<true>(A, pl, cc, (const double *)dinv, b_local, x_ext, work, work_bytes, prm, st, stream);
}
