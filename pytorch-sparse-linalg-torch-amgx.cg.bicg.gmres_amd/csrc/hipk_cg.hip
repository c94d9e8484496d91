// hipk_cg.hip -- device-resident conjugate gradient.
//
// Restates `_isolve(_cg_solve)` (TSL:806-856, 968-1016) for M = identity as three
// kernels per iteration, all scalars living in device memory:
//   K1 spmv+dot   Ap = A p, partials of <p,Ap>            (TSL:845-846)   B_spmv
//   K2 update     alpha = gamma/<p,Ap>; r -= alpha Ap; partials of <r,r>
//                                                          (TSL:846, 848-850)   24 n bytes
//   K3 direction  alpha again (same partials, same bits), beta = <r,r>/gamma; x += alpha p; p = r + beta p;
//                 gamma <- <r,r>; stop test                (TSL:847, 851-853, 841) 40 n bytes
// = B_spmv + 64 n bytes per iteration: the x update rides on the pass that already streams p, 8 n bytes
// less than the 72 n of SURVEY 8d; the arithmetic per element is unchanged.
// Cache-resident sizes beyond the one-launch loops (the headline among them) defer the x update: nothing reads x before the solve
// ends, so K3 alternates between hipk_cg_pdir_kernel (p = r + beta p into a SECOND p buffer: 24 n bytes) and hipk_cg_xdir_kernel
// (the same, and x = (x + alpha_{k-1} p_{k-1}) + alpha_k p_k for two iterations at once, in the reference's order and with its
// roundings: 48 n bytes), with the alphas from the scalar block (K2 leaves them there) -- B_spmv + 60 n bytes per iteration on
// average; hipk_cg_xflush_kernel after the loop adds the term an odd iteration count leaves owed.
// On fp64 constant-coefficient stencils of those sizes K1 and K2 are ONE launch, hipk_cg_fuse_update_kernel (hipk_cg_fuse.h): Ap stays in
// LDS, <p,Ap> crosses the workgroups inside the launch -- B_spmv - 8 n + 16 n bytes instead of B_spmv + 24 n.
// With the x update deferred that launch also does K3 (its direction tail: <r,r> crosses the workgroups the same way, r_{k+1} is
// still in registers): ONE launch per iteration, 16 n bytes for a p-only step and 40 n for one with x instead of 24 n and 48 n --
// B_spmv + 36 n bytes per iteration on average.
// Every workgroup re-derives alpha/beta from the chunk
// partials of the previous kernel with the fixed tree, so no grid barrier, no atomics
// and no host round trip are needed; the host follows the loop through a pinned word the direction kernel
// stores to (hipk_pacer, hipk_solve.h) and the kernels of iterations >= stop_it return immediately, so the
// solve stops at exactly the iteration the reference stops at.
#include <type_traits>
#include <math.h>
#include <stdlib.h>

#include <vector>

#include "hipk_blas1.h"
#include "hipk_solve.h"
#include "hipk_spmv.h"
#include "hipk_handoff.h"
#include "hipk_fx.h"

// progress / placement block of the one-launch loops (hipk_cg_solve_lds_kernel), zeroed before each launch
struct hipk_lds_ctl {
    double rs_last;    // <r,r> of the last finished iteration
    int64_t it_done;   // iterations finished when the launch returned
    int32_t redo;      // < 0: its resident workgroups did not all arrive / were spread over several XCDs (nothing was modified)
    int32_t bar;       // counter barrier of its placement check
    unsigned xcc_mask;
    unsigned pad;
};
struct hipk_cg_scal {
    double gamma[2];   // <r,r> ping-pong by iteration parity
    double atol2;      // max(tol^2 <b,b>, atol^2)            (TSL:815-817)
    double bs;         // <b,b>
    double res2;       // true ||b - A x||^2 after the loop  (TSL:1008)
    double xx;         // <x,x>                               (TSL:1013)
    int64_t stop_it;   // iterations >= stop_it are no-ops
    int64_t *host_sig; // pinned host word the direction kernel reports to (hipk_pacer), or null
    union {
        struct {
            double dir_alpha;  // hipk_cg_scalars_kernel -> hipk_cg_direction_flat_kernel (streaming policy): gamma / <p,Ap>, <r,r> / gamma
            double dir_beta;
        };
        // deferred x update (never together with the streaming policy, so the two share their words and the block keeps its
        // size): alpha of iteration k, the value (T)(gamma / <p,Ap>) every consumer derives, in slot k & 1 -- stored by the
        // update launch of iteration k, read by hipk_cg_xdir_kernel and hipk_cg_xflush_kernel
        double alpha[2];
    };
    hipk_lds_ctl ctl;  // hipk_cg_solve_lds_kernel (small systems: the whole loop in one launch)
};
static_assert(sizeof(hipk_cg_scal) <= 256, "the scalar block is 256 bytes");
#include "hipk_cg_mid.h"   // one-launch loop for mid-size systems (uses hipk_lds_ctl)
// the bookkeeping of every deferred-x K3 and of the fused launch's direction tail (hipk_cg_fuse.h, hence up here): gamma of the
// next pass, the stop test, the host's signal word (TSL:853, 841)
__device__ __forceinline__ void hipk_cg_dir_done(hipk_cg_scal *scal, int64_t it, int64_t maxiter, double rr) {
    scal->gamma[(it + 1) & 1] = rr;  // TSL:853
    // TSL:841 for the NEXT pass: stop when k+1 >= maxiter or rs <= atol2 (workgroups of THIS launch compare against `it`)
    const bool done = (it + 1 >= maxiter || rr <= scal->atol2);
    if (done) scal->stop_it = it + 1;
    hipk_signal(scal->host_sig, done ? (HIPK_SIG_STOP | (it + 1)) : (it + 1));
}
#include "hipk_cg_fuse.h"  // the stencil SpMV and the update step in one launch (uses hipk_cg_scal)

// gamma0 = <r0,r0>, bs = <b,b>, atol2; p = r0.
template <typename T>
__global__ __launch_bounds__(HIPK_THREADS) void hipk_cg_start_kernel(
    int64_t n, int ch, int g, hipk_cg_scal *__restrict__ scal, const double *__restrict__ part_rr,
    const double *__restrict__ part_bb, const T *__restrict__ r, T *__restrict__ p, double tol2, double atol_sq,
    int64_t maxiter, int64_t *host_sig = nullptr) {
    __shared__ double sbuf[2 * HIPK_THREADS];
    double gamma0, bs;
    hipk_reduce_parts2(part_rr, part_bb, g, gamma0, bs, sbuf);  // g = partial count of ALL ranks
    const int c = blockIdx.x;
    hipk_chunk_loop<T>(n, ch, c, [&](int64_t i, int nv) {
        T rv[hipk_vec<T>::VEC];
        hipk_ld<T>(r, i, nv, rv);
        hipk_st<T>(p, i, nv, rv);
    });
    if (c == 0 && threadIdx.x == 0) {
        const double a2 = tol2 * bs;
        const double atol2 = (a2 > atol_sq) ? a2 : atol_sq;  // torch.maximum: NaN-propagation irrelevant here
        scal->gamma[0] = gamma0;
        scal->gamma[1] = 0.0;
        scal->atol2 = atol2;
        scal->bs = bs;
        // TSL:841: `if k >= maxiter or rs <= atol2: break` evaluated before the first SpMV
        const bool done = (maxiter <= 0 || gamma0 <= atol2);
        scal->stop_it = done ? 0 : INT64_MAX;
        scal->host_sig = host_sig;
        if (done) hipk_signal(host_sig, HIPK_SIG_STOP);
    }
}

// The two per-iteration vector kernels run as ONE wave of workgroups (a chunk each, <= 2048 of them on 2048
// slots), so whatever a workgroup does before its first vector load is exposed in full: the stop word, the
// partial sums and the fold's barriers.  Both kernels therefore request the first HIPK_BASE_CHUNK elements of
// two operands BEFORE reading the stop word and folding the partials (hipk_pre, hipk_blas1.h; no store happens
// until the stop test has passed).  Order of operations per element is unchanged.
// SMALL (systems of <= 8 reduction chunks, launch-bound): <p,Ap> is folded here from the SpMV's per-wavefront tile
// sums (hipk_fold_tiles8: part_pAp then points at them, `ntiles` tiles), the combine launch is skipped.
// NT (systems whose CG working set -- x, r, p, Ap -- is far beyond the Infinity Cache): every vector is a stream.
// alpha_out (the deferred x update follows: &scal->alpha[it & 1], words this kernel does not read): one thread leaves alpha there.
template <typename T, bool SMALL = false, bool NT = false>
__global__ __launch_bounds__(HIPK_THREADS) void hipk_cg_update_kernel(
    int64_t n, int ch, int g, const hipk_cg_scal *__restrict__ scal, int64_t it,
    const double *__restrict__ part_pAp, const T *__restrict__ Ap, T *__restrict__ r, double *__restrict__ part_rr,
    int ntiles = 0, double *__restrict__ alpha_out = nullptr) {
    const int c = blockIdx.x;
    hipk_pre<T, 2, NT> pre;
    pre.issue(n, ch, c, {Ap, (const T *)r});
    if (it >= scal->stop_it) return;
    __shared__ double sbuf[HIPK_THREADS];
    const double pAp = SMALL ? hipk_fold_tiles8(part_pAp, ntiles, ch / HIPK_TILE, g, sbuf)
                             : hipk_reduce_parts(part_pAp, g, sbuf);
    const double gamma = scal->gamma[it & 1];
    const T alpha = (T)(gamma / pAp);  // TSL:846
    if (alpha_out != nullptr && c == 0 && threadIdx.x == 0) *alpha_out = (double)alpha;
    double acc = 0.0;
    pre.run([&](int64_t i, int nv, T(&v)[2][hipk_vec<T>::VEC]) {
        constexpr int VEC = hipk_vec<T>::VEC;
        T rv[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const T m1 = alpha * v[0][k];
            rv[k] = v[1][k] - m1;  // TSL:848
            if (k < nv) acc = fma((double)rv[k], (double)rv[k], acc);  // TSL:850
        }
        hipk_st<T>(r, i, nv, rv);
    });
    acc = hipk_block_sum(acc, sbuf);
    if (threadIdx.x == 0) part_rr[c] = acc;
}

// NOX: p only -- the row-partitioned solver with the x update on a side stream (hipk_cg_xupdate_kernel).  A compile-time switch:
// as a run-time branch it cost the hot instantiation its 8 workgroups per CU (74 VGPRs: 22.6 -> 25.4 us at N = 4 M).
template <typename T, bool SMALL = false, bool NT = false, bool NOX = false>
__global__ __launch_bounds__(HIPK_THREADS) void hipk_cg_direction_kernel(
    int64_t n, int ch, int g, hipk_cg_scal *__restrict__ scal, int64_t it, int64_t maxiter,
    const double *__restrict__ part_pAp, const double *__restrict__ part_rr, const T *__restrict__ r,
    T *__restrict__ p, T *__restrict__ x, int ntiles = 0) {
    const int c = blockIdx.x;
    // r and p are requested up front; x (needed last) is loaded step by step after the fold: all three would
    // take 76 VGPRs and drop the kernel to 6 workgroups per CU (1536 slots < 1954 chunks: a second round)
    // streaming policy (NT): x is the third batched operand, two steps per batch (instead of a load inside the step, behind the
    // previous step's stores); same-box A/B at N = 64 M: 457 vs 464 us, no gain (profiles/r02_vector_tail_ab.txt)
    typename std::conditional<NT && !NOX, hipk_pre<T, 3, true, 2>, hipk_pre<T, 2, NT>>::type pre;
    if constexpr (NT && !NOX) pre.issue(n, ch, c, {r, (const T *)p, (const T *)x});
    else pre.issue(n, ch, c, {r, (const T *)p});
    if (it >= scal->stop_it) return;
    __shared__ double sbuf[2 * HIPK_THREADS];
    double pAp, rr;
    if (SMALL) {
        pAp = hipk_fold_tiles8(part_pAp, ntiles, ch / HIPK_TILE, g, sbuf);
        rr = hipk_reduce_parts(part_rr, g, sbuf);
    } else {
        hipk_reduce_parts2(part_pAp, part_rr, g, pAp, rr, sbuf);
    }
    const double gamma = scal->gamma[it & 1];
    const T alpha = (T)(gamma / pAp);  // TSL:846, the same bits hipk_cg_update_kernel derived
    const T beta = (T)(rr / gamma);    // TSL:851
    if constexpr (NOX) {
        pre.run([&](int64_t i, int nv, T(&v)[2][hipk_vec<T>::VEC]) {
            constexpr int VEC = hipk_vec<T>::VEC;
            T pv[VEC];
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const T m = beta * v[1][k];
                pv[k] = v[0][k] + m;  // TSL:852
            }
            hipk_st<T>(p, i, nv, pv);
        });
    } else if constexpr (NT) {
        pre.run([&](int64_t i, int nv, T(&v)[3][hipk_vec<T>::VEC]) {
            constexpr int VEC = hipk_vec<T>::VEC;
            T xv[VEC], pv[VEC];
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const T m0 = alpha * v[1][k];
                xv[k] = v[2][k] + m0;  // TSL:847 (with the p of this iteration, before it is replaced)
                const T m = beta * v[1][k];
                pv[k] = v[0][k] + m;  // TSL:852
            }
            hipk_st_nt_vec<T>(x, i, nv, xv);  // x is not read again before the next direction kernel
            hipk_st<T>(p, i, nv, pv);
        });
    } else {
        pre.run([&](int64_t i, int nv, T(&v)[2][hipk_vec<T>::VEC]) {
            constexpr int VEC = hipk_vec<T>::VEC;
            T xv[VEC], pv[VEC];
            hipk_ld<T>((const T *)x, i, nv, xv);
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const T m0 = alpha * v[1][k];
                xv[k] = xv[k] + m0;  // TSL:847 (with the p of this iteration, before it is replaced)
                const T m = beta * v[1][k];
                pv[k] = v[0][k] + m;  // TSL:852
            }
            hipk_st<T>(x, i, nv, xv);
            hipk_st<T>(p, i, nv, pv);
        });
    }
    if (c == 0 && threadIdx.x == 0) {
        scal->gamma[(it + 1) & 1] = rr;  // TSL:853
        // TSL:841 for the NEXT pass: stop when k+1 >= maxiter or rs <= atol2.
        // Workgroups of THIS launch compare against `it`, so they are unaffected.
        const bool done = (it + 1 >= maxiter || rr <= scal->atol2);
        if (done) scal->stop_it = it + 1;
        hipk_signal(scal->host_sig, done ? (HIPK_SIG_STOP | (it + 1)) : (it + 1));
    }
}

// ---- K3 with the x update deferred (the three-launch sequence of cache-resident sizes; hipk_cg_solve_t drives them) ------------
// Nothing reads x before the solve ends, so x is updated every SECOND iteration for two iterations at once, in the reference's
// order and with its roundings: x = (x + alpha_{k-1} p_{k-1}) + alpha_k p_k, each product and each sum rounded on its own -- the
// bits two successive `x += alpha p` give.  p ping-pongs between two buffers so that p_{k-1} is still there; the alphas come from
// scal->alpha (hipk_cg_update_kernel's alpha_out), so no K3 folds part_pAp.

// hipk_reduce_parts with this thread's partials requested EARLY, all at once: the fold's own loads are eight dependent round trips
// when each waits for the one before (the compiler does not hoist a load out of its `i < g`), and a wait for any of them is a
// wait for every vector access issued before it.  Clamped indices make the loads unconditional; the sum skips what the original
// skips, so the bits are hipk_reduce_parts'.
struct hipk_parts_pre {
    static constexpr int NK = HIPK_MAX_PARTS / HIPK_THREADS;
    double v[NK];
    __device__ __forceinline__ void issue(const double *__restrict__ part, int g) {
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const int i = threadIdx.x + k * HIPK_THREADS;
            v[k] = part[i < g ? i : g - 1];
        }
    }
    __device__ __forceinline__ double fold(int g, double *sbuf) const {
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < NK; ++k)
            if ((int)threadIdx.x + k * HIPK_THREADS < g) acc = acc + v[k];
        return hipk_block_sum(acc, sbuf);
    }
};

// One chunk of either K3.  XUP: also the x update.  FULL: the chunk has all of its first HIPK_BASE_CHUNK elements (every chunk but
// a ragged last one): they go through registers, N0 steps per thread, without a validity count per step; the rest of a larger
// chunk (n > 4 M rows), and a ragged chunk from its start, step by step as hipk_pre::run's tail.  The chunk is addressed through
// uniform base pointers and 32-bit element offsets (rb, pb, qb, xb: r, p_k, the other p buffer, x at the chunk's first element):
// with 64-bit indices and counts per thread the three operands of four steps (48 registers in fp64) did not leave room for 8
// workgroups per CU.  FULL is a compile-time branch of the whole body so that each form counts its own loads in flight.
//   p only:  r and p_k are requested, then the partials: the fold's first wait is for all of them, the rest of it is LDS only.
//   with x:  x, p_{k-1}, p_k are requested first; the x part needs the two alphas only, so its stores leave before the fold, r
//            is requested into the registers of p_{k-1}, the partials into those of x: the fold's first wait is for the x stores
//            and r, the rest of it is LDS only.  qb holds p_{k-1} and receives p_{k+1}: every thread reads its elements first.
template <typename T, bool XUP, bool FULL>
__device__ __forceinline__ void hipk_cg_dir_chunk(int lim, int g, hipk_cg_scal *__restrict__ scal, int64_t it, int64_t maxiter,
                                                  const double *__restrict__ part_rr, const T *__restrict__ rb, const T *__restrict__ pb,
                                                  T *qb, T *xb, double *sbuf, bool lead, int64_t stop, double gamma, T alpha_prev, T alpha) {
    constexpr int VEC = hipk_vec<T>::VEC;
    constexpr int N0 = HIPK_BASE_CHUNK / (VEC * HIPK_THREADS);
    constexpr unsigned STEP = VEC * HIPK_THREADS;
    const unsigned o0 = VEC * threadIdx.x;
    hipk_parts_pre parts;
    T xv[N0][VEC], qv[N0][VEC], pv[N0][VEC];
    T (&rv)[N0][VEC] = qv;   // with x: r arrives where p_{k-1} was
    if constexpr (FULL) {
#pragma unroll
        for (int k = 0; k < N0; ++k) {
            const unsigned o = o0 + k * STEP;
            if constexpr (XUP) {
                hipk_ld<T>((const T *)xb, o, VEC, xv[k]);
                hipk_ld<T>((const T *)qb, o, VEC, qv[k]);
            } else {
                hipk_ld<T>(rb, o, VEC, rv[k]);
            }
            hipk_ld<T>(pb, o, VEC, pv[k]);
        }
    }
    if (it >= stop) return;
    if constexpr (XUP) {
        if constexpr (FULL) {
#pragma unroll
            for (int k = 0; k < N0; ++k) {
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    const T m0 = alpha_prev * qv[k][e];
                    const T x1 = xv[k][e] + m0;   // TSL:847 of iteration it - 1
                    const T m1 = alpha * pv[k][e];
                    xv[k][e] = x1 + m1;           // TSL:847 of iteration it
                }
                hipk_st<T>(xb, o0 + k * STEP, VEC, xv[k]);
            }
#pragma unroll
            for (int k = 0; k < N0; ++k) hipk_ld<T>(rb, o0 + k * STEP, VEC, rv[k]);
        }
    }
    // (the instruction scheduler otherwise starts the fold between the chunk's loads, and the last of them wait for the first)
    __builtin_amdgcn_sched_barrier(0);
    parts.issue(part_rr, g);
    const double rr = parts.fold(g, sbuf);          // the tree of hipk_reduce_parts2: the direction kernel's bits
    const T beta = (T)(rr / gamma);                 // TSL:851
    if constexpr (FULL) {
#pragma unroll
        for (int k = 0; k < N0; ++k) {
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const T m = beta * pv[k][e];
                pv[k][e] = rv[k][e] + m;  // TSL:852
            }
            hipk_st<T>(qb, o0 + k * STEP, VEC, pv[k]);
        }
    }
    for (unsigned o = o0 + (FULL ? N0 * STEP : 0u); (int)o < lim; o += STEP) {
        const int nv = (lim - (int)o < VEC) ? lim - (int)o : VEC;
        T xs[VEC], qs[VEC], ps[VEC], rs[VEC];
        if constexpr (XUP) {
            hipk_ld<T>((const T *)xb, o, nv, xs);
            hipk_ld<T>((const T *)qb, o, nv, qs);
        }
        hipk_ld<T>(pb, o, nv, ps);
        hipk_ld<T>(rb, o, nv, rs);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            if constexpr (XUP) {
                const T m0 = alpha_prev * qs[e];
                const T x1 = xs[e] + m0;
                const T m1 = alpha * ps[e];
                xs[e] = x1 + m1;
            }
            const T m = beta * ps[e];
            ps[e] = rs[e] + m;
        }
        if constexpr (XUP) hipk_st<T>(xb, o, nv, xs);
        hipk_st<T>(qb, o, nv, ps);
    }
    if (lead) hipk_cg_dir_done(scal, it, maxiter, rr);
}

template <typename T, bool XUP>
__device__ __forceinline__ void hipk_cg_dir_deferred(int64_t n, int ch, int g, hipk_cg_scal *__restrict__ scal, int64_t it, int64_t maxiter,
                                                     const double *__restrict__ part_rr, const T *__restrict__ r, const T *__restrict__ p_cur,
                                                     T *p_other, T *x) {
    __shared__ double sbuf[HIPK_THREADS];
    const int c = blockIdx.x;
    const int64_t base = (int64_t)c * ch;
    const int lim = (int)((base + ch < n) ? ch : n - base);   // elements of this chunk
    const bool lead = c == 0 && threadIdx.x == 0;
    // the scalars are requested here (scalar loads, before the two forms part) and looked at after the chunk's loads have been issued
    const int64_t stop = scal->stop_it;
    const double gamma = scal->gamma[it & 1];
    // TSL:846 of iterations it - 1 and it, the bits the update kernels derived
    const T alpha_prev = XUP ? (T)scal->alpha[(it - 1) & 1] : (T)0, alpha = XUP ? (T)scal->alpha[it & 1] : (T)0;
    if (lim >= HIPK_BASE_CHUNK)
        hipk_cg_dir_chunk<T, XUP, true>(lim, g, scal, it, maxiter, part_rr, r + base, p_cur + base, p_other + base, XUP ? x + base : x, sbuf, lead, stop, gamma, alpha_prev, alpha);
    else
        hipk_cg_dir_chunk<T, XUP, false>(lim, g, scal, it, maxiter, part_rr, r + base, p_cur + base, p_other + base, XUP ? x + base : x, sbuf, lead, stop, gamma, alpha_prev, alpha);
}

// iterations that only form p: p_next = r + beta p_cur into the OTHER buffer (3 passes instead of 5)
template <typename T>
__global__ __launch_bounds__(HIPK_THREADS) void hipk_cg_pdir_kernel(int64_t n, int ch, int g, hipk_cg_scal *__restrict__ scal, int64_t it,
                                                                    int64_t maxiter, const double *__restrict__ part_rr,
                                                                    const T *__restrict__ r, const T *__restrict__ p_cur,
                                                                    T *__restrict__ p_next) {
    hipk_cg_dir_deferred<T, false>(n, ch, g, scal, it, maxiter, part_rr, r, p_cur, p_next, (T *)nullptr);
}

// iterations that also update x (6 passes): x = (x + alpha_{k-1} p_{k-1}) + alpha_k p_k.  pq holds p_{k-1} and receives p_{k+1}:
// one pointer, not restrict against itself
template <typename T>
__global__ __launch_bounds__(HIPK_THREADS) void hipk_cg_xdir_kernel(int64_t n, int ch, int g, hipk_cg_scal *__restrict__ scal, int64_t it,
                                                                    int64_t maxiter, const double *__restrict__ part_rr,
                                                                    const T *__restrict__ r, const T *__restrict__ p_cur, T *pq,
                                                                    T *__restrict__ x) {
    hipk_cg_dir_deferred<T, true>(n, ch, g, scal, it, maxiter, part_rr, r, p_cur, pq, x);
}

// after the loop: K iterations were completed (the device's stop word once it has fired, else the host's count), the deferred
// sequence began at it0.  K - it0 odd: iteration K - 1 only formed p, x still lacks alpha_{K-1} p_{K-1} -- and p_{K-1} sits in the
// buffer the sequence began with (K - 1 - it0 is even; the launches past the stop were no-ops).  Even, or K <= it0: nothing to do.
template <typename T>
__global__ __launch_bounds__(HIPK_THREADS) void hipk_cg_xflush_kernel(int64_t n, int ch, const hipk_cg_scal *__restrict__ scal, int64_t it_host,
                                                                      int64_t it0, const T *__restrict__ p_first, T *__restrict__ x,
                                                                      int dir_tail = 0) {
    // (the direction tail of the fused launch gave up: iteration stop_it is half done, hipk_cg_steps::fuse_end settles x)
    if (dir_tail && scal->ctl.redo == kFuseDirGaveUp) return;
    const int64_t stop = scal->stop_it;
    const int64_t K = stop < it_host ? stop : it_host;
    if (K <= it0 || ((K - it0) & 1) == 0) return;
    const T alpha = (T)scal->alpha[(K - 1) & 1];
    hipk_chunk_loop<T>(n, ch, blockIdx.x, [&](int64_t i, int nv) {
        constexpr int VEC = hipk_vec<T>::VEC;
        T xv[VEC], pv[VEC];
        hipk_ld<T>((const T *)x, i, nv, xv);
        hipk_ld<T>(p_first, i, nv, pv);
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const T m0 = alpha * pv[k];
            xv[k] = xv[k] + m0;  // TSL:847
        }
        hipk_st<T>(x, i, nv, xv);
    });
}

// ---- TWO launches per iteration for launch-bound mid-size systems (33 .. 150 reduction chunks: 65 k < n <= 307 k) ----------------
// Above the one-launch kernels' size an iteration of three launches costs ~15 us whatever the three kernels move (a dependent
// launch is ~4.5 us end to end on MI355X: hipk_tile_combine_kernel, one wavefront per chunk, averages 4.6 us in the profiles).
// The direction step is folded into the SpMV: K1(k) folds <r,r> of iteration k-1 (every workgroup, the same bits), does the stop
// test and the gamma bookkeeping, forms p_k = r + beta p_{k-1} ON THE FLY at the gathered columns (the owner's formula on the
// owner's operands: the bits the direction kernel would have stored), writes its own rows of p_k into the OTHER p buffer and
// Ap_k, and leaves the per-wavefront tile sums of <p_k, Ap_k>; K2(k) folds them, alpha, x += alpha p_k, r -= alpha Ap_k, <r,r>
// partials.  Same operations, same order per element as the three-launch sequence: same bits
// (tests/test_gpu_api.py::test_cg_two_launch_iteration_is_bit_identical).  General CSR tiles (the FAST form of hipk_spmv_kernel:
// every tile fits the LDS product buffer, no long rows), also for matrices that have a coded form: at these sizes the matrix
// comes from L2 / the Infinity Cache and the kernel is launch-bound either way.
struct hipk_cg2_args {
    const int *crow;
    const int *col;
    const void *val;
    int64_t n;
    int ch, g;
    hipk_cg_scal *scal;
    int64_t it, maxiter;
    const double *part_rr;   // chunk partials of <r,r> (K2 of the iteration before; unused at it == 0)
    const void *r;
    const void *p_old;
    void *p_new;
    void *Ap;
    double *tpart;           // per-wavefront tile sums of <p, Ap>, 4 per tile
};

template <typename T, int CAP>
__global__ __launch_bounds__(HIPK_THREADS) void hipk_cg2_spmv_kernel(hipk_cg2_args a) {
    constexpr int NI = CAP / HIPK_THREADS;
    const int ntiles = (int)((a.n + HIPK_TILE - 1) / HIPK_TILE);
    const int tile = hipk_xcd_tile(blockIdx.x, ntiles);
    __shared__ __attribute__((aligned(16))) T prod[CAP];
    __shared__ int crowL[HIPK_TILE + 1];
    __shared__ double sbuf[HIPK_THREADS];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int *__restrict__ crow = a.crow;
    const int *__restrict__ col = a.col;
    const T *__restrict__ val = (const T *)a.val;
    const T *__restrict__ r = (const T *)a.r;
    const T *__restrict__ po = (const T *)a.p_old;
    hipk_cg_scal *scal = a.scal;
    const int64_t it = a.it;
    const int64_t r0 = (int64_t)(tile < 0 ? 0 : tile) * HIPK_TILE;
    const int nr = tile < 0 ? 0 : (int)((a.n - r0 < HIPK_TILE) ? (a.n - r0) : HIPK_TILE);
    int crow_t = 0, crow_e = 0;
    T rrow = (T)0, prow = (T)0;
    if (t < nr) {
        crow_t = crow[r0 + t];
        rrow = r[r0 + t];
        prow = po[r0 + t];
    }
    if (t == 0 && nr > 0) crow_e = crow[r0 + nr];
    if (it >= scal->stop_it) return;
    // <r,r> of the iteration before -> gamma_it, beta, the stop test of THIS pass (TSL:841, 851-853); every workgroup the same bits
    T beta = (T)0;
    if (it > 0) {
        const double gamma = hipk_reduce_parts(a.part_rr, a.g, sbuf);
        const double gamma_prev = scal->gamma[(it - 1) & 1];
        beta = (T)(gamma / gamma_prev);  // TSL:851
        const bool done = (it >= a.maxiter || gamma <= scal->atol2);
        if (blockIdx.x == 0 && t == 0) {
            scal->gamma[it & 1] = gamma;  // TSL:853
            if (done) scal->stop_it = it;
            hipk_signal(scal->host_sig, done ? (HIPK_SIG_STOP | it) : it);
        }
        if (done) return;
    }
    if (tile < 0) return;
    if (t < nr) crowL[t] = crow_t;
    if (t == 0) crowL[nr] = crow_e;
    __syncthreads();
    const int j0 = crowL[0];
    const int cnt = crowL[nr] - j0;
    if (cnt > 0) {
        const int jb = __builtin_amdgcn_readfirstlane(j0);
        const int *__restrict__ colb = col + jb;
        const T *__restrict__ valb = val + jb;
        unsigned jj[NI];
        int cc[NI];
        T vv[NI], rv[NI], pv[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int j = t + i * HIPK_THREADS;
            jj[i] = (unsigned)(j < cnt ? j : 0);
        }
#pragma unroll
        for (int i = 0; i < NI; ++i) cc[i] = colb[jj[i]];
#pragma unroll
        for (int i = 0; i < NI; ++i) vv[i] = valb[jj[i]];
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            rv[i] = r[cc[i]];
            pv[i] = po[cc[i]];
        }
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const T m = beta * pv[i];
            const T pj = rv[i] + m;  // TSL:852 at column cc[i]: the bits its owner stores
            prod[t + i * HIPK_THREADS] = vv[i] * pj;
        }
    }
    __syncthreads();
    double d0 = 0.0;
    if (t < nr) {
        const int lo = crowL[t] - j0, len = crowL[t + 1] - j0 - lo;
        T s = (T)0;
        for (int j = 0; j < len; ++j) s = s + prod[lo + j];
        const T m = beta * prow;
        const T pn = rrow + m;  // TSL:852, own row
        ((T *)a.p_new)[r0 + t] = pn;
        ((T *)a.Ap)[r0 + t] = s;
        d0 = (double)pn * (double)s;
    }
    d0 = hipk_wave_sum(d0);
    if (lane == 0) a.tpart[(size_t)tile * 4 + wave] = d0;
}

// K2: <p,Ap> from the tile sums (the combine kernel's chunk fold, then the spec's fold of the chunk partials), alpha,
// x += alpha p, r -= alpha Ap, partials of <r,r>.  grid = chunks (<= 256).
template <typename T>
__global__ __launch_bounds__(HIPK_THREADS) void hipk_cg2_update_kernel(int64_t n, int ch, int g, const hipk_cg_scal *__restrict__ scal,
                                                                      int64_t it, const double *__restrict__ tpart, int ntiles,
                                                                      const T *__restrict__ Ap, const T *__restrict__ p,
                                                                      T *__restrict__ r, T *__restrict__ x,
                                                                      double *__restrict__ part_rr) {
    const int c = blockIdx.x;
    hipk_pre<T, 2, false> pre;
    pre.issue(n, ch, c, {Ap, (const T *)r});
    if (it >= scal->stop_it) return;
    __shared__ double sbuf[HIPK_THREADS];
    __shared__ double cp[256];
    // chunk partial k = hipk_wave_fold over the chunk's <= 8 tiles (ch = 2048), by ONE thread per chunk: with cnt <= 8 that fold is
    // lane l < cnt holding ((0.0 + tp_l) + 0.0) + 0.0, the other lanes 0.0, and the wavefront tree, whose strides 32, 16, 8 add
    // zeros and whose strides 4, 2, 1 are ((v0 + v4) + (v2 + v6)) + ((v1 + v5) + (v3 + v7)).  (A wavefront per chunk, g / 4 folds
    // in series per workgroup, made this kernel 3 us per 32 chunks slower: 29.5 instead of 17.3 us per iteration at n = 250 k.)
    if ((int)threadIdx.x < g) {
        const int k = threadIdx.x, first = k * 8;
        const int cnt = (ntiles - first < 8) ? ntiles - first : 8;
        double v[8];
#pragma unroll
        for (int l = 0; l < 8; ++l) {
            double tl = 0.0;
            if (l < cnt) {
                const double *w4 = tpart + (size_t)(first + l) * 4;
                tl = 0.0 + ((w4[0] + w4[1]) + (w4[2] + w4[3]));
            }
            v[l] = ((tl + 0.0) + 0.0) + 0.0;   // a[0] + a[2], then + a[1] (+ a[3]) of hipk_wave_fold, then the strides 32, 16, 8
        }
        cp[k] = ((v[0] + v[4]) + (v[2] + v[6])) + ((v[1] + v[5]) + (v[3] + v[7]));
    }
    __syncthreads();
    const double pAp = hipk_reduce_parts(cp, g, sbuf);
    const double gamma = scal->gamma[it & 1];
    const T alpha = (T)(gamma / pAp);  // TSL:846
    double acc = 0.0;
    pre.run([&](int64_t i, int nv, T(&v)[2][hipk_vec<T>::VEC]) {
        constexpr int VEC = hipk_vec<T>::VEC;
        T rv[VEC], xv[VEC], pv[VEC];
        hipk_ld<T>(p, i, nv, pv);
        hipk_ld<T>((const T *)x, i, nv, xv);
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const T m0 = alpha * pv[k];
            xv[k] = xv[k] + m0;  // TSL:847
            const T m1 = alpha * v[0][k];
            rv[k] = v[1][k] - m1;  // TSL:848
            if (k < nv) acc = fma((double)rv[k], (double)rv[k], acc);  // TSL:850
        }
        hipk_st<T>(x, i, nv, xv);
        hipk_st<T>(r, i, nv, rv);
    });
    acc = hipk_block_sum(acc, sbuf);
    if (threadIdx.x == 0) part_rr[c] = acc;
}

// ---- row-partitioned CG with the exchanges folded into the kernels (hipk_fx.h; hipk_dist.hip drives them) -----------------
// The update / direction kernels above with an exchange in front: workgroups 0 .. world-1 publish this rank's partials (and, in
// the direction kernel, the boundary entries of r) into the peers' mailboxes, every workgroup waits for all sources and folds the
// gathered partials straight from its own mailbox.  grid = max(chunks, world): surplus workgroups only publish and wait.
__global__ __launch_bounds__(HIPK_THREADS) HIPK_SGPR80 void hipk_cg_update_fx_kernel(int64_t n, int ch, int g, const hipk_cg_scal *__restrict__ scal,
                                                                         int64_t it, const double *__restrict__ Ap, double *__restrict__ r,
                                                                         double *__restrict__ part_rr, hipk_fx fx) {
    typedef double T;
    const int c = blockIdx.x;
    hipk_pre<T, 2, false> pre;
    pre.issue(n, ch, c, {Ap, (const T *)r});
    if (it >= scal->stop_it) return;   // the same word on every rank (same partials, same fold): all ranks skip together
    __shared__ double sbuf[HIPK_THREADS];
    __shared__ int fx_ok;
    hipk_fx_publish(fx);
    if (c == 0) hipk_fx_collect(fx, g, sbuf, &fx_ok);
    hipk_fx_await(fx);
    const double pAp = hipk_fx_scalar(fx, 0);
    const double gamma = scal->gamma[it & 1];
    const T alpha = (T)(gamma / pAp);  // TSL:846
    double acc = 0.0;
    pre.run([&](int64_t i, int nv, T(&v)[2][hipk_vec<T>::VEC]) {
        constexpr int VEC = hipk_vec<T>::VEC;
        T rv[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const T m1 = alpha * v[0][k];
            rv[k] = v[1][k] - m1;  // TSL:848
            if (k < nv) acc = fma((double)rv[k], (double)rv[k], acc);  // TSL:850
        }
        hipk_st<T>(r, i, nv, rv);
    });
    acc = hipk_block_sum(acc, sbuf);
    if (threadIdx.x == 0 && (int64_t)c * ch < n) part_rr[c] = acc;
}

// n = n_ext (own rows + ghost tail), n_own = own rows.  The ghost entries of r arrive with the exchange: the workgroups whose chunk
// reaches into the tail copy their part from the mailbox into r BEFORE they request their operands; everybody else requests first.
__global__ __launch_bounds__(HIPK_THREADS) HIPK_SGPR80 __attribute__((amdgpu_waves_per_eu(8, 8))) void hipk_cg_direction_fx_kernel(int64_t n, int64_t n_own, int ch, int g,
                                                                            hipk_cg_scal *__restrict__ scal, int64_t it, int64_t maxiter,
                                                                            double *__restrict__ r, double *__restrict__ p,
                                                                            double *__restrict__ x, hipk_fx fx) {
    typedef double T;
    const int c = blockIdx.x;
    const bool tail = (int64_t)(c + 1) * ch > n_own && (int64_t)c * ch < n;
    __shared__ double sbuf[HIPK_THREADS];
    __shared__ int fx_ok;
    hipk_pre<T, 2, false> pre;
    if (!tail) pre.issue(n, ch, c, {(const T *)r, (const T *)p});
    if (it >= scal->stop_it) return;
    hipk_fx_publish(fx);
    if (c == 0) hipk_fx_collect(fx, g, sbuf, &fx_ok);
    hipk_fx_await(fx);
    if (tail) {
        const double *halo = hipk_fx_halo(fx);   // fine-grained memory: read from memory, after the collector's flag
        const int64_t lo = ((int64_t)c * ch > n_own ? (int64_t)c * ch : n_own), hi = ((int64_t)(c + 1) * ch < n ? (int64_t)(c + 1) * ch : n);
        for (int64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) r[i] = halo[i - n_own];
        __syncthreads();
        pre.issue(n, ch, c, {(const T *)r, (const T *)p});
    }
    const double pAp = hipk_fx_scalar(fx, 0), rr = hipk_fx_scalar(fx, 1);
    const double gamma = scal->gamma[it & 1];
    const T alpha = (T)(gamma / pAp);  // TSL:846, the same bits hipk_cg_update_fx_kernel derived
    const T beta = (T)(rr / gamma);    // TSL:851
    pre.run([&](int64_t i, int nv, T(&v)[2][hipk_vec<T>::VEC]) {
        constexpr int VEC = hipk_vec<T>::VEC;
        T xv[VEC], pv[VEC];
        hipk_ld<T>((const T *)x, i, nv, xv);
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const T m0 = alpha * v[1][k];
            xv[k] = xv[k] + m0;  // TSL:847 (with the p of this iteration, before it is replaced)
            const T m = beta * v[1][k];
            pv[k] = v[0][k] + m;  // TSL:852
        }
        hipk_st<T>(x, i, nv, xv);
        hipk_st<T>(p, i, nv, pv);
    });
    if (c == 0 && threadIdx.x == 0) {
        scal->gamma[(it + 1) & 1] = rr;  // TSL:853
        const bool done = (it + 1 >= maxiter || rr <= scal->atol2);  // TSL:841 for the NEXT pass
        if (done) scal->stop_it = it + 1;
        hipk_signal(scal->host_sig, done ? (HIPK_SIG_STOP | (it + 1)) : (it + 1));
    }
}

// hipk_dist.hip's entry points to them (fp64; fx->seq / ch / kind / parts / vec filled by the caller per exchange)
int hipk_cg_update_fx(int64_t n_local, int chunk_rows, int g_red, const void *scal_dev, int64_t it, const void *Ap, void *r,
                      double *part_rr_out, const hipk_fx *fx, hipStream_t stream) {
    int grid = (int)((n_local + chunk_rows - 1) / chunk_rows);
    if (grid < fx->world) grid = fx->world;
    hipk_cg_update_fx_kernel<<<grid, HIPK_THREADS, 0, stream>>>(n_local, chunk_rows, g_red, (const hipk_cg_scal *)scal_dev, it,
                                                               (const double *)Ap, (double *)r, part_rr_out, *fx);
    HIPK_CHECK_HIP(hipGetLastError());
    return HIPK_OK;
}
int hipk_cg_direction_fx(int64_t n_ext, int64_t n_local, int chunk_rows, int g_red, void *scal_dev, int64_t it, int64_t maxiter, void *r,
                         void *p, void *x, const hipk_fx *fx, hipStream_t stream) {
    int grid = (int)((n_ext + chunk_rows - 1) / chunk_rows);
    if (grid < fx->world) grid = fx->world;
    hipk_cg_direction_fx_kernel<<<grid, HIPK_THREADS, 0, stream>>>(n_ext, n_local, chunk_rows, g_red, (hipk_cg_scal *)scal_dev, it, maxiter,
                                                                  (double *)r, (double *)p, (double *)x, *fx);
    HIPK_CHECK_HIP(hipGetLastError());
    return HIPK_OK;
}

// Streaming policy on one device (vectors in HBM: N >> 8 M rows): the direction step as TWO launches -- alpha, beta, the next gamma
// and the stop test once, by one workgroup (the same fold of the same partials: the same bits); then a FLAT grid of short
// workgroups (2048 elements each, every load requested before the stop word is read), which a step without a dot is free to use.
// Why: at N = 64 M a workgroup per 256 KB chunk keeps 1954 x 5 distant streams open; the same bytes move 6-10 % faster from short
// workgroups over adjacent addresses, and lose less when the vectors landed badly (profiles/r02_axpy_probe_64m.txt,
// r02_axpy_realloc_64m.txt: 5.8 -> 6.1 TB/s, and 4.9 -> 5.4 TB/s in the slow placement); per workgroup the fold of 2 x 1954
// partials is what stood in the way.  The extra launch costs ~4 us of an iteration of ~1 ms.
__global__ __launch_bounds__(HIPK_THREADS) void hipk_cg_scalars_kernel(int g, hipk_cg_scal *__restrict__ scal, int64_t it, int64_t maxiter,
                                                                       const double *__restrict__ part_pAp,
                                                                       const double *__restrict__ part_rr) {
    if (it >= scal->stop_it) return;
    __shared__ double sbuf[2 * HIPK_THREADS];
    double pAp, rr;
    hipk_reduce_parts2(part_pAp, part_rr, g, pAp, rr, sbuf);
    if (threadIdx.x == 0) {
        const double gamma = scal->gamma[it & 1];
        scal->dir_alpha = gamma / pAp;       // TSL:846, the same bits hipk_cg_update_kernel derived
        scal->dir_beta = rr / gamma;         // TSL:851
        scal->gamma[(it + 1) & 1] = rr;      // TSL:853
        const bool done = (it + 1 >= maxiter || rr <= scal->atol2);  // TSL:841 for the NEXT pass (this pass compares against `it`)
        if (done) scal->stop_it = it + 1;
        hipk_signal(scal->host_sig, done ? (HIPK_SIG_STOP | (it + 1)) : (it + 1));
    }
}

template <typename T>
__global__ __launch_bounds__(HIPK_THREADS) void hipk_cg_direction_flat_kernel(int64_t n, const hipk_cg_scal *__restrict__ scal, int64_t it,
                                                                              const T *__restrict__ r, T *__restrict__ p,
                                                                              T *__restrict__ x) {
    constexpr int VEC = hipk_vec<T>::VEC;
    constexpr int STEPS = HIPK_BASE_CHUNK / (VEC * HIPK_THREADS);
    const int64_t base = (int64_t)blockIdx.x * HIPK_BASE_CHUNK + (int64_t)VEC * threadIdx.x;
    T rv[STEPS][VEC], pv[STEPS][VEC], xv[STEPS][VEC];
    int nvs[STEPS];
#pragma unroll
    for (int k = 0; k < STEPS; ++k) {
        const int64_t i = base + (int64_t)k * VEC * HIPK_THREADS;
        nvs[k] = (i < n) ? ((n - i < VEC) ? (int)(n - i) : VEC) : 0;
        if (nvs[k] > 0) {
            hipk_ld_nt_vec<T>(r, i, nvs[k], rv[k]);
            hipk_ld_nt_vec<T>((const T *)p, i, nvs[k], pv[k]);
            hipk_ld_nt_vec<T>((const T *)x, i, nvs[k], xv[k]);
        }
    }
    if (it >= scal->stop_it) return;  // hipk_cg_scalars_kernel of THIS pass has run: it sets stop_it = it + 1 at the earliest
    const T alpha = (T)scal->dir_alpha;
    const T beta = (T)scal->dir_beta;
#pragma unroll
    for (int k = 0; k < STEPS; ++k) {
        if (nvs[k] > 0) {
            const int64_t i = base + (int64_t)k * VEC * HIPK_THREADS;
            T xo[VEC], po[VEC];
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const T m0 = alpha * pv[k][e];
                xo[e] = xv[k][e] + m0;  // TSL:847 (with the p of this iteration, before it is replaced)
                const T m = beta * pv[k][e];
                po[e] = rv[k][e] + m;  // TSL:852
            }
            hipk_st_nt_vec<T>(x, i, nvs[k], xo);  // x is not read again before the next direction step
            hipk_st<T>(p, i, nvs[k], po);
        }
    }
}

// ---- placement probe (include/hipk.h: hipk_placement_probe).  At N = 64 M the direction step above runs at one of two discrete
// speeds -- 5.85 or 4.9 TB/s -- depending on where the three vectors landed PHYSICALLY (profiles/r02_axpy_realloc_64m.txt: the same
// kernel at the same virtual addresses, re-allocated; vectors in separate allocations were slow every time, vectors in ONE
// allocation fast in about half of the draws).  This kernel has the step's memory shape (reads r, p, x non-temporal, writes p and
// x) and stores back the bits it loaded, so it can run on live vectors; the host times it and re-draws the allocation when it
// reads the slow level.
__device__ __forceinline__ bool hipk_value_bits_eq(double a, double b) { return __double_as_longlong(a) == __double_as_longlong(b); }
__device__ __forceinline__ bool hipk_value_bits_eq(float a, float b) { return __float_as_int(a) == __float_as_int(b); }
template <typename T>
__global__ __launch_bounds__(HIPK_THREADS) void hipk_probe3_kernel(int64_t n, const T *__restrict__ r, T *__restrict__ p, T *__restrict__ x,
                                                                   T never) {
    constexpr int VEC = hipk_vec<T>::VEC;
    constexpr int STEPS = HIPK_BASE_CHUNK / (VEC * HIPK_THREADS);
    const int64_t base = (int64_t)blockIdx.x * HIPK_BASE_CHUNK + (int64_t)VEC * threadIdx.x;
    T rv[STEPS][VEC], pv[STEPS][VEC], xv[STEPS][VEC];
    int nvs[STEPS];
#pragma unroll
    for (int k = 0; k < STEPS; ++k) {
        const int64_t i = base + (int64_t)k * VEC * HIPK_THREADS;
        nvs[k] = (i < n) ? ((n - i < VEC) ? (int)(n - i) : VEC) : 0;
        if (nvs[k] > 0) {
            hipk_ld_nt_vec<T>(r, i, nvs[k], rv[k]);
            hipk_ld_nt_vec<T>((const T *)p, i, nvs[k], pv[k]);
            hipk_ld_nt_vec<T>((const T *)x, i, nvs[k], xv[k]);
        }
    }
#pragma unroll
    for (int k = 0; k < STEPS; ++k) {
        if (nvs[k] > 0) {
            const int64_t i = base + (int64_t)k * VEC * HIPK_THREADS;
            // `never` is a NaN with a payload no computation produces: the comparison keeps the loads of r alive, the stores put
            // back what was loaded
#pragma unroll
            for (int e = 0; e < VEC; ++e)
                if (hipk_value_bits_eq(rv[k][e], never)) pv[k][e] = rv[k][e];
            hipk_st_nt_vec<T>(x, i, nvs[k], xv[k]);
            hipk_st<T>(p, i, nvs[k], pv[k]);
        }
    }
}

extern "C" int hipk_placement_probe(int64_t n, const void *r, void *p, void *x, int dtype, int reps, double *us_out,
                                    hipk_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    HIPK_REQUIRE(n > 0 && r && p && x && us_out, HIPK_ERR_ARG, "null argument");
    HIPK_REQUIRE(dtype == HIPK_F64 || dtype == HIPK_F32, HIPK_ERR_UNSUPPORTED, "dtype must be f32/f64");
    HIPK_REQUIRE(hipk_aligned16(r) && hipk_aligned16(p) && hipk_aligned16(x), HIPK_ERR_ALIGN, "vectors must be 16-byte aligned");
    if (reps < 1) reps = 1;
    if (reps > 16) reps = 16;
    const unsigned grid = (unsigned)((n + HIPK_BASE_CHUNK - 1) / HIPK_BASE_CHUNK);
    hipk_event_pair ev[16];
    for (int i = 0; i < reps; ++i) HIPK_CHECK_HIP(ev[i].create());
    // one untimed pass (first touch, TLB), then `reps` passes each with events bound to its dispatch (hipk_solve.h)
    for (int i = -1; i < reps; ++i) {
        void *argv[5];
        double nan64;
        float nan32;
        const unsigned long long b64 = 0x7FF8DEADBEEF1234ull;
        const unsigned b32 = 0x7FC0BEEFu;
        memcpy(&nan64, &b64, 8);
        memcpy(&nan32, &b32, 4);
        argv[0] = (void *)&n;
        argv[1] = (void *)&r;
        argv[2] = (void *)&p;
        argv[3] = (void *)&x;
        argv[4] = dtype == HIPK_F64 ? (void *)&nan64 : (void *)&nan32;
        const void *fn = dtype == HIPK_F64 ? (const void *)hipk_probe3_kernel<double> : (const void *)hipk_probe3_kernel<float>;
        if (i < 0)
            HIPK_CHECK_HIP(hipLaunchKernel(fn, dim3(grid), dim3(HIPK_THREADS), argv, 0, stream));
        else
            HIPK_CHECK_HIP(hipExtLaunchKernel(fn, dim3(grid), dim3(HIPK_THREADS), argv, 0, stream, ev[i].a, ev[i].b, 0));
    }
    HIPK_CHECK_HIP(hipStreamSynchronize(stream));
    double best = 1e300;
    for (int i = 0; i < reps; ++i) {
        float ms = 0.f;
        HIPK_CHECK_HIP(hipEventElapsedTime(&ms, ev[i].a, ev[i].b));
        if ((double)ms * 1e3 < best) best = (double)ms * 1e3;
    }
    *us_out = best;
    return HIPK_OK;
}

// x += alpha p alone (TSL:847): the row-partitioned solver runs it on a side stream while the <r,r> / halo collective of the
// iteration is in flight; alpha from the same partials and the same gamma as the update and direction kernels (same bits)
template <typename T>
__global__ __launch_bounds__(HIPK_THREADS) void hipk_cg_xupdate_kernel(int64_t n, int ch, int g, const hipk_cg_scal *__restrict__ scal,
                                                                       int64_t it, const double *__restrict__ part_pAp,
                                                                       const T *__restrict__ p, T *__restrict__ x) {
    const int c = blockIdx.x;
    hipk_pre<T, 2> pre;
    pre.issue(n, ch, c, {p, (const T *)x});
    if (it >= scal->stop_it) return;
    __shared__ double sbuf[HIPK_THREADS];
    const double pAp = hipk_reduce_parts(part_pAp, g, sbuf);
    const T alpha = (T)(scal->gamma[it & 1] / pAp);  // TSL:846
    pre.run([&](int64_t i, int nv, T(&v)[2][hipk_vec<T>::VEC]) {
        constexpr int VEC = hipk_vec<T>::VEC;
        T xv[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const T m0 = alpha * v[0][k];
            xv[k] = v[1][k] + m0;
        }
        hipk_st<T>(x, i, nv, xv);
    });
}

// =====================================================================================================================
// Small systems (<= 8 reduction chunks = n <= 16384, rows of <= 12 entries): THE WHOLE CG LOOP IN ONE LAUNCH.
// Three launches of >= 4.9 us per iteration for 80 KB vectors leave such systems launch-bound (16 us per iteration at n = 10^4).
// Here 8 g workgroups stay resident on one XCD and meet at two hand-offs per iteration (csrc/hipk_handoff.h; the scheme of
// hipk_gm_solve_lds_kernel).  Every thread plays two roles:
//   * VECTOR role: row (u, e8) of the spec's virtual-thread layout (sub-workgroup s of chunk c owns the virtual threads s + 8u):
//     x, r, p of that row live in REGISTERS for the whole solve; <r,r> is the chain of its virtual thread + a 32-lane tree, published
//     as a sub-partial that every consumer folds with the last three levels of the chunk tree -- the bits of the chunk dot;
//   * SpMV role: row tile*256 + tid of ONE 256-row tile, because <p,Ap> is the TILED dot of the SpMV epilogue (wavefront sums over
//     64 contiguous rows).  The row's matrix entries and the p values they multiply stay in registers: after the <r,r> hand-off
//     the thread gathers r at its columns and advances its own copies, p_j = r_j + beta p_j -- the owner's formula on the owner's
//     operands, the same bits -- so p itself is never exchanged.
// hand-off 1: tile sums of <p,Ap> + Ap by tile rows;  hand-off 2: sub-partials of <r,r> + r.  Arithmetic per element = the
// three-kernel loop's (TSL:845-853), bit for bit.
template <typename T>
struct hipk_cg_lds_args {
    int64_t n;
    int g;
    const int *crow;
    const int *col;
    const T *val;
    T *x, *r, *p;
    T *Ap;               // exchange buffer: A p by rows
    hipk_lds_ctl *ctl;          // progress of the launch
    double *gamma;              // [2] by iteration parity; in: gamma of iteration it0 (it0 > 0 or M = identity), out: of the last one
    const double *atol2;        // device scalars of the solve's header block
    int64_t *stop_it;
    const T *dinv;              // PRE: the Jacobi preconditioner's diagonal (M = diag(dinv), TSL:849)
    const double *rz0_parts;    // PRE, it0 = 0: chunk partials of gamma0 = <r0, M r0> (hipk_pcg_start_kernel)
    double *tile_pp;     // [ntiles * 4] wavefront sums of <p,Ap>
    double *rr_sub;      // [8 g] sub-partials of <r,r>
    double *rz_sub;      // PRE: [8 g] sub-partials of <r, M r>
    unsigned long long *flag_a, *flag_b;   // [64] each, zeroed before the launch
    int64_t it0;         // iterations done before this launch
    int64_t maxiter;
    int64_t max_its;     // iteration budget of one launch
    int test_not_resident;   // tests (hipk_test_fail_launch): report the placement check as failed
    int spread;              // more than 64 workgroups: one per block all over the chip (then LOCAL = false)
};
static constexpr int kCgRowRegs = 12;

template <typename T, bool LOCAL, bool PRE>
__global__ __launch_bounds__(HIPK_THREADS, 2) void hipk_cg_solve_lds_kernel(hipk_cg_lds_args<T> a) {
    constexpr int VEC = hipk_vec<T>::VEC;
    int wg = blockIdx.x;                             // spread (more than 64 workgroups): one per block, anywhere on the chip
    if (!a.spread) {
        if (blockIdx.x & 7) return;                  // the working blocks share an XCD (dispatch is round-robin over 8)
        wg = blockIdx.x >> 3;
    }
    const int c = wg / kGmSub, s = wg % kGmSub;
    const int g = a.g, nwg = g * kGmSub;
    if (c >= g) return;
    hipk_lds_ctl *scal = a.ctl;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int u = tid & 31, e8 = tid >> 5;
    const int64_t n = a.n;
    const int64_t base = (int64_t)c * HIPK_BASE_CHUNK;
    const int64_t row = base + (int64_t)VEC * (s + kGmSub * u) + (int64_t)(e8 / VEC) * (VEC * HIPK_THREADS) + (e8 % VEC);
    const bool live = row < n;
    const int ntiles = (int)((n + HIPK_TILE - 1) / HIPK_TILE);
    const int tile = c * (HIPK_BASE_CHUNK / HIPK_TILE) + s;
    const int64_t trow = (int64_t)tile * HIPK_TILE + tid;
    const bool tlive = trow < n;

    __shared__ T wl[HIPK_THREADS], wz[HIPK_THREADS];
    __shared__ double bc[4];
    __shared__ int fail;
    __shared__ unsigned long long res_lds;
    if (tid == 0) fail = 0;

    // vector role
    T x_own = live ? a.x[row] : (T)0, r_own = live ? a.r[row] : (T)0, p_own = live ? a.p[row] : (T)0;
    // SpMV role: the tile row's entries, and p at its columns (the launches before this one left p in memory)
    int lo = 0, len = 0;
    if (tlive) {
        lo = a.crow[trow];
        len = a.crow[trow + 1] - lo;
    }
    unsigned cj[kCgRowRegs];
    T vj[kCgRowRegs], pg[kCgRowRegs];
#pragma unroll
    for (int j = 0; j < kCgRowRegs; ++j) {
        const int cc = (j < len) ? a.col[lo + j] : 0;
        cj[j] = (unsigned)cc * (unsigned)sizeof(T);
        vj[j] = (j < len) ? a.val[lo + j] : (T)0;
        pg[j] = (j < len) ? a.p[cc] : (T)0;
    }
    T p_t = tlive ? a.p[trow] : (T)0;
    // PRE: the diagonal of M at the own row, at the tile row and at the tile row's columns
    T d_own = (T)1, d_t = (T)1, dc[kCgRowRegs];
#pragma unroll
    for (int j = 0; j < kCgRowRegs; ++j) dc[j] = (T)1;
    if (PRE) {
        d_own = live ? a.dinv[row] : (T)0;
        d_t = tlive ? a.dinv[trow] : (T)0;
#pragma unroll
        for (int j = 0; j < kCgRowRegs; ++j) dc[j] = (j < len) ? a.dinv[a.col[lo + j]] : (T)0;
    }
    int wmax = len < kCgRowRegs ? len : kCgRowRegs;
    for (int off = 32; off > 0; off >>= 1) {
        const int o = __shfl_xor(wmax, off);
        wmax = o > wmax ? o : wmax;
    }
    wmax = __builtin_amdgcn_readfirstlane(wmax);
    double gamma = a.gamma[a.it0 & 1];
    const double atol2 = *a.atol2;
    const int64_t stop0 = *a.stop_it;
    double rs_last = scal->rs_last;

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
    if (PRE && a.it0 == 0) {   // gamma0 = <r0, M r0>: chunk partials of the launch before this one (hipk_reduce_parts)
        if (tid < 64) {
            double a8 = (tid < g) ? a.rz0_parts[tid] : 0.0;
            a8 = 0.0 + a8;
            a8 = hipk_wave_sum(a8);
            if (tid == 0) bc[2] = a8;
        }
        __syncthreads();
        gamma = bc[2];
    }
    unsigned long long seq = 0;
    int64_t it = a.it0;
    bool done = stop0 <= it;
    while (!done) {
        // ---- SpMV role: (A p) of the tile row, wavefront sums of p .* (A p)  (TSL:845-846)
        T acc_row = (T)0;
#pragma unroll
        for (int j = 0; j < kCgRowRegs; ++j)
            if (j < wmax) {
                const T pr = vj[j] * pg[j];
                acc_row = (j < len) ? acc_row + pr : acc_row;
            }
        const T Ap_t = tlive ? acc_row : (T)0;
        double d0 = tlive ? (double)p_t * (double)Ap_t : 0.0;
        d0 = hipk_wave_sum(d0);
        if (lane == 0 && tile < ntiles) hipk_ho_store<LOCAL>(&a.tile_pp[(size_t)tile * 4 + wave], d0);
        if (tlive) hipk_ho_store<LOCAL>(a.Ap + trow, Ap_t);
        if (hipk_ho_sync<LOCAL>(a.flag_a, wg, nwg, ++seq, 0u, &res_lds) == ~0ull) {
            if (tid == 0) scal->redo = -3;   // cannot happen once every workgroup has passed the placement check
            return;
        }
        // ---- vector role: alpha, r, x, <r,r> sub-partial  (TSL:846-850)
        const T Ap_own = live ? hipk_peek_t<T>(a.Ap + row) : (T)0;
        if (tid < 64) {
            const double *tp = a.tile_pp;
            const double pAp = hipk_fold_64x8(tid, g, [&](int ci, int tt) {
                const int tl = ci * (HIPK_BASE_CHUNK / HIPK_TILE) + tt;
                if (tl >= ntiles) return 0.0;
                const double *w4 = tp + (size_t)tl * 4;
                const double w0 = hipk_peek(w4), w1 = hipk_peek(w4 + 1), w2 = hipk_peek(w4 + 2), w3 = hipk_peek(w4 + 3);
                return 0.0 + ((w0 + w1) + (w2 + w3));
            });
            if (tid == 0) bc[0] = pAp;
        }
        __syncthreads();
        const T alpha = (T)(gamma / bc[0]);
        {
            const T m1 = alpha * Ap_own;
            r_own = r_own - m1;
            const T m0 = alpha * p_own;
            x_own = x_own + m0;
        }
        wl[tid] = r_own;
        if (PRE) wz[tid] = d_own * r_own;   // z = M r (TSL:849), never stored to memory
        if (live) hipk_ho_store<LOCAL>(a.r + row, r_own);
        __syncthreads();
        if (tid < 32) {
            double acc = 0.0, acc1 = 0.0;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const double v = (double)wl[e * 32 + tid];
                acc = fma(v, v, acc);
                if (PRE) acc1 = fma(v, (double)wz[e * 32 + tid], acc1);   // TSL:850
            }
            acc = hipk_half_sum(acc);
            if (PRE) acc1 = hipk_half_sum(acc1);
            if (tid == 0) {
                hipk_ho_store<LOCAL>(&a.rr_sub[wg], acc);
                if (PRE) hipk_ho_store<LOCAL>(&a.rz_sub[wg], acc1);
            }
        }
        if (hipk_ho_sync<LOCAL>(a.flag_b, wg, nwg, ++seq, 0u, &res_lds) == ~0ull) {
            if (tid == 0) scal->redo = -3;
            return;
        }
        // ---- beta, p (both roles), stop test  (TSL:851-853, 841)
        T rg[kCgRowRegs];
#pragma unroll
        for (int j = 0; j < kCgRowRegs; ++j)
            if (j < wmax) rg[j] = hipk_peek_off<T>(a.r, cj[j]);
        const T r_t = tlive ? hipk_peek_t<T>(a.r + trow) : (T)0;
        if (tid < 64) {
            const double rr = hipk_fold_64x8(tid, g, [&](int ci, int ss) { return hipk_peek(a.rr_sub + ci * kGmSub + ss); });
            if (tid == 0) bc[1] = rr;
        } else if (PRE && tid < 128) {
            const double rz = hipk_fold_64x8(tid - 64, g, [&](int ci, int ss) { return hipk_peek(a.rz_sub + ci * kGmSub + ss); });
            if (tid == 64) bc[3] = rz;
        }
        __syncthreads();
        const double rr = bc[1];
        const double gamma_new = PRE ? bc[3] : rr;   // <r,z> steers alpha and beta, <r,r> the stop test (TSL:835-841)
        const T beta = (T)(gamma_new / gamma);
        {
            const T z_own = PRE ? d_own * r_own : r_own;
            const T m = beta * p_own;
            p_own = z_own + m;
            const T z_t = PRE ? d_t * r_t : r_t;
            const T mt = beta * p_t;
            p_t = z_t + mt;
        }
#pragma unroll
        for (int j = 0; j < kCgRowRegs; ++j)
            if (j < wmax) {
                const T zj = PRE ? dc[j] * rg[j] : rg[j];
                const T m = beta * pg[j];
                pg[j] = zj + m;
            }
        gamma = gamma_new;
        rs_last = rr;
        ++it;
        done = (it >= a.maxiter || rr <= atol2);
        if (it - a.it0 >= a.max_its) break;
    }
    if (live) {
        a.x[row] = x_own;
        a.p[row] = p_own;
    }
    if (wg == 0 && tid == 0) {
        a.gamma[it & 1] = gamma;
        scal->rs_last = rs_last;
        scal->it_done = it;
        if (done && it < stop0) *a.stop_it = it;
    }
}

// res2 = sum parts0, xx = sum parts1 -> scal
__global__ __launch_bounds__(HIPK_THREADS) void hipk_cg_final_kernel(hipk_cg_scal *__restrict__ scal, int g,
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


// two launches per iteration (hipk_cg2_*): 33 .. 150 reduction chunks.  Same box, alternating, 5-point Poisson, us per iteration
// two / three launches: n = 90 k 12.4 / 15.7-16.7, 160 k 14.0 / 16.7-17.5, 250 k 15.7 / 17.0-17.9, 360 k 18.5 / 18.7-18.8,
// 518 k 21.2 / 20.2 (the general CSR tiles' 12 bytes per entry catch up with the saved launch): profiles/r03_cg_two_launch.txt
static constexpr int kCg2MaxChunks = 150;

// x, r, p, Ap beyond 1.5 x the 256 MiB Infinity Cache: the vector kernels treat every operand as a stream
static inline bool hipk_cg_streams_by_size(size_t n, size_t sv) { return 4 * n * sv > (size_t)384 << 20; }

// the one-launch instantiations the dispatch sites below select (hipk_mid_pick), each with the name hipk_last_solve_path reports.
// Two chunks per workgroup put four rows on a thread: at most 7 entries each in registers
#define HIPK_MID_ROW(W, NCH, PRE)                                                                                          \
    {W, NCH, PRE, hipk_cg_mid_kernel<T, W, NCH, PRE>,                                                                      \
     HIPK_FORM_OF_T(T, "hipk_cg_mid_kernel<", #W "," #NCH "," #PRE ">")}
template <typename T>
static const hipk_mid_entry<hipk_cg_mid_args> hipk_cg_mid_table[] = {
    HIPK_MID_ROW(5, 1, false), HIPK_MID_ROW(7, 1, false), HIPK_MID_ROW(9, 1, false), HIPK_MID_ROW(12, 1, false),
    HIPK_MID_ROW(5, 2, false), HIPK_MID_ROW(7, 2, false),
    HIPK_MID_ROW(5, 1, true),  HIPK_MID_ROW(7, 1, true),  HIPK_MID_ROW(9, 1, true),  HIPK_MID_ROW(12, 1, true)};
#undef HIPK_MID_ROW
static constexpr int kPcgMidMaxChunks = 256;                                 // one chunk per workgroup, one workgroup per CU
static constexpr size_t kPcgMidSlotBytes = 3 * (size_t)kMidMaxChunks * 256;   // <p,Ap>, <r,r>, <r,z> slot arrays

// ---------------------------------------------------------------- the workspace of a cg or Jacobi pcg solve
// Byte offsets, from (n, dtype, pre) alone: hipk_cg_work_bytes and hipk_pcg_work_bytes return .total, the solve takes its pointers
// from the rest.  scalars (hipk_cg_scal / hipk_pcg_scal) | partial slots (cg: the four of hipk_scratch_bytes, pcg: six) | r, p, Ap |
// what the size allows behind Ap.  The loop forms of a solve -- the mid loop, the LDS loop, one launch sequence -- run one after
// the other: a one-launch loop has returned (finished, or handed the solve back) before the next form's first launch is
// enqueued, and none runs twice.  A region of one form may therefore lie in bytes that another form owns.
struct hipk_cg_layout {
    size_t scal;
    size_t part_a, part_b, part_c;   // <p,Ap> | <r,r> | spare dot slot of the SpMV
    size_t part_z[2];                // pcg: <r,z> ping-pong (read by all workgroups of the update kernel while the early ones already
                                     // write the next one)
    size_t part_d;                   // <b,b> / <x,x>: pcg a slot of its own, cg part_a
    size_t r, p, Ap;
    // The LDS loop (hipk_cg_solve_lds_kernel) in slots of the launch sequences, which only write them once they run (pcg:
    // part_z[1] is first written by the update kernel of iteration 0; hipk_cg_steps<T, true>::one_launch rebuilds the slot the
    // sequence reads after a hand-back):
    size_t lds_flags;    // 2 x kHoMaxWg hand-off words, the upper half of the spare slot
    size_t lds_rr_sub;   // sub-partials of <r,r>, in its chunk-partial slot (part_b, which holds those of <r0,r0> at iteration 0)
    size_t lds_rz_sub;   // pcg: sub-partials of <r,z>, in part_z[1]
    // The mid loop (hipk_cg_mid_kernel), present iff mid.  It keeps r as 16-byte flagged words whatever the dtype -- one more
    // fp64 vector, three more fp32 ones -- from Ap on: at these sizes the place of Ap is ll_bytes long and Ap is its head.
    bool mid;
    size_t ll_bytes;
    size_t r_ll;                   // = Ap
    size_t pap_ll, rr_ll, rz_ll;   // the chunk-partial slots of <p,Ap>, <r,r> and (pcg) <r,z>, kMidSlotArray bytes each
    // A second direction vector behind Ap: the two-launch form gathers the old p while it forms the new one, the deferred-x form
    // keeps p_j by parity.  At the mid sizes it lies in the mid loop's bytes (the tail of r_ll and, where 2 vec = ll_bytes + 256,
    // the first line of pap_ll); beyond them, up to the size at which the streaming policy takes over, it is a vector of its own.
    // No room (fourth_vector false) up to kMidMinChunks chunks, at the streaming sizes, and in a pcg solve, which has neither form.
    bool fourth_vector;
    size_t p2;
    // The fused SpMV + update launch (hipk_cg_fuse.h) keeps Ap on chip, so the head of Ap is its own: the chunks' flagged <p,Ap>
    // words, then the collectors' eight hand-out lines, then the same again for the <r,r> of the direction tail (the kernel finds
    // the lines behind the words and the second pair behind the first) -- one region, cleared by one memset when the sequence begins.  (Not in the partial
    // slots: hipk_cg_direction_kernel folds the plain <p,Ap> partials from part_a, which the fused launch therefore still writes.)
    // A sequence of the separate kernels that takes over after a give-up writes Ap again; the fused form is not tried again then.
    size_t fuse_words;
    size_t total;
};
static constexpr size_t kFuseBytes = 2 * (kFuseWordsBytes + kFuseCtlBytes);   // <p,Ap>'s words and replicas, then <r,r>'s (the direction tail)
static_assert(kFuseWordsBytes % 256 == 0 && kFuseCtlBytes == 8 * 16 * kFuseReplicaSlots, "the replicas follow the words, 128 bytes apart");
static_assert(kFuseBytes == 2 * (kFuseWordsBytes + kFuseCtlBytes) && (kFuseWordsBytes + kFuseCtlBytes) % 256 == 0,
              "the direction tail's words and replicas follow the first pair, laid out the same");
static_assert(kFuseBytes <= (size_t)kMidMaxChunks * HIPK_BASE_CHUNK * sizeof(double),
              "the fused form runs beyond the mid loop's chunk count, fp64: Ap is longer than its region");
static constexpr size_t kMidSlotArray = (size_t)kMidMaxChunks * 256;   // a slot array of the mid loop at the widest slot stride
static_assert(kMidSlotBytes == 2 * kMidSlotArray && kPcgMidSlotBytes == 3 * kMidSlotArray, "pap_ll, rr_ll and (pcg) rz_ll");
static_assert(HIPK_MAX_PARTS / 2 + 2 * kHoMaxWg <= HIPK_MAX_PARTS, "the LDS loop's hand-off flags fit the upper half of the spare slot");
static_assert(kHoMaxWg <= HIPK_MAX_PARTS, "the LDS loop's sub-partials fit a chunk-partial slot");
static_assert(kMidSlotBytes >= 256, "p2 ends inside the mid loop's bytes: 2 vec <= ll_bytes + 256");
static_assert(HIPK_SCRATCH_SLOTS == 4, "cg: part_a, part_b, part_c and one unused slot");

static hipk_cg_layout hipk_cg_make_layout(int64_t n, int dtype, bool pre) {
    const size_t sv = (dtype == HIPK_F64) ? 8 : 4, rows = (size_t)(n > 0 ? n : 1), vec = hipk_align_up(rows * sv, 256);
    const size_t slot = HIPK_MAX_PARTS * sizeof(double);
    const hipk_geom gm = hipk_make_geom(n > 0 ? n : 1);
    hipk_cg_layout L;
    hipk_carve take;
    L.scal = take(256);
    L.part_a = take(slot);
    L.part_b = take(slot);
    L.part_c = take(slot);
    L.part_z[0] = take(slot);   // (cg: the fourth slot of hipk_scratch_bytes, unused)
    L.part_z[1] = pre ? take(slot) : 0;
    L.part_d = pre ? take(slot) : L.part_a;
    L.lds_flags = L.part_c + slot / 2;
    L.lds_rr_sub = L.part_b;
    L.lds_rz_sub = L.part_z[1];
    L.r = take(vec);
    L.p = take(vec);
    L.mid = gm.g > kMidMinChunks && gm.g <= (pre ? kPcgMidMaxChunks : kMidMaxChunks);
    L.ll_bytes = hipk_align_up(rows * 16, 256);
    L.Ap = L.r_ll = take(L.mid ? L.ll_bytes : vec);
    L.pap_ll = L.mid ? take(pre ? kPcgMidSlotBytes : kMidSlotBytes) : 0;
    L.rr_ll = L.pap_ll + kMidSlotArray;
    L.rz_ll = L.rr_ll + kMidSlotArray;
    // beyond the mid loop, up to the size at which the streaming policy takes over (hipk_cg_path_begin): a vector of its own
    const bool second_p = !pre && !L.mid && gm.g > kMidMaxChunks && !hipk_cg_streams_by_size(rows, sv);
    L.p2 = L.Ap + vec;
    if (second_p) take(vec);
    L.fourth_vector = !pre && (L.mid || second_p);
    L.fuse_words = L.Ap;
    L.total = take.o;
    return L;
}
extern "C" size_t hipk_cg_work_bytes(int64_t n, int dtype) { return hipk_cg_make_layout(n, dtype, false).total; }
extern "C" size_t hipk_pcg_work_bytes(int64_t n, int dtype) { return hipk_cg_make_layout(n, dtype, true).total; }

// ---- which paths a cg (PRE = false) or Jacobi pcg (PRE = true) solve takes: the only place that knows CG's switches and size
// limits.  Three steps, because a loop that handed the solve back changes what the next path may do:
//   hipk_cg_path_begin   before the iteration loop: small, streams, flat_dir and the mid loop
//   hipk_cg_path_lds     after the mid loop (mid_done: it finished the solve): the LDS loop
//   hipk_cg_path_two     after both loops (done: one of them finished), at iteration `it`: the two-launch sequence
// What is left is the three-launch sequence (small / streams / flat_dir pick its kernels).
struct hipk_cg_path {
    bool small = false;        // <= 8 reduction chunks: no combine launch, the vector kernels fold the SpMV's tile sums (plain CG)
    bool streams = false;      // plain CG: the vector kernels treat every operand as a stream
    bool flat_dir = false;     // plain CG, with streams: the direction step as a scalars launch + a flat grid
    bool mid = false;          // hipk_cg_mid_kernel: the whole loop in one launch, a workgroup per nch chunks (hipk_cg_mid.h)
    const hipk_mid_entry<hipk_cg_mid_args> *mid_entry = nullptr;
    hipk_mid_plan mid_plan;
    size_t mid_lds = 0;
    int nch = 1, slot_stride = 16, xcd_aware = 1;
    bool lds_loop = false;     // hipk_cg_solve_lds_kernel: the whole loop in one launch, eight workgroups per chunk
    bool spread = false;       // ... spread over the chip (more than 64 workgroups) instead of on ONE XCD
    bool local = false;        // ... hand-offs through that XCD's L2 (a -2 of the kernel: agent scope from then on)
    int64_t max_its = 0;       // iterations one launch of either loop may run
    bool two_launch = false;   // plain CG: hipk_cg2_spmv_kernel + hipk_cg2_update_kernel per iteration
    bool defer_x = false;      // plain CG, three launches: x updated every second iteration (hipk_cg_pdir_kernel / hipk_cg_xdir_kernel)
    bool fuse_update = false;  // plain CG, fp64 stencils: SpMV and update step in one launch (hipk_cg_fuse_update_kernel), two launches in all
    bool fuse_dir = false;     // ... and, with the x update deferred, the direction step as that launch's tail: one launch in all
    bool fuse_keep_p = false;  // ... whose p_k of uniform tiles stays in the walk's registers instead of being loaded again
    void (*fuse_kern)(hipk_spmv_args, hipk_cg_fuse_args) = nullptr;
    hipk_spmv_args fuse_sa;    // ... its SpMV arguments, as hipk_launch_spmv fills them for the kernel it replaces
};

template <typename T, bool PRE>
static hipk_cg_path hipk_cg_path_begin(hipk_csr_s *A, const hipk_params *prm, int64_t maxiter, bool mid_failed, hipStream_t stream) {
    const int64_t n = A->n_rows;
    const int g = A->geom.g;
    hipk_cg_path path;
    if (!PRE) {   // the Jacobi launch sequence has one form: its kernels fold chunk partials and use the default cache policy
        path.small = g <= 8 && !hipk_sw_present("HIPK_CG_NO_SMALL");
        // x, r, p, Ap beyond 1.5 x the 256 MiB Infinity Cache (HIPK_CG_STREAMS=0/1 forces the choice: A/B measurements)
        path.streams = hipk_sw_force("HIPK_CG_STREAMS", hipk_cg_streams_by_size((size_t)n, sizeof(T)));
        // with it, and a vector alone beyond the 256 MiB Infinity Cache, the direction step as a scalars launch + a flat grid
        // (same vectors, same process, per CG iteration: N = 64 M 1079 -> 1011 us; N = 32 M 473 -> 471; N = 16 M, where p still finds
        // room in that cache, 237 -> 246: not taken there).  HIPK_CG_FLAT_DIRECTION=0|1 forces (tools/flat_probe.py, tests)
        path.flat_dir = hipk_sw_force("HIPK_CG_FLAT_DIRECTION", (size_t)n * sizeof(T) > ((size_t)256 << 20));
    }
    // launch-bound systems of 9 .. 512 chunks (fp64, rows of <= 12 entries within a window around their chunk): the whole loop in
    // one launch, one workgroup of 1024 threads per CU; HIPK_CG_MID=0 leaves them to the paths below.
    // (At 9 .. 32 chunks it replaces the eight-workgroups-per-chunk kernel below: 5.0 against 10.7 us per iteration at n = 40 000.)
    // PRE: a chunk per workgroup only, so up to n_cu (and 256) chunks -- hipk_cg_mid_table has no PRE rows of two chunks.
    // plain: a chunk each up to n_cu chunks, two each beyond
    path.nch = (PRE || g <= A->n_cu) ? 1 : 2;
    const int nch = path.nch;
    path.mid_entry = hipk_mid_pick(hipk_cg_mid_table<T>, A->max_row_len, nch, PRE);
    auto mid_lds = [nch](int slots) { return hipk_cg_mid_lds_bytes(slots * HIPK_TILE, nch, PRE, sizeof(T)); };
    // (hipk_mid_eligible last: it builds the handle's window plan on the stream and queries occupancy)
    path.mid = g > kMidMinChunks && g <= (PRE ? kPcgMidMaxChunks : kMidMaxChunks) && (!PRE || g <= A->n_cu) && A->geom.ch == HIPK_BASE_CHUNK &&
               A->op_cb == nullptr && A->crow != nullptr && A->max_row_len <= 12 && prm->profile == 0 && maxiter > 0 && !mid_failed &&
               hipk_sw_enabled("HIPK_CG_MID") && !hipk_sw_present("HIPK_CG_NO_LDS_LOOP") && !hipk_sw_present("HIPK_CG_NO_SMALL") &&
               path.mid_entry && hipk_mid_eligible(A, path.mid_entry, (g + nch - 1) / nch, mid_lds, stream, &path.mid_plan, &path.mid_lds);
    if (path.mid) {
        // a 256-byte line per chunk partial: every workgroup polls every slot, and packed slots are ONE memory channel's hot spot (same
        // box, CG, us per iteration, 256 B / 16 B per slot: 5.1 / 5.8 at 79 chunks, 5.4 / 6.6 at 123, 6.8 / 8.2 at 254; 64 B from 257
        // chunks: 9.65 / 9.95 at 489; 16 B up to 32 chunks: 5.05 / 5.3 at 20) -- HIPK_CG_MID_STRIDE forces
        const int stride = g <= 32 ? 1 : g <= 256 ? 16 : 4;
        // PRE: the two A/B switches of the mid loop are not consulted (historical, kept)
        path.slot_stride = PRE ? stride : (int)hipk_sw_int("HIPK_CG_MID_STRIDE", stride);
        if (path.slot_stride < 1 || path.slot_stride > 16) path.slot_stride = 16;
        path.xcd_aware = PRE || hipk_sw_enabled("HIPK_CG_MID_XCD");
        path.max_its = hipk_sw_int("HIPK_CG_LAUNCH_ITS", 16384, 1);
    }
    return path;
}

// launch-bound systems with short rows: up to 64 workgroups (8 chunks) on ONE XCD, up to 512 (64 chunks, n <= 131072) spread over
// the chip, two per compute unit.  (Measured per iteration, one launch vs three launches: 5.5 vs 16 us at 8 chunks, 10.6 vs 19.9
// at 16, 12.3 vs 16.6 at 32, 18.3 vs 18.3 at 64: the agent-scope hand-offs grow with the workgroup count -- taken up to 32
// chunks, n <= 65536.)  lds_failed: its workgroups once failed to meet (a shared device): do not wait for that verdict again
static void hipk_cg_path_lds(hipk_cg_path &path, const hipk_csr_s *A, const hipk_params *prm, int64_t maxiter, bool mid_done, bool lds_failed) {
    const int g = A->geom.g;
    path.spread = kGmSub * g > 64;
    path.lds_loop = g <= 32 && !hipk_sw_present("HIPK_CG_NO_SMALL") && A->geom.ch == HIPK_BASE_CHUNK && A->max_row_len <= kCgRowRegs &&
                    prm->profile == 0 && maxiter > 0 && kGmSub * g <= (path.spread ? 2 * A->n_cu : 2 * (A->n_cu / 8)) && !lds_failed &&
                    !hipk_sw_present("HIPK_CG_NO_LDS_LOOP") && !(path.spread && hipk_sw_present("HIPK_NO_LDS_SPREAD")) && !mid_done;
    if (path.lds_loop) {
        path.local = !path.spread && !hipk_sw_present("HIPK_CG_LOOP_AGENT");
        path.max_its = hipk_sw_int("HIPK_CG_LAUNCH_ITS", 16384, 1);
    }
}

// launch-bound mid-size systems of plain CG, 33 .. kCg2MaxChunks chunks: TWO launches per iteration, from iteration 0 only (p_0 = r_0
// sits where its first pass reads it) and with room for a fourth vector in the workspace.  cap2: the kernel's tile capacity
static void hipk_cg_path_two(hipk_cg_path &path, const hipk_csr_s *A, const hipk_params *prm, bool done, int64_t it, int cap2, const hipk_cg_layout &lay) {
    const int g = A->geom.g;
    path.two_launch = !done && !path.small && g > 32 && g <= kCg2MaxChunks && A->geom.ch == HIPK_BASE_CHUNK && A->op_cb == nullptr &&
                      A->crow != nullptr && A->max_tile_nnz <= cap2 && A->max_row_len <= HIPK_LONG_ROW && prm->profile == 0 && it == 0 &&
                      hipk_sw_enabled("HIPK_CG_TWO_LAUNCH") && lay.fourth_vector;
}

// the three-launch sequence of plain CG with the x update deferred (hipk_cg_pdir_kernel, hipk_cg_xdir_kernel, hipk_cg_xflush_kernel):
// the general form only (chunk partials, default cache policy), a matrix operand, no per-kernel profile (a profiled solve times
// the kernels it names), room for a fourth vector in the workspace (a size of the streaming policy forced to HIPK_CG_STREAMS=0
// finds none), from any iteration a one-launch loop handed back at.  HIPK_CG_DEFER_X=0: hipk_cg_direction_kernel every iteration
static void hipk_cg_path_defer(hipk_cg_path &path, const hipk_csr_s *A, const hipk_params *prm, bool done, const hipk_cg_layout &lay) {
    path.defer_x = !done && !path.two_launch && !path.small && !path.streams && A->op_cb == nullptr && prm->profile == 0 &&
                   lay.fourth_vector && hipk_sw_enabled("HIPK_CG_DEFER_X");
}

// hipk_cg_fuse_update_kernel in place of the SpMV and hipk_cg_update_kernel, in the deferred-x sequence and in the plain three-launch
// sequence (their direction kernels unchanged): the general form only, fp64, a matrix operand, no per-kernel profile; the handle's
// CG-loop SpMV (sa: y = A p with <p, y>) resolves to the chunk walk of the two-rows-per-lane kernel on chunks of HIPK_BASE_CHUNK
// rows -- today constant-coefficient stencils of 512 < g <= 2048 chunks --; all g workgroups can be resident at once (the
// occupancy API's answer for the fused kernel x compute units; the kernel holds <= 80 SGPRs and <= 64 VGPRs by construction --
// tests/test_gpu_cg_fuse_update.py reads the compiler's report -- because that API answers 8 where the chip admits 7 above 80
// SGPRs: DESIGN section 9); the launch's sequence number fits 31 bits; the collector never gave up on this handle;
// HIPK_CG_FUSE_UPDATE=0|1 forces (read per solve).
// fuse_dir: with the x update deferred (path.defer_x) the direction step runs as that launch's tail, same envelope;
// HIPK_CG_FUSE_DIRECTION=0|1 forces (read per solve).
// fuse_keep_p: the tail takes p_k of the uniform tiles from the walk's registers (hipk_cg_fuse.h, step 7); HIPK_CG_FUSE_KEEP_P=0
// makes it load all of p_k again (read per solve; same bits).
// No gate by chunk count inside that envelope: every run beat every run of the separate kernels at 591, 958 and 1954 chunks (+2 %,
// +6 %, +11.7 %: profiles/cg_fuse_update_ab.md).
template <typename T>
static void hipk_cg_path_fuse(hipk_cg_path &path, hipk_csr_s *A, const hipk_params *prm, bool done, int64_t it, int64_t maxiter,
                              const hipk_spmv_args &sa) {
    path.fuse_update = path.fuse_dir = path.fuse_keep_p = false;
    if (sizeof(T) != 8 || done || path.two_launch || path.small || path.streams || A->op_cb != nullptr || prm->profile != 0 ||
        A->geom.ch != HIPK_BASE_CHUNK || A->geom.g <= kMidMaxChunks || A->cg_fuse_failed || maxiter - it >= ((int64_t)1 << 31) ||
        !hipk_sw_force("HIPK_CG_FUSE_UPDATE", true))
        return;
    if (!hipk_spmv_resolves_wide_chunk(A, sa, &path.fuse_sa)) return;
    path.fuse_kern = A->sell_w == 5 ? hipk_cg_fuse_update_kernel<5> : A->sell_w == 8 ? hipk_cg_fuse_update_kernel<8> : hipk_cg_fuse_update_kernel<4>;
    int occ = 0;
    const bool resident = hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, path.fuse_kern, HIPK_THREADS, 0) == hipSuccess &&
                          (int64_t)occ * A->n_cu >= A->geom.g;
    (void)hipGetLastError();
    path.fuse_update = resident;
    path.fuse_dir = resident && path.defer_x && hipk_sw_force("HIPK_CG_FUSE_DIRECTION", true);
    path.fuse_keep_p = path.fuse_dir && hipk_sw_enabled("HIPK_CG_FUSE_KEEP_P");
}

// {redo, it_done, stop_it} of a host copy of hipk_cg_scal / hipk_pcg_scal (hipk_resident_run)
template <typename S>
static hipk_loop_state hipk_cg_loop_state(const S &h) {
    return {h.ctl.redo, h.ctl.it_done, h.stop_it};
}

// ------------------------------------------------------------------ step API (include/hipk.h)
extern "C" size_t hipk_cg_scal_bytes(void) { return sizeof(hipk_cg_scal); }

static int hipk_step_check(int64_t n_local, int chunk_rows, int g_red, int dtype) {
    HIPK_REQUIRE(n_local > 0, HIPK_ERR_ARG, "n_local must be positive");
    HIPK_REQUIRE(chunk_rows >= HIPK_BASE_CHUNK && chunk_rows % HIPK_BASE_CHUNK == 0, HIPK_ERR_ARG, "chunk_rows");
    HIPK_REQUIRE(g_red >= 1 && g_red <= HIPK_MAX_PARTS, HIPK_ERR_ARG, "g_red out of range");
    HIPK_REQUIRE((n_local + chunk_rows - 1) / chunk_rows <= g_red, HIPK_ERR_ARG, "more local chunks than g_red");
    HIPK_REQUIRE(dtype == HIPK_F64 || dtype == HIPK_F32, HIPK_ERR_UNSUPPORTED, "dtype");
    return HIPK_OK;
}

// The step kernels access their vector operands 16 bytes at a time (hipk_ld / hipk_st), as hipk_dot, hipk_axpy, hipk_dot_parts and
// hipk_spmv_ex do, which refuse an operand that is not 16-byte aligned; so do the step entry points.  A null pointer passes: which
// operands may be null is each entry point's own test.
static int hipk_step_align(const void *a, const void *b, const void *c = nullptr) {
    HIPK_REQUIRE(hipk_aligned16(a) && hipk_aligned16(b) && hipk_aligned16(c), HIPK_ERR_ALIGN, "vector operands must be 16-byte aligned");
    return HIPK_OK;
}

extern "C" int hipk_cg_start(int64_t n_local, int chunk_rows, int g_red, void *scal_dev, const double *part_rr,
                             const double *part_bb, const void *r, void *p, int dtype, double tol, double atol,
                             int64_t maxiter, hipk_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    int rc = hipk_step_check(n_local, chunk_rows, g_red, dtype);
    if (rc != HIPK_OK) return rc;
    HIPK_REQUIRE(scal_dev && part_rr && part_bb && r && p, HIPK_ERR_ARG, "null argument");
    if ((rc = hipk_step_align(r, p)) != HIPK_OK) return rc;
    const float tolf = (float)tol, atolf = (float)atol;
    const double tol2 = (double)(tolf * tolf), atol_sq = (double)(atolf * atolf);
    const int grid = (int)((n_local + chunk_rows - 1) / chunk_rows);
    if (dtype == HIPK_F64)
        hipk_cg_start_kernel<double><<<grid, HIPK_THREADS, 0, stream>>>(n_local, chunk_rows, g_red, (hipk_cg_scal *)scal_dev,
                                                                         part_rr, part_bb, (const double *)r, (double *)p,
                                                                         tol2, atol_sq, maxiter);
    else
        hipk_cg_start_kernel<float><<<grid, HIPK_THREADS, 0, stream>>>(n_local, chunk_rows, g_red, (hipk_cg_scal *)scal_dev,
                                                                        part_rr, part_bb, (const float *)r, (float *)p, tol2,
                                                                        atol_sq, maxiter);
    HIPK_CHECK_HIP(hipGetLastError());
    return HIPK_OK;
}

extern "C" int hipk_cg_update(int64_t n_local, int chunk_rows, int g_red, const void *scal_dev, int64_t it,
                              const double *part_pAp, const void *Ap, void *r, double *part_rr_out, int dtype,
                              hipk_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    int rc = hipk_step_check(n_local, chunk_rows, g_red, dtype);
    if (rc != HIPK_OK) return rc;
    HIPK_REQUIRE(scal_dev && part_pAp && Ap && r && part_rr_out, HIPK_ERR_ARG, "null argument");
    if ((rc = hipk_step_align(Ap, r)) != HIPK_OK) return rc;
    const int grid = (int)((n_local + chunk_rows - 1) / chunk_rows);
    if (dtype == HIPK_F64)
        hipk_cg_update_kernel<double><<<grid, HIPK_THREADS, 0, stream>>>(n_local, chunk_rows, g_red,
                                                                          (const hipk_cg_scal *)scal_dev, it, part_pAp,
                                                                          (const double *)Ap, (double *)r, part_rr_out);
    else
        hipk_cg_update_kernel<float><<<grid, HIPK_THREADS, 0, stream>>>(n_local, chunk_rows, g_red,
                                                                         (const hipk_cg_scal *)scal_dev, it, part_pAp,
                                                                         (const float *)Ap, (float *)r, part_rr_out);
    HIPK_CHECK_HIP(hipGetLastError());
    return HIPK_OK;
}

extern "C" int hipk_cg_direction(int64_t n_local, int chunk_rows, int g_red, void *scal_dev, int64_t it,
                                 int64_t maxiter, const double *part_pAp, const double *part_rr, const void *r, void *p,
                                 void *x, int dtype, hipk_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    int rc = hipk_step_check(n_local, chunk_rows, g_red, dtype);
    if (rc != HIPK_OK) return rc;
    HIPK_REQUIRE(scal_dev && part_pAp && part_rr && r && p, HIPK_ERR_ARG, "null argument");   // x == NULL: p only (see hipk_cg_xupdate)
    if ((rc = hipk_step_align(r, p, x)) != HIPK_OK) return rc;
    const int grid = (int)((n_local + chunk_rows - 1) / chunk_rows);
    if (dtype == HIPK_F64 && x)
        hipk_cg_direction_kernel<double><<<grid, HIPK_THREADS, 0, stream>>>(n_local, chunk_rows, g_red,
                                                                             (hipk_cg_scal *)scal_dev, it, maxiter,
                                                                             part_pAp, part_rr, (const double *)r,
                                                                             (double *)p, (double *)x);
    else if (dtype == HIPK_F64)
        hipk_cg_direction_kernel<double, false, false, true><<<grid, HIPK_THREADS, 0, stream>>>(
            n_local, chunk_rows, g_red, (hipk_cg_scal *)scal_dev, it, maxiter, part_pAp, part_rr, (const double *)r, (double *)p, nullptr);
    else if (x)
        hipk_cg_direction_kernel<float><<<grid, HIPK_THREADS, 0, stream>>>(n_local, chunk_rows, g_red,
                                                                            (hipk_cg_scal *)scal_dev, it, maxiter,
                                                                            part_pAp, part_rr, (const float *)r,
                                                                            (float *)p, (float *)x);
    else
        hipk_cg_direction_kernel<float, false, false, true><<<grid, HIPK_THREADS, 0, stream>>>(
            n_local, chunk_rows, g_red, (hipk_cg_scal *)scal_dev, it, maxiter, part_pAp, part_rr, (const float *)r, (float *)p, nullptr);
    HIPK_CHECK_HIP(hipGetLastError());
    return HIPK_OK;
}

extern "C" int hipk_cg_xupdate(int64_t n_local, int chunk_rows, int g_red, const void *scal_dev, int64_t it,
                               const double *part_pAp, const void *p, void *x, int dtype, hipk_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    int rc = hipk_step_check(n_local, chunk_rows, g_red, dtype);
    if (rc != HIPK_OK) return rc;
    HIPK_REQUIRE(scal_dev && part_pAp && p && x, HIPK_ERR_ARG, "null argument");
    if ((rc = hipk_step_align(p, x)) != HIPK_OK) return rc;
    const int grid = (int)((n_local + chunk_rows - 1) / chunk_rows);
    if (dtype == HIPK_F64)
        hipk_cg_xupdate_kernel<double><<<grid, HIPK_THREADS, 0, stream>>>(n_local, chunk_rows, g_red, (const hipk_cg_scal *)scal_dev, it,
                                                                          part_pAp, (const double *)p, (double *)x);
    else
        hipk_cg_xupdate_kernel<float><<<grid, HIPK_THREADS, 0, stream>>>(n_local, chunk_rows, g_red, (const hipk_cg_scal *)scal_dev, it,
                                                                         part_pAp, (const float *)p, (float *)x);
    HIPK_CHECK_HIP(hipGetLastError());
    return HIPK_OK;
}

// ---- step API for CG with a CALLABLE preconditioner ("arbitrary callable M between fused kernels") ----
// The host drives  SpMV+<p,Ap> | hipk_cg_update (r, <r,r>) | z = M(r) by the caller, any device code on the same
// stream | hipk_dot_parts(r, z) | hipk_cgm_direction.  gamma = <r,z> steers alpha and beta, the stop test uses
// rs = <r,r> (TSL:835-841); the arithmetic per element is hipk_pcg_direction_kernel's with z read instead of formed,
// so M = (r -> dinv * r) reproduces hipk_pcg_solve bit for bit.
template <typename T>
__global__ __launch_bounds__(HIPK_THREADS) void hipk_cgm_start_kernel(
    int64_t n, int ch, int g, hipk_cg_scal *__restrict__ scal, const double *__restrict__ part_rz,
    const double *__restrict__ part_rr, const double *__restrict__ part_bb, const T *__restrict__ z, T *__restrict__ p,
    double tol2, double atol_sq, int64_t maxiter) {
    __shared__ double sbuf[2 * HIPK_THREADS];
    double gamma0, rr0;
    hipk_reduce_parts2(part_rz, part_rr, g, gamma0, rr0, sbuf);
    const double bs = hipk_reduce_parts(part_bb, g, sbuf);
    hipk_chunk_loop<T>(n, ch, blockIdx.x, [&](int64_t i, int nv) {
        T zv[hipk_vec<T>::VEC];
        hipk_ld<T>(z, i, nv, zv);
        hipk_st<T>(p, i, nv, zv);  // p0 = z0 (TSL:822)
    });
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const double a2 = tol2 * bs;
        const double atol2 = (a2 > atol_sq) ? a2 : atol_sq;
        scal->gamma[0] = gamma0;
        scal->gamma[1] = 0.0;
        scal->atol2 = atol2;
        scal->bs = bs;
        scal->stop_it = (maxiter <= 0 || rr0 <= atol2) ? 0 : INT64_MAX;  // TSL:841 before the first SpMV
        scal->host_sig = nullptr;
    }
}

template <typename T>
__global__ __launch_bounds__(HIPK_THREADS) void hipk_cgm_direction_kernel(
    int64_t n, int ch, int g, hipk_cg_scal *__restrict__ scal, int64_t it, int64_t maxiter,
    const double *__restrict__ part_pAp, const double *__restrict__ part_rz, const double *__restrict__ part_rr,
    const T *__restrict__ z, T *__restrict__ p, T *__restrict__ x) {
    const int c = blockIdx.x;
    hipk_pre<T, 2> pre;
    pre.issue(n, ch, c, {z, (const T *)p});
    if (it >= scal->stop_it) return;
    __shared__ double sbuf[2 * HIPK_THREADS];
    double pAp, gamma_new;
    hipk_reduce_parts2(part_pAp, part_rz, g, pAp, gamma_new, sbuf);
    const double rr = hipk_reduce_parts(part_rr, g, sbuf);
    const double gamma = scal->gamma[it & 1];
    const T alpha = (T)(gamma / pAp);       // the bits hipk_cg_update_kernel derived
    const T beta = (T)(gamma_new / gamma);  // TSL:851
    pre.run([&](int64_t i, int nv, T(&v)[2][hipk_vec<T>::VEC]) {
        constexpr int VEC = hipk_vec<T>::VEC;
        T xv[VEC], pv[VEC];
        hipk_ld<T>((const T *)x, i, nv, xv);
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const T m0 = alpha * v[1][k];
            xv[k] = xv[k] + m0;  // TSL:847
            const T m = beta * v[1][k];
            pv[k] = v[0][k] + m;  // TSL:852
        }
        hipk_st<T>(x, i, nv, xv);
        hipk_st<T>(p, i, nv, pv);
    });
    if (c == 0 && threadIdx.x == 0) {
        scal->gamma[(it + 1) & 1] = gamma_new;
        if (it + 1 >= maxiter || rr <= scal->atol2) scal->stop_it = it + 1;  // TSL:841 for the next pass
    }
}

extern "C" int hipk_cgm_start(int64_t n_local, int chunk_rows, int g_red, void *scal_dev, const double *part_rz,
                              const double *part_rr, const double *part_bb, const void *z, void *p, int dtype,
                              double tol, double atol, int64_t maxiter, hipk_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    int rc = hipk_step_check(n_local, chunk_rows, g_red, dtype);
    if (rc != HIPK_OK) return rc;
    HIPK_REQUIRE(scal_dev && part_rz && part_rr && part_bb && z && p, HIPK_ERR_ARG, "null argument");
    if ((rc = hipk_step_align(z, p)) != HIPK_OK) return rc;
    const float tolf = (float)tol, atolf = (float)atol;
    const double tol2 = (double)(tolf * tolf), atol_sq = (double)(atolf * atolf);
    const int grid = (int)((n_local + chunk_rows - 1) / chunk_rows);
    if (dtype == HIPK_F64)
        hipk_cgm_start_kernel<double><<<grid, HIPK_THREADS, 0, stream>>>(n_local, chunk_rows, g_red, (hipk_cg_scal *)scal_dev,
                                                                          part_rz, part_rr, part_bb, (const double *)z,
                                                                          (double *)p, tol2, atol_sq, maxiter);
    else
        hipk_cgm_start_kernel<float><<<grid, HIPK_THREADS, 0, stream>>>(n_local, chunk_rows, g_red, (hipk_cg_scal *)scal_dev,
                                                                         part_rz, part_rr, part_bb, (const float *)z,
                                                                         (float *)p, tol2, atol_sq, maxiter);
    HIPK_CHECK_HIP(hipGetLastError());
    return HIPK_OK;
}

extern "C" int hipk_cgm_direction(int64_t n_local, int chunk_rows, int g_red, void *scal_dev, int64_t it, int64_t maxiter,
                                  const double *part_pAp, const double *part_rz, const double *part_rr, const void *z,
                                  void *p, void *x, int dtype, hipk_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    int rc = hipk_step_check(n_local, chunk_rows, g_red, dtype);
    if (rc != HIPK_OK) return rc;
    HIPK_REQUIRE(scal_dev && part_pAp && part_rz && part_rr && z && p && x, HIPK_ERR_ARG, "null argument");
    if ((rc = hipk_step_align(z, p, x)) != HIPK_OK) return rc;
    const int grid = (int)((n_local + chunk_rows - 1) / chunk_rows);
    if (dtype == HIPK_F64)
        hipk_cgm_direction_kernel<double><<<grid, HIPK_THREADS, 0, stream>>>(
            n_local, chunk_rows, g_red, (hipk_cg_scal *)scal_dev, it, maxiter, part_pAp, part_rz, part_rr, (const double *)z,
            (double *)p, (double *)x);
    else
        hipk_cgm_direction_kernel<float><<<grid, HIPK_THREADS, 0, stream>>>(
            n_local, chunk_rows, g_red, (hipk_cg_scal *)scal_dev, it, maxiter, part_pAp, part_rz, part_rr, (const float *)z,
            (float *)p, (float *)x);
    HIPK_CHECK_HIP(hipGetLastError());
    return HIPK_OK;
}

// =====================================================================================================
// CG with a Jacobi preconditioner, M = diag(dinv)  (TSL:806-856 with `M is not _identity`).
// z = M r is never stored: the update kernel forms it for <r,z>, the direction kernel forms it again (same
// operands, same bits) for p = z + beta p.  gamma = <r,z> drives alpha and beta; the stop test uses rs = <r,r>
// (TSL:835-841); the final `info` compares ||M (b - A x)|| (TSL:1007).  Per iteration: SpMV + 32 n + 48 n bytes
// (16 n more than plain CG: dinv is read by both vector kernels).  Mirrored by orc_pcg_jacobi.
//   partial slots: a <p,Ap> | b <r,r> | c spare dot of the SpMV | z0, z1 <r,z> ping-pong (read by all workgroups
//   of the update kernel while the early ones already write the next one) | d <b,b> / <x,x>
struct hipk_pcg_scal {
    double atol2, bs, res2, xx, rs_last;
    int64_t stop_it;
    int64_t *host_sig;  // as in hipk_cg_scal
    int64_t pad;
    double gamma[2];    // hipk_cg_solve_lds_kernel<.., PRE>: <r,z> by iteration parity (the launch sequence keeps it as partials)
    hipk_lds_ctl ctl;
};
static_assert(sizeof(hipk_pcg_scal) <= 256, "the scalar block is 256 bytes");

template <typename T>
__global__ __launch_bounds__(HIPK_THREADS) void hipk_pcg_start_kernel(
    int64_t n, int ch, int g, hipk_pcg_scal *__restrict__ scal, const double *__restrict__ part_rr,
    const double *__restrict__ part_bb, const T *__restrict__ r, const T *__restrict__ dinv, T *__restrict__ p,
    double *__restrict__ part_rz, double tol2, double atol_sq, int64_t maxiter, int64_t *host_sig) {
    __shared__ double sbuf[2 * HIPK_THREADS];
    double rr0, bs;
    hipk_reduce_parts2(part_rr, part_bb, g, rr0, bs, sbuf);
    const int c = blockIdx.x;
    double acc = 0.0;
    hipk_chunk_loop<T>(n, ch, c, [&](int64_t i, int nv) {
        constexpr int VEC = hipk_vec<T>::VEC;
        T rv[VEC], dv[VEC], zv[VEC];
        hipk_ld<T>(r, i, nv, rv);
        hipk_ld<T>(dinv, i, nv, dv);
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            zv[k] = dv[k] * rv[k];  // z0 = M r0 (TSL:821)
            if (k < nv) acc = fma((double)rv[k], (double)zv[k], acc);  // gamma0 = <r0, z0> (TSL:826)
        }
        hipk_st<T>(p, i, nv, zv);  // p0 = z0
    });
    acc = hipk_block_sum(acc, sbuf);
    if (threadIdx.x == 0) part_rz[c] = acc;
    if (c == 0 && threadIdx.x == 0) {
        const double a2 = tol2 * bs;
        const double atol2 = (a2 > atol_sq) ? a2 : atol_sq;
        scal->atol2 = atol2;
        scal->bs = bs;
        scal->rs_last = rr0;
        const bool done = (maxiter <= 0 || rr0 <= atol2);  // TSL:841 before the first SpMV
        scal->stop_it = done ? 0 : INT64_MAX;
        scal->host_sig = host_sig;
        if (done) hipk_signal(host_sig, HIPK_SIG_STOP);
    }
}

template <typename T>
__global__ __launch_bounds__(HIPK_THREADS) void hipk_pcg_update_kernel(
    int64_t n, int ch, int g, const hipk_pcg_scal *__restrict__ scal, int64_t it, const double *__restrict__ part_pAp,
    const double *__restrict__ part_rz_in, const T *__restrict__ Ap, const T *__restrict__ dinv, T *__restrict__ r,
    double *__restrict__ part_rr, double *__restrict__ part_rz_out) {
    const int c = blockIdx.x;
    hipk_pre<T, 2> pre;
    pre.issue(n, ch, c, {Ap, (const T *)r});
    if (it >= scal->stop_it) return;
    __shared__ double sbuf[2 * HIPK_THREADS];
    double pAp, gamma;
    hipk_reduce_parts2(part_pAp, part_rz_in, g, pAp, gamma, sbuf);
    const T alpha = (T)(gamma / pAp);  // TSL:846
    double acc0 = 0.0, acc1 = 0.0;
    pre.run([&](int64_t i, int nv, T(&v)[2][hipk_vec<T>::VEC]) {
        constexpr int VEC = hipk_vec<T>::VEC;
        T rv[VEC], dv[VEC];
        hipk_ld<T>(dinv, i, nv, dv);
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const T m1 = alpha * v[0][k];
            rv[k] = v[1][k] - m1;        // TSL:848
            const T z = dv[k] * rv[k];   // TSL:849
            if (k < nv) {
                acc0 = fma((double)rv[k], (double)rv[k], acc0);  // rs of the next test (TSL:838)
                acc1 = fma((double)rv[k], (double)z, acc1);      // TSL:850
            }
        }
        hipk_st<T>(r, i, nv, rv);
    });
    hipk_block_sum2(acc0, acc1, sbuf);
    if (threadIdx.x == 0) {
        part_rr[c] = acc0;
        part_rz_out[c] = acc1;
    }
}

template <typename T>
__global__ __launch_bounds__(HIPK_THREADS) void hipk_pcg_direction_kernel(
    int64_t n, int ch, int g, hipk_pcg_scal *__restrict__ scal, int64_t it, int64_t maxiter,
    const double *__restrict__ part_pAp, const double *__restrict__ part_rz_old, const double *__restrict__ part_rz_new,
    const double *__restrict__ part_rr, const T *__restrict__ r, const T *__restrict__ dinv, T *__restrict__ p,
    T *__restrict__ x) {
    const int c = blockIdx.x;
    hipk_pre<T, 1> pre;  // four operand streams: one early operand keeps the kernel at 8 workgroups per CU
    pre.issue(n, ch, c, {(const T *)p});
    if (it >= scal->stop_it) return;
    __shared__ double sbuf[2 * HIPK_THREADS];
    double pAp, gamma, gamma_new, rr;
    hipk_reduce_parts2(part_pAp, part_rz_old, g, pAp, gamma, sbuf);
    hipk_reduce_parts2(part_rz_new, part_rr, g, gamma_new, rr, sbuf);
    const T alpha = (T)(gamma / pAp);       // the bits hipk_pcg_update_kernel derived
    const T beta = (T)(gamma_new / gamma);  // TSL:851
    pre.run([&](int64_t i, int nv, T(&v)[1][hipk_vec<T>::VEC]) {
        constexpr int VEC = hipk_vec<T>::VEC;
        T rv[VEC], xv[VEC], dv[VEC], pv[VEC];
        hipk_ld<T>(r, i, nv, rv);
        hipk_ld<T>((const T *)x, i, nv, xv);
        hipk_ld<T>(dinv, i, nv, dv);
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const T m0 = alpha * v[0][k];
            xv[k] = xv[k] + m0;              // TSL:847
            const T z = dv[k] * rv[k];       // TSL:849 again
            const T m = beta * v[0][k];
            pv[k] = z + m;                   // TSL:852
        }
        hipk_st<T>(x, i, nv, xv);
        hipk_st<T>(p, i, nv, pv);
    });
    if (c == 0 && threadIdx.x == 0) {
        scal->rs_last = rr;
        const bool done = (it + 1 >= maxiter || rr <= scal->atol2);  // TSL:841 for the next pass
        if (done) scal->stop_it = it + 1;
        hipk_signal(scal->host_sig, done ? (HIPK_SIG_STOP | (it + 1)) : (it + 1));
    }
}

// partials of || dinv .* res ||^2   (final `_norm(M(b - A x))`, TSL:1007)
template <typename T>
__global__ __launch_bounds__(HIPK_THREADS) void hipk_pcg_resnorm_kernel(int64_t n, int ch, const T *__restrict__ res,
                                                                        const T *__restrict__ dinv,
                                                                        double *__restrict__ part) {
    __shared__ double sbuf[HIPK_THREADS];
    const int c = blockIdx.x;
    double acc = 0.0;
    hipk_chunk_loop<T>(n, ch, c, [&](int64_t i, int nv) {
        constexpr int VEC = hipk_vec<T>::VEC;
        T rv[VEC], dv[VEC];
        hipk_ld<T>(res, i, nv, rv);
        hipk_ld<T>(dinv, i, nv, dv);
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const T m = dv[k] * rv[k];
            if (k < nv) acc = fma((double)m, (double)m, acc);
        }
    });
    acc = hipk_block_sum(acc, sbuf);
    if (threadIdx.x == 0) part[c] = acc;
}

__global__ __launch_bounds__(HIPK_THREADS) void hipk_pcg_final_kernel(hipk_pcg_scal *__restrict__ scal, int g,
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

// hipk_last_cg_fused_directions (include/hipk.h): the iterations of this thread's last CG solve whose direction step ran as the
// tail of hipk_cg_fuse_update_kernel
static thread_local int64_t hipk_cg_fused_directions = 0;
extern "C" int hipk_last_cg_fused_directions(void) { return (int)(hipk_cg_fused_directions > INT32_MAX ? INT32_MAX : hipk_cg_fused_directions); }
// hipk_last_cg_fused_kept_p: ... and those of them whose launch had keep_p set
static thread_local int64_t hipk_cg_fused_kept_p = 0;
extern "C" int hipk_last_cg_fused_kept_p(void) { return (int)(hipk_cg_fused_kept_p > INT32_MAX ? INT32_MAX : hipk_cg_fused_kept_p); }

// what the three-launch sequence of plain CG launches for its update and direction steps (hipk_cg_steps::pick)
template <typename T>
struct hipk_cg_kernels {
    decltype(&hipk_cg_update_kernel<T>) update;
    decltype(&hipk_cg_direction_kernel<T>) direction;   // null: the flat form, hipk_cg_scalars_kernel + hipk_cg_direction_flat_kernel
    const double *pap;   // what they fold <p,Ap> from: the chunk partials, or (small) the SpMV's tile sums
    int ntiles;          // small: the tile count; else 0
    const char *form;
};

// One single-device solve of hipk_cg_solve (PRE = false) or hipk_pcg_solve (PRE = true, M = diag(dinv)): its operands, workspace
// and state, and the steps hipk_cg_solve_t and hipk_pcg_solve_t drive it through.
template <typename T, bool PRE>
struct hipk_cg_steps {
    typedef typename std::conditional<PRE, hipk_pcg_scal, hipk_cg_scal>::type S;
    static constexpr int kCap2 = sizeof(T) == 8 ? 1280 : 2048;   // the tile capacity of hipk_cg2_spmv_kernel
    hipk_csr_s *A;
    const T *dinv, *b;
    T *x;
    const hipk_params *prm;
    hipStream_t stream;
    const int64_t n, maxiter;
    const hipk_geom gm;
    const int ntiles;
    const hipk_cg_layout lay;
    char *const work;
    S *const scal = hipk_at<S>(work, lay.scal);
    double *const part_a = hipk_at<double>(work, lay.part_a), *const part_b = hipk_at<double>(work, lay.part_b);
    double *const part_c = hipk_at<double>(work, lay.part_c), *const part_d = hipk_at<double>(work, lay.part_d);
    double *const part_z[2] = {hipk_at<double>(work, lay.part_z[0]), hipk_at<double>(work, lay.part_z[1])};
    T *const r = hipk_at<T>(work, lay.r), *const p = hipk_at<T>(work, lay.p), *const Ap = hipk_at<T>(work, lay.Ap);
    hipk_spmv_args sa = hipk_spmv_base(A);   // the SpMV of an iteration, Ap = A p with <p,Ap>
    hipk_event_pair whole;
    hipk_spmv_profiler prof;
    hipk_pacer pace;
    hipk_cg_path path;
    int64_t it = 0, stop = INT64_MAX;
    bool done = false;       // a one-launch loop finished the solve
    char handed[128] = "";   // the one-launch loops that handed this solve back
    int p_first = 0;         // deferred x: which of {p, p2} holds p_it when the sequence begins (1 after a fused sequence gave up
                             // an odd number of iterations into it)

    // profile: the KIND of kernel whose durations are reported (hipk_spmv_profiler; only launches of it carry events), 0: none
    hipk_cg_steps(hipk_csr_s *A_, const T *dinv_, const T *b_, T *x_, char *w, const hipk_params *prm_, hipStream_t s_, int profile)
        : A(A_), dinv(dinv_), b(b_), x(x_), prm(prm_), stream(s_), n(A_->n_rows), maxiter(hipk_default_maxiter(prm_, A_->n_rows)), gm(A_->geom),
          ntiles((int)((A_->n_rows + HIPK_TILE - 1) / HIPK_TILE)), lay(hipk_cg_make_layout(A_->n_rows, A_->dtype, PRE)), work(w), prof(profile),
          pace(A_->host_poll, &scal->stop_it, prm_->check_every > 0 ? prm_->check_every : 64) {}

    // y = b - A x; the chunk partials of its squared norm in part_yy, or (null) none
    int residual(T *y, double *part_yy) const {
        hipk_spmv_args sr = sa;   // the handle's arrays and geometry; everything an iteration's SpMV sets is set again
        sr.x = x;
        sr.y = y;
        sr.mode = HIPK_SPMV_RESID | (part_yy ? HIPK_SPMV_DOT_YY : 0);
        sr.w = nullptr;
        sr.bsub = b;
        sr.part0 = part_c;
        sr.part1 = part_yy ? part_yy : part_c;
        sr.stop_it = nullptr;
        sr.skip_combine = 0;
        return hipk_launch_spmv(A, sr, stream);
    }

    // r0 = b - A x0 with <r0,r0> partials (TSL:820, 826); <b,b> partials (TSL:815); p0 (PRE: z0 = M r0, p0 = z0, the partials of
    // gamma0 = <r0,z0> in part_z[0]), the stop word and the tolerances
    int start() {
        hipk_set_solve_path(nullptr, "");
        HIPK_CHECK_HIP(whole.create());
        HIPK_CHECK_HIP(hipEventRecord(whole.a, stream));
        HIPK_TRY(residual(r, part_b));
        HIPK_TRY(hipk_launch_dot_parts(n, b, b, A->dtype, part_d, stream));
        HIPK_CHECK_HIP(pace.create());   // zeroes the pinned signal word: before the kernel that may write it is enqueued
        const hipk_tol_sq tol(prm);
        if constexpr (PRE)
            hipk_pcg_start_kernel<T><<<gm.g, HIPK_THREADS, 0, stream>>>(n, gm.ch, gm.g, scal, part_b, part_d, r, dinv, p, part_z[0], tol.tol2,
                                                                         tol.atol_sq, maxiter, pace.device_sig());
        else
            hipk_cg_start_kernel<T><<<gm.g, HIPK_THREADS, 0, stream>>>(n, gm.ch, gm.g, scal, part_b, part_d, r, p, tol.tol2, tol.atol_sq, maxiter,
                                                                        pace.device_sig());
        HIPK_CHECK_HIP(hipGetLastError());
        sa.x = p;
        sa.y = Ap;
        sa.mode = HIPK_SPMV_DOT_W;
        sa.w = p;
        sa.part0 = part_a;
        sa.part1 = part_c;
        sa.stop_it = &scal->stop_it;
        return HIPK_OK;
    }

    // launch-bound mid-size systems: the whole loop in one launch, path.mid_entry's kernel on workgroups of path.nch chunks, from
    // iteration `it` -- HIPK_OK, HIPK_HANDED_BACK or an error (hipk_resident_run); failed: the caller's latch
    int mid_loop(bool &failed, const char *entry) {
        const hipk_mid_entry<hipk_cg_mid_args> *mid = path.mid_entry;
        const size_t lds = path.mid_lds;
        const int grid = (gm.g + mid->nch - 1) / mid->nch;
        hipk_cg_mid_args ca;
        memset(&ca, 0, sizeof(ca));
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
        ca.r_ll = hipk_at<unsigned long long>(work, lay.r_ll);
        ca.pap_ll = hipk_at<unsigned long long>(work, lay.pap_ll);
        ca.rr_ll = hipk_at<unsigned long long>(work, lay.rr_ll);
        if (PRE) ca.rz_ll = hipk_at<unsigned long long>(work, lay.rz_ll);
        ca.dinv = dinv;
        ca.rz0_parts = PRE ? part_z[0] : nullptr;
        ca.slot_stride = path.slot_stride;
        ca.xcd_aware = path.xcd_aware;
        ca.ctl = &scal->ctl;
        ca.gamma = scal->gamma;
        ca.atol2 = &scal->atol2;
        ca.stop_it = &scal->stop_it;
        ca.maxiter = maxiter;
        ca.max_its = path.max_its;
        auto launch = [&](int64_t it0, int test_not_resident, bool) -> int {
            ca.it0 = it0;
            ca.test_not_resident = test_not_resident;
            HIPK_CHECK_HIP(hipMemsetAsync(ca.r_ll, 0, lay.ll_bytes, stream));
            HIPK_CHECK_HIP(hipMemsetAsync(ca.pap_ll, 0, PRE ? kPcgMidSlotBytes : kMidSlotBytes, stream));
            HIPK_CHECK_HIP(hipMemsetAsync(&scal->ctl, 0, sizeof(hipk_lds_ctl), stream));
            mid->kern<<<hipk_xcd_grid(grid), 1024, lds, stream>>>(ca);   // hipk_xcd_chunk: padded to a multiple of 8
            return HIPK_OK;
        };
        return hipk_resident_run(stream, scal, launch, hipk_cg_loop_state<S>, it, maxiter, nullptr, failed, handed, mid->name, entry);
    }

    // launch-bound systems with short rows: the whole loop in one launch, hipk_cg_solve_lds_kernel, from iteration `it` -- as
    // mid_loop; *form: the instantiation of its last launch (hipk_last_solve_form)
    int lds_loop(bool &failed, const char *entry, const char **form) {
        bool local = path.local;   // a -2 (spread over several XCDs): agent-scope hand-offs
        const int lgrid = path.spread ? kGmSub * gm.g : 8 * kGmSub * gm.g;
        hipk_cg_lds_args<T> ca;
        ca.n = n;
        ca.g = gm.g;
        ca.crow = A->crow;
        ca.col = A->col;
        ca.val = (const T *)A->val;
        ca.x = x;
        ca.r = r;
        ca.p = p;
        ca.Ap = Ap;
        ca.ctl = &scal->ctl;
        ca.gamma = scal->gamma;
        ca.atol2 = &scal->atol2;
        ca.stop_it = &scal->stop_it;
        ca.dinv = dinv;
        ca.rz0_parts = PRE ? part_z[0] : nullptr;
        ca.rz_sub = PRE ? hipk_at<double>(work, lay.lds_rz_sub) : nullptr;
        ca.tile_pp = A->tile_part;
        ca.rr_sub = hipk_at<double>(work, lay.lds_rr_sub);
        ca.flag_a = hipk_at<unsigned long long>(work, lay.lds_flags);
        ca.flag_b = ca.flag_a + kHoMaxWg;
        ca.spread = path.spread ? 1 : 0;
        ca.maxiter = maxiter;
        ca.max_its = path.max_its;
        auto launch = [&](int64_t it0, int test_not_resident, bool loc) -> int {
            ca.it0 = it0;
            ca.test_not_resident = test_not_resident;
            HIPK_CHECK_HIP(hipMemsetAsync(ca.flag_a, 0, 2 * kHoMaxWg * sizeof(unsigned long long), stream));
            HIPK_CHECK_HIP(hipMemsetAsync(&scal->ctl, 0, sizeof(hipk_lds_ctl), stream));
            (loc ? hipk_cg_solve_lds_kernel<T, true, PRE> : hipk_cg_solve_lds_kernel<T, false, PRE>)<<<lgrid, HIPK_THREADS, 0, stream>>>(ca);
            return HIPK_OK;
        };
        const int run = hipk_resident_run(stream, scal, launch, hipk_cg_loop_state<S>, it, maxiter, &local, failed, handed,
                                          "hipk_cg_solve_lds_kernel", entry);
        *form = local ? (PRE ? HIPK_FORM_OF_T(T, "hipk_cg_solve_lds_kernel<", "true,true>") : HIPK_FORM_OF_T(T, "hipk_cg_solve_lds_kernel<", "true,false>"))
                      : (PRE ? HIPK_FORM_OF_T(T, "hipk_cg_solve_lds_kernel<", "false,true>") : HIPK_FORM_OF_T(T, "hipk_cg_solve_lds_kernel<", "false,false>"));
        return run;
    }

    // The one-launch section: the mid loop, else the LDS loop, from iteration `it`; `done` when one of them finished the solve,
    // else the caller's launch sequence goes on from `it` (and names its form).  Records the path hipk_last_solve_path reports.
    // The latches: a one-launch loop once handed a solve back in this process
    int one_launch(bool &mid_failed, bool &lds_failed, const char *entry) {
        path = hipk_cg_path_begin<T, PRE>(A, prm, maxiter, mid_failed, stream);
        sa.skip_combine = path.small ? 1 : 0;
        // a hand-back at it > 0 (from an EARLIER launch of the loop): x, r, p are in memory, but <r,z> only as scal->gamma[it & 1], while
        // the Jacobi launch sequence folds it from the chunk partials part_z[it & 1].  Rebuild that slot as {gamma, 0, 0, ...}: the
        // fold of it is gamma, bit for bit.  (Plain CG's launch sequence reads gamma itself.)
        auto after = [&](int run) -> int {
            if (PRE && run == HIPK_HANDED_BACK && it > 0) {
                HIPK_CHECK_HIP(hipMemsetAsync(part_z[it & 1], 0, (size_t)gm.g * sizeof(double), stream));
                HIPK_CHECK_HIP(hipMemcpyAsync(part_z[it & 1], &scal->gamma[it & 1], sizeof(double), hipMemcpyDeviceToDevice, stream));
            }
            return HIPK_OK;
        };
        bool mid_done = false, lds_done = false;
        const char *lds_form = "";
        if (path.mid) {
            const int run = mid_loop(mid_failed, entry);
            if (run < 0) return run;
            HIPK_TRY(after(run));
            mid_done = run == HIPK_OK;
        }
        hipk_cg_path_lds(path, A, prm, maxiter, mid_done, lds_failed);
        if (path.lds_loop) {   // a hand-back (not co-resident; that launch modified nothing): the launch sequence takes over
            const int run = lds_loop(lds_failed, entry, &lds_form);
            if (run < 0) return run;
            HIPK_TRY(after(run));
            lds_done = run == HIPK_OK;
        }
        done = mid_done || lds_done;
        hipk_set_solve_path(handed, mid_done ? path.mid_entry->name : lds_done ? "hipk_cg_solve_lds_kernel" : "launch sequence");
        if (done) hipk_set_solve_form(mid_done ? path.mid_entry->name : lds_form);
        return HIPK_OK;
    }

    // ---- the launch sequences: the host enqueues iterations a few ahead of the GPU and stops when the direction kernel reports
    // the stop (hipk_pacer, hipk_solve.h); launches past the stop are no-ops on the device.

    // plain CG, 33 .. kCg2MaxChunks chunks: hipk_cg2_spmv_kernel + hipk_cg2_update_kernel per iteration
    int two_launch_sequence() {
        T *pbuf[2] = {p, hipk_at<T>(work, lay.p2)};   // p_0 = r_0 sits in pbuf[0] (start kernel); pass k reads pbuf[k & 1], writes the other
        hipk_cg2_args ca;
        ca.crow = A->crow;
        ca.col = A->col;
        ca.val = A->val;
        ca.n = n;
        ca.ch = gm.ch;
        ca.g = gm.g;
        ca.scal = scal;
        ca.maxiter = maxiter;
        ca.part_rr = part_b;
        ca.r = r;
        ca.Ap = Ap;
        ca.tpart = A->tile_part;
        const int grid1 = ((ntiles + 7) >> 3) << 3;
        // pass `maxiter` is bookkeeping only (its K1 folds the last <r,r>, sets the stop word and gamma: TSL:841 "k >= maxiter")
        for (; it <= maxiter; ++it) {
            HIPK_CHECK_HIP(pace.gate(it, stream, &stop));
            if (stop <= it) break;
            ca.it = it;
            ca.p_old = pbuf[it & 1];
            ca.p_new = pbuf[(it + 1) & 1];
            hipk_cg2_spmv_kernel<T, kCap2><<<grid1, HIPK_THREADS, 0, stream>>>(ca);
            if (it < maxiter)
                hipk_cg2_update_kernel<T><<<gm.g, HIPK_THREADS, 0, stream>>>(n, gm.ch, gm.g, scal, it, A->tile_part, ntiles, Ap,
                                                                            (const T *)pbuf[(it + 1) & 1], r, x, part_b);
            if ((it & 63) == 63) HIPK_CHECK_HIP(hipGetLastError());
        }
        if (it > maxiter) it = maxiter;
        return HIPK_OK;
    }

    // plain CG, three launches with the x update deferred: SpMV, hipk_cg_update_kernel, hipk_cg_pdir_kernel / hipk_cg_xdir_kernel
    int deferred_x_sequence() {
        // p_j of iteration it0 + j lives in pbuf[j & 1]; even j only forms p_{j+1} in the other buffer, odd j also brings x up to date
        T *pbuf[2] = {p_first ? hipk_at<T>(work, lay.p2) : p, p_first ? p : hipk_at<T>(work, lay.p2)};
        const int64_t it0 = it;
        if (path.fuse_update) HIPK_TRY(fuse_begin());
        for (; it < maxiter; ++it) {
            HIPK_CHECK_HIP(pace.gate(it, stream, &stop));
            if (stop <= it) break;
            const int j = (int)((it - it0) & 1);
            if (path.fuse_dir) {   // one launch: the direction step is its tail (odd j: with the x part)
                fuse_launch(it0, pbuf[j], pbuf[j ^ 1], j ? x : nullptr);
                if ((it & 63) == 63) HIPK_CHECK_HIP(hipGetLastError());
                continue;
            }
            if (path.fuse_update) {
                fuse_launch(it0, pbuf[j]);
            } else {
                sa.it = it;
                sa.x = sa.w = pbuf[j];
                HIPK_TRY(hipk_launch_spmv(A, sa, stream, &prof));
                hipk_cg_update_kernel<T><<<gm.g, HIPK_THREADS, 0, stream>>>(n, gm.ch, gm.g, scal, it, part_a, Ap, r, part_b, 0, &scal->alpha[it & 1]);
            }
            if (j == 0)
                hipk_cg_pdir_kernel<T><<<gm.g, HIPK_THREADS, 0, stream>>>(n, gm.ch, gm.g, scal, it, maxiter, part_b, r, pbuf[0], pbuf[1]);
            else
                hipk_cg_xdir_kernel<T><<<gm.g, HIPK_THREADS, 0, stream>>>(n, gm.ch, gm.g, scal, it, maxiter, part_b, r, pbuf[1], pbuf[0], x);
            if ((it & 63) == 63) HIPK_CHECK_HIP(hipGetLastError());
        }
        // an odd number of iterations: the last one's x update is still owed (the device knows how many were completed)
        hipk_cg_xflush_kernel<T><<<gm.g, HIPK_THREADS, 0, stream>>>(n, gm.ch, scal, it, it0, pbuf[0], x, path.fuse_dir ? 1 : 0);
        return path.fuse_update ? fuse_end(it0, true, pbuf) : HIPK_OK;
    }

    // ---- hipk_cg_fuse_update_kernel in place of the SpMV and the update launch (hipk_cg_path_fuse)
    // the sequence begins: the flagged words and the collectors' hand-out lines (one region, the head of Ap) and the give-up word
    int fuse_begin() {
        HIPK_CHECK_HIP(hipMemsetAsync(hipk_at<char>(work, lay.fuse_words), 0, kFuseBytes, stream));
        HIPK_CHECK_HIP(hipMemsetAsync(&scal->ctl, 0, sizeof(hipk_lds_ctl), stream));
        // tests: HIPK_TEST_CG_FUSE_GIVE_UP=k makes the collectors of iteration k behave as if their poll had run out
        fuse_give_up_at = hipk_sw_present("HIPK_TEST_CG_FUSE_GIVE_UP") ? hipk_sw_int("HIPK_TEST_CG_FUSE_GIVE_UP", -1) : -1;
        // ... HIPK_TEST_CG_FUSE_DIR_GIVE_UP=k those of its second hand-off (the direction tail)
        fuse_dir_give_up_at = hipk_sw_present("HIPK_TEST_CG_FUSE_DIR_GIVE_UP") ? hipk_sw_int("HIPK_TEST_CG_FUSE_DIR_GIVE_UP", -1) : -1;
        // ... HIPK_TEST_CG_FUSE_GIVE_UP_WHO=s only collector s of the eight, at either
        const int64_t who = hipk_sw_present("HIPK_TEST_CG_FUSE_GIVE_UP_WHO") ? hipk_sw_int("HIPK_TEST_CG_FUSE_GIVE_UP_WHO", -1) : -1;
        fuse_give_up_who = who >= 0 && who < (int64_t)kFuseCollectors ? 1 << (int)who : (1 << kFuseCollectors) - 1;
        fuse_note();
        return HIPK_OK;
    }
    // the kernel note of the loop's products (hipk_last_spmv_kernel); again after the solve's last residual, which has its own
    void fuse_note() const {
        char name[64];
        snprintf(name, sizeof(name), "hipk_cg_fuse_update_kernel<%d>", A->sell_w);
        hipk_note_spmv_kernel(name);
    }
    // iteration `it` of a sequence that began at it0: Ap = A pk on chip, alpha, r -= alpha Ap, the partials of <r,r>
    // p_next (the direction tail): p_{it+1} = r + beta pk into it, the next pass's gamma, the stop test; xq: also the x part
    void fuse_launch(int64_t it0, const T *pk, T *p_next = nullptr, T *xq = nullptr) {
        hipk_spmv_args fa = path.fuse_sa;
        fa.it = it;
        fa.x = fa.w = pk;
        hipk_cg_fuse_args ff;
        ff.scal = (hipk_cg_scal *)scal;
        ff.r = (double *)r;
        ff.part_rr = part_b;
        ff.part_pap = part_a;
        ff.words = hipk_at<char>(work, lay.fuse_words);
        ff.seq = (unsigned)(it - it0) + 1u;
        ff.give_up = (it == fuse_give_up_at ? fuse_give_up_who : 0) | (p_next != nullptr && it == fuse_dir_give_up_at ? fuse_give_up_who << 8 : 0);
        ff.p_next = (double *)p_next;
        ff.x = (double *)xq;
        ff.maxiter = maxiter;
        ff.keep_p = p_next != nullptr && path.fuse_keep_p ? 1 : 0;
        path.fuse_kern<<<hipk_xcd_grid(gm.g), HIPK_THREADS, 0, stream>>>(fa, ff);
    }
    // the sequence has ended: HIPK_OK, or HIPK_HANDED_BACK when a collector gave up at some iteration -- the state is that
    // iteration's, the latch is set on the handle, the stop word and the pacer are rearmed, and the caller goes on from `it` with
    // the separate kernels.  deferred: the flush has brought x up to date; p of that iteration is where its parity put it
    // A collector of the direction tail gave up (ctl.redo = kFuseDirGaveUp) at iteration K = stop_it, j = K - it0 into the sequence:
    // r, part_rr and alpha_K are K's, p_{K+1} is not stored, the flush has done nothing.  hipk_cg_pdir_kernel finishes K from
    // pbuf[j & 1] into the other buffer (and does its bookkeeping), and the caller goes on at K + 1 with p_{K+1} there.  x: odd j,
    // the tail's x part has brought it up to date through K; even j, it lacks alpha_K p_K only, which the flush kernel adds as
    // the one owed term of a sequence of one iteration begun at K -- so the sequence that goes on owes nothing.
    int fuse_end(int64_t it0, bool deferred, T *const *pbuf = nullptr) {
        S hs;
        HIPK_CHECK_HIP(hipGetLastError());
        HIPK_CHECK_HIP(hipMemcpyAsync(&hs, scal, sizeof(hs), hipMemcpyDeviceToHost, stream));
        HIPK_CHECK_HIP(hipStreamSynchronize(stream));
        const int64_t ran = (hs.stop_it < it ? hs.stop_it : it) - it0;   // iterations this sequence completed
        if (path.fuse_dir) hipk_cg_fused_directions += ran > 0 ? ran : 0;
        if (path.fuse_keep_p) hipk_cg_fused_kept_p += ran > 0 ? ran : 0;
        if (hs.ctl.redo == -3) {
            hipk_set_error("hipk_cg_solve: a collector of the fused SpMV + update launch stopped arriving");
            return HIPK_ERR_HIP;
        }
        const bool dir_gave_up = path.fuse_dir && hs.ctl.redo == kFuseDirGaveUp;
        if (hs.ctl.redo != -1 && !dir_gave_up) return HIPK_OK;
        A->cg_fuse_failed = 1;
        path.fuse_update = path.fuse_dir = path.fuse_keep_p = false;
        it = hs.stop_it;
        stop = INT64_MAX;
        HIPK_CHECK_HIP(hipMemcpyAsync(&scal->stop_it, &stop, sizeof(int64_t), hipMemcpyHostToDevice, stream));
        HIPK_CHECK_HIP(hipMemsetAsync(&scal->ctl, 0, sizeof(hipk_lds_ctl), stream));
        HIPK_CHECK_HIP(hipStreamSynchronize(stream));
        HIPK_CHECK_HIP(pace.resume(it));
        if (dir_gave_up) {
            const int j = (int)((it - it0) & 1);
            hipk_cg_pdir_kernel<T><<<gm.g, HIPK_THREADS, 0, stream>>>(n, gm.ch, gm.g, scal, it, maxiter, part_b, r, pbuf[j], pbuf[j ^ 1]);
            if (j == 0) hipk_cg_xflush_kernel<T><<<gm.g, HIPK_THREADS, 0, stream>>>(n, gm.ch, scal, it + 1, it, pbuf[0], x);
            HIPK_CHECK_HIP(hipGetLastError());
            ++it;
        }
        if (deferred) p_first ^= (int)((it - it0) & 1);
        return HIPK_HANDED_BACK;
    }
    int64_t fuse_give_up_at = -1, fuse_dir_give_up_at = -1;
    int fuse_give_up_who = (1 << kFuseCollectors) - 1;   // bit s: collector s obeys them

    // the kernels of the plain three-launch sequence (hipk_cg_path: small / streams / flat_dir) and the form they make
    hipk_cg_kernels<T> pick() const {
        if (path.small)
            return {hipk_cg_update_kernel<T, true>, hipk_cg_direction_kernel<T, true>, A->tile_part, ntiles, HIPK_FORM("cg three-launch, small")};
        if (path.streams && path.flat_dir)
            return {hipk_cg_update_kernel<T, false, true>, nullptr, part_a, 0, HIPK_FORM("cg three-launch, streams + flat direction")};
        if (path.streams)
            return {hipk_cg_update_kernel<T, false, true>, hipk_cg_direction_kernel<T, false, true>, part_a, 0, HIPK_FORM("cg three-launch, streams")};
        return {hipk_cg_update_kernel<T>, hipk_cg_direction_kernel<T>, part_a, 0, HIPK_FORM("cg three-launch")};
    }

    // plain CG: SpMV, update, direction.  params.profile selects the kernel whose durations are reported (1 SpMV, 2 update,
    // 3 direction -- of the flat form its flat kernel, the step's 40 n bytes --, 4 the scalars launch before that)
    int three_launch_sequence(const hipk_cg_kernels<T> &k) {
        const int64_t it0 = it;
        if (path.fuse_update) HIPK_TRY(fuse_begin());
        for (; it < maxiter; ++it) {
            HIPK_CHECK_HIP(pace.gate(it, stream, &stop));
            if (stop <= it) break;
            if (path.fuse_update) {
                fuse_launch(it0, p);
            } else {
                sa.it = it;
                HIPK_TRY(hipk_launch_spmv(A, sa, stream, &prof));
                hipk_launch_timed(&prof, HIPK_K_UPDATE, k.update, gm.g, HIPK_THREADS, 0, stream, n, gm.ch, gm.g, scal, it, k.pap, Ap, r, part_b, k.ntiles,
                                  (double *)nullptr);
            }
            if (k.direction) {
                hipk_launch_timed(&prof, HIPK_K_DIRECTION, k.direction, gm.g, HIPK_THREADS, 0, stream, n, gm.ch, gm.g, scal, it, maxiter, k.pap, part_b, r,
                                  p, x, k.ntiles);
            } else {
                hipk_launch_timed(&prof, HIPK_K_SCALARS, hipk_cg_scalars_kernel, 1, HIPK_THREADS, 0, stream, gm.g, scal, it, maxiter, part_a, part_b);
                hipk_launch_timed(&prof, HIPK_K_DIRECTION, hipk_cg_direction_flat_kernel<T>, (unsigned)((n + HIPK_BASE_CHUNK - 1) / HIPK_BASE_CHUNK),
                                  HIPK_THREADS, 0, stream, n, scal, it, r, p, x);
            }
            if ((it & 63) == 63) HIPK_CHECK_HIP(hipGetLastError());
        }
        return path.fuse_update ? fuse_end(it0, false) : HIPK_OK;
    }

    // Jacobi PCG: SpMV, hipk_pcg_update_kernel, hipk_pcg_direction_kernel
    int jacobi_sequence() {
        for (; it < maxiter; ++it) {
            HIPK_CHECK_HIP(pace.gate(it, stream, &stop));
            if (stop <= it) break;
            sa.it = it;
            HIPK_TRY(hipk_launch_spmv(A, sa, stream));
            hipk_pcg_update_kernel<T><<<gm.g, HIPK_THREADS, 0, stream>>>(n, gm.ch, gm.g, scal, it, part_a, part_z[it & 1], Ap, dinv, r, part_b,
                                                                          part_z[(it + 1) & 1]);
            hipk_pcg_direction_kernel<T><<<gm.g, HIPK_THREADS, 0, stream>>>(n, gm.ch, gm.g, scal, it, maxiter, part_a, part_z[it & 1],
                                                                             part_z[(it + 1) & 1], part_b, r, dinv, p, x);
            if ((it & 63) == 63) HIPK_CHECK_HIP(hipGetLastError());
        }
        return HIPK_OK;
    }

    // TSL:1007-1014: the true residual (PRE: ||M (b - A x)||) and ||x|| decide info
    int finish(hipk_stats *st) {
        HIPK_CHECK_HIP(hipGetLastError());
        if constexpr (PRE) {
            HIPK_TRY(residual(Ap, nullptr));
            hipk_pcg_resnorm_kernel<T><<<gm.g, HIPK_THREADS, 0, stream>>>(n, gm.ch, Ap, dinv, part_b);
        } else {
            HIPK_TRY(residual(Ap, part_b));
        }
        HIPK_TRY(hipk_launch_dot_parts(n, x, x, A->dtype, part_d, stream));
        if constexpr (PRE)
            hipk_pcg_final_kernel<<<1, HIPK_THREADS, 0, stream>>>(scal, gm.g, part_b, part_d);
        else
            hipk_cg_final_kernel<<<1, HIPK_THREADS, 0, stream>>>(scal, gm.g, part_b, part_d);
        HIPK_CHECK_HIP(hipGetLastError());
        S hs;
        HIPK_CHECK_HIP(hipEventRecord(whole.b, stream));
        HIPK_CHECK_HIP(hipMemcpyAsync(&hs, scal, sizeof(hs), hipMemcpyDeviceToHost, stream));
        HIPK_CHECK_HIP(hipStreamSynchronize(stream));

        const int64_t iterations = (hs.stop_it < it) ? hs.stop_it : it;  // the device's stop word is authoritative
        hipk_finish_isolve_stats(st, prm, hs.bs, hs.res2, hs.xx, iterations, iterations + 2);   // + r0 and the true residual
        if constexpr (PRE)
            st->recurrence_rs = (done && iterations > 0) ? hs.ctl.rs_last : hs.rs_last;
        else
            st->recurrence_rs = hs.gamma[iterations & 1];
        st->breakdown = 0;
        float ms = 0.f;
        HIPK_CHECK_HIP(hipEventElapsedTime(&ms, whole.a, whole.b));
        st->solve_ms = ms;
        HIPK_CHECK_HIP(prof.collect(st, iterations));
        return HIPK_OK;
    }
};

template <typename T>
static int hipk_cg_solve_t(hipk_csr_s *A, const T *b, T *x, char *work, const hipk_params *prm, hipk_stats *st, hipStream_t stream) {
    static bool mid_failed = false, lds_loop_failed = false;   // per dtype; hipk_pcg_solve_t has its own
    hipk_cg_steps<T, false> s(A, nullptr, b, x, work, prm, stream, prm->profile);
    hipk_cg_fused_directions = hipk_cg_fused_kept_p = 0;
    HIPK_TRY(s.start());
    HIPK_TRY(s.one_launch(mid_failed, lds_loop_failed, "hipk_cg_solve"));
    // what is left when neither loop finished: two launches per iteration, else three with the x update deferred, else three
    hipk_cg_path_two(s.path, A, prm, s.done, s.it, s.kCap2, s.lay);
    hipk_cg_path_defer(s.path, A, prm, s.done, s.lay);
    hipk_cg_path_fuse<T>(s.path, A, prm, s.done, s.it, s.maxiter, s.sa);
    if (!s.done) {
        const hipk_cg_kernels<T> k = s.pick();   // (the deferred-x form reports the three-launch form it replaces the direction step of)
        hipk_set_solve_form(!s.path.two_launch ? k.form
                            : sizeof(T) == 8   ? HIPK_FORM("cg two-launch: hipk_cg2_spmv_kernel<double,1280> + hipk_cg2_update_kernel")
                                               : HIPK_FORM("cg two-launch: hipk_cg2_spmv_kernel<float,2048> + hipk_cg2_update_kernel"));
        // (a fused sequence whose collector gave up has handed the solve back at s.it: the same sequence again, separate kernels)
        int run = s.path.two_launch ? s.two_launch_sequence() : s.path.defer_x ? s.deferred_x_sequence() : s.three_launch_sequence(k);
        if (run == HIPK_HANDED_BACK) run = s.path.defer_x ? s.deferred_x_sequence() : s.three_launch_sequence(k);
        HIPK_TRY(run);
    }
    const int rc = s.finish(st);
    if (!s.done && s.path.fuse_update) s.fuse_note();   // the loop's products, not the true residual's, are what a fused solve reports
    return rc;
}

template <typename T>
static int hipk_pcg_solve_t(hipk_csr_s *A, const T *dinv, const T *b, T *x, char *work, const hipk_params *prm, hipk_stats *st, hipStream_t stream) {
    static bool mid_failed = false, lds_loop_failed = false;   // per dtype
    hipk_cg_steps<T, true> s(A, dinv, b, x, work, prm, stream, 0);   // (no per-kernel profile of the Jacobi kernels)
    HIPK_TRY(s.start());
    HIPK_TRY(s.one_launch(mid_failed, lds_loop_failed, "hipk_pcg_solve"));
    if (!s.done) {
        hipk_set_solve_form(HIPK_FORM("pcg three-launch, Jacobi"));
        HIPK_TRY(s.jacobi_sequence());
    }
    return s.finish(st);
}

extern "C" int hipk_cg_solve(hipk_csr_t A, const void *b, void *x, void *work, size_t work_bytes,
                             const hipk_params *prm, hipk_stats *st, hipk_stream_t stream) {
    HIPK_TRY(hipk_solve_check(A, true, nullptr, b, x, work, work_bytes, hipk_cg_work_bytes, prm, st));
    if (A->dtype == HIPK_F64)
        return hipk_cg_solve_t<double>(A, (const double *)b, (double *)x, (char *)work, prm, st, (hipStream_t)stream);
    return hipk_cg_solve_t<float>(A, (const float *)b, (float *)x, (char *)work, prm, st, (hipStream_t)stream);
}

extern "C" int hipk_pcg_solve(hipk_csr_t A, const void *dinv, const void *b, void *x, void *work, size_t work_bytes,
                              const hipk_params *prm, hipk_stats *st, hipk_stream_t stream) {
    HIPK_TRY(hipk_solve_check(A, dinv != nullptr, dinv, b, x, work, work_bytes, hipk_pcg_work_bytes, prm, st));
    if (A->dtype == HIPK_F64)
        return hipk_pcg_solve_t<double>(A, (const double *)dinv, (const double *)b, (double *)x, (char *)work, prm, st, (hipStream_t)stream);
    return hipk_pcg_solve_t<float>(A, (const float *)dinv, (const float *)b, (float *)x, (char *)work, prm, st, (hipStream_t)stream);
}

// =====================================================================================================================
// Row-partitioned CG with the Jacobi preconditioner, the loop of one rank in C: the launch sequence of hipk_pcg_solve on the row
// block, with the conventions of hipk_dist_cg_solve (csrc/hipk_dist.hip: fixed batches, the stop word read one batch late, the
// same collectives on every rank).  Every kernel folds the gathered partials of ALL ranks in global chunk order, so the iterates
// are bitwise those of hipk_pcg_solve on the whole system.  Per iteration, on the solver's stream:
//   SpMV p -> Ap, <p,Ap> | all-gather <p,Ap> | update (r, <r,r>, <r,z>) | ONE group: all-gather <r,r> + all-gather <r,z> + the
//   halo of r | direction over n_ext (x, p = z + beta p, stop test)
// -- two collective launches, as plain CG.  The direction kernel forms z = dinv .* r on the ghost rows as well, from the exchanged
// r and the caller's dinv tail: the owner's operands, the owner's bits.  <r,z> lives in a ping-pong pair of gathered arrays by
// iteration parity: the update kernel reads the old one while the direction kernel reads both.
#include "hipk_dist_xchg.h"

struct hipk_dpcg_layout {
    size_t scal, part_loc, part_rz, spare, g_pAp, g_rr, g_bb, g_xx, g_rz0, g_rz1, send_buf, slab_loc, slab_all, p, r, Ap, total;
};
static hipk_dpcg_layout hipk_dpcg_make_layout(const hipk_dist_plan *pl) {
    hipk_dpcg_layout L;
    hipk_carve take;
    const size_t per = (size_t)pl->per, W = (size_t)pl->world;
    const size_t next = (size_t)(pl->n_ext > 0 ? pl->n_ext : 1), nloc = (size_t)(pl->n_local > 0 ? pl->n_local : 1);
    L.scal = take(256);
    L.part_loc = take(per * 8);
    L.part_rz = take(per * 8);
    L.spare = take(per * 8);
    L.g_pAp = take(W * per * 8);
    L.g_rr = take(W * per * 8);
    L.g_bb = take(W * per * 8);
    L.g_xx = take(W * per * 8);
    L.g_rz0 = take(W * per * 8);
    L.g_rz1 = take(W * per * 8);
    L.send_buf = take((size_t)(pl->n_send > 0 ? pl->n_send : 1) * 8);
    L.slab_loc = take((size_t)(pl->slab > 0 ? pl->slab : 1) * 8);
    L.slab_all = take((size_t)(pl->slab > 0 ? pl->slab : 1) * W * 8);
    L.p = take(next * 8);
    L.r = take(next * 8);
    L.Ap = take(nloc * 8);
    L.total = take.o;
    return L;
}

extern "C" size_t hipk_dist_pcg_work_bytes(const hipk_dist_plan *plan) {
    if (!plan || plan->world < 1 || plan->per < 1) return 0;
    return hipk_dpcg_make_layout(plan).total;
}

extern "C" int hipk_dist_pcg_solve(hipk_csr_t A, const hipk_dist_plan *pl, const hipk_rccl *cc, const void *dinv_ext,
                                   const void *b_local, void *x_ext, void *work, size_t work_bytes, const hipk_params *prm,
                                   hipk_stats *st, hipk_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    HIPK_TRY(hipk_dist_check(A, pl, cc, true, dinv_ext, b_local, x_ext, work, prm, st));
    const hipk_dpcg_layout L = hipk_dpcg_make_layout(pl);
    HIPK_REQUIRE(work_bytes >= L.total, HIPK_ERR_WORKSPACE, "work too small");
    memset(st, 0, sizeof(*st));
    typedef double T;
    char *wk = (char *)work;
    hipk_pcg_scal *scal = (hipk_pcg_scal *)(wk + L.scal);
    double *part_loc = (double *)(wk + L.part_loc), *part_rz = (double *)(wk + L.part_rz), *spare = (double *)(wk + L.spare);
    double *g_pAp = (double *)(wk + L.g_pAp), *g_rr = (double *)(wk + L.g_rr), *g_bb = (double *)(wk + L.g_bb);
    double *g_xx = (double *)(wk + L.g_xx);
    double *g_rz[2] = {(double *)(wk + L.g_rz0), (double *)(wk + L.g_rz1)};
    T *p = (T *)(wk + L.p), *r = (T *)(wk + L.r), *Ap = (T *)(wk + L.Ap);
    T *x = (T *)x_ext;
    const T *b = (const T *)b_local, *dinv = (const T *)dinv_ext;
    const int64_t n = pl->n_local, n_ext = pl->n_ext;
    const int ch = pl->chunk_rows, G = pl->g_red;
    const int grid = (int)((n + ch - 1) / ch), grid_ext = (int)((n_ext + ch - 1) / ch);
    const int64_t maxiter = hipk_default_maxiter(prm, pl->n_global);
    const hipk_tol_sq tol(prm);
    const int64_t *stop_dev = &scal->stop_it;
    const hipk_dist_xchg xc(pl, cc, stream, (double *)(wk + L.send_buf), (double *)(wk + L.slab_loc), (double *)(wk + L.slab_all),
                            "hipk_dist_pcg_solve");

    hipk_event_pair whole;
    HIPK_CHECK_HIP(whole.create());
    HIPK_CHECK_HIP(hipEventRecord(whole.a, stream));
    HIPK_CHECK_HIP(hipMemsetAsync(wk, 0, L.total, stream));
    if (n_ext > n) HIPK_CHECK_HIP(hipMemsetAsync(x + n, 0, (size_t)(n_ext - n) * 8, stream));

    // ---- r0 = b - A x0, <r0,r0>; <b,b>; z0 = M r0, p0 = z0, gamma0 = <r0,z0> (TSL:815-826); the halo of p0 from its owners
    HIPK_TRY(xc.run(x));
    HIPK_TRY(hipk_dist_spmv(A, x, r, HIPK_SPMV_RESID | HIPK_SPMV_DOT_YY, nullptr, b, nullptr, spare, part_loc, nullptr, 0, stream));
    HIPK_TRY(xc.parts(part_loc, g_rr));
    HIPK_TRY(hipk_dot_parts(n, ch, b, b, HIPK_F64, part_loc, stream));
    HIPK_TRY(xc.parts(part_loc, g_bb));
    hipk_pcg_start_kernel<T><<<grid, HIPK_THREADS, 0, stream>>>(n, ch, G, scal, g_rr, g_bb, r, dinv, p, part_rz, tol.tol2, tol.atol_sq,
                                                                 maxiter, nullptr);
    HIPK_CHECK_HIP(hipGetLastError());
    HIPK_TRY(xc.run(p, part_rz, g_rz[0]));

    // ---- the loop: fixed batches, the stop word read one batch late (hipk_dist_batches)
    int64_t it = 0, stop = INT64_MAX;
    HIPK_TRY(hipk_dist_batches(prm, A->host_poll, stop_dev, maxiter, stream, it, stop, [&](int64_t it) -> int {
        double *rz_old = g_rz[it & 1], *rz_new = g_rz[(it + 1) & 1];
        HIPK_TRY(hipk_dist_spmv(A, p, Ap, HIPK_SPMV_DOT_W, p, nullptr, nullptr, part_loc, spare, stop_dev, it, stream));
        HIPK_TRY(xc.parts(part_loc, g_pAp));
        hipk_pcg_update_kernel<T><<<grid, HIPK_THREADS, 0, stream>>>(n, ch, G, scal, it, g_pAp, rz_old, Ap, dinv, r, part_loc, part_rz);
        HIPK_TRY(xc.run(r, part_loc, g_rr, part_rz, rz_new));
        hipk_pcg_direction_kernel<T><<<grid_ext, HIPK_THREADS, 0, stream>>>(n_ext, ch, G, scal, it, maxiter, g_pAp, rz_old, rz_new,
                                                                             g_rr, r, dinv, p, x);
        return HIPK_OK;
    }));

    // ---- TSL:1007-1014 with M: ||M (b - A x)||, ||x||
    HIPK_TRY(xc.run(x));
    HIPK_TRY(hipk_dist_spmv(A, x, Ap, HIPK_SPMV_RESID, nullptr, b, nullptr, spare, spare, nullptr, 0, stream));
    hipk_pcg_resnorm_kernel<T><<<grid, HIPK_THREADS, 0, stream>>>(n, ch, Ap, dinv, part_loc);
    HIPK_CHECK_HIP(hipGetLastError());
    HIPK_TRY(xc.parts(part_loc, g_rr));
    HIPK_TRY(hipk_dot_parts(n, ch, x, x, HIPK_F64, part_loc, stream));
    HIPK_TRY(xc.parts(part_loc, g_xx));
    hipk_pcg_final_kernel<<<1, HIPK_THREADS, 0, stream>>>(scal, G, g_rr, g_xx);
    HIPK_CHECK_HIP(hipGetLastError());
    hipk_pcg_scal hs;
    HIPK_CHECK_HIP(hipEventRecord(whole.b, stream));
    HIPK_CHECK_HIP(hipMemcpyAsync(&hs, scal, sizeof(hs), hipMemcpyDeviceToHost, stream));
    HIPK_CHECK_HIP(hipStreamSynchronize(stream));
    const int64_t iterations = (hs.stop_it < it) ? hs.stop_it : it;
    hipk_finish_isolve_stats(st, prm, hs.bs, hs.res2, hs.xx, iterations, iterations + 2);
    st->recurrence_rs = hs.rs_last;
    float ms = 0.f;
    HIPK_CHECK_HIP(hipEventElapsedTime(&ms, whole.a, whole.b));
    st->solve_ms = ms;
    return HIPK_OK;
}

// Row-partitioned CG with the Chebyshev polynomial preconditioner, and that preconditioner's apply on a row block
#include "hipk_dist_cheb.h"

#ifdef HIPK_GM_STAMPS
// diagnostic twin only: per-workgroup phase time sums of the last hipk_cg_mid_kernel launch (hipk_cg_mid.h)
extern "C" int hipk_debug_mid_stamps(unsigned long long *out, size_t count) {
    const size_t have = sizeof(hipk_mid_stamps) / sizeof(unsigned long long);
    HIPK_CHECK_HIP(hipDeviceSynchronize());
    HIPK_CHECK_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(hipk_mid_stamps), sizeof(unsigned long long) * (count < have ? count : have)));
    return HIPK_OK;
}
#endif
