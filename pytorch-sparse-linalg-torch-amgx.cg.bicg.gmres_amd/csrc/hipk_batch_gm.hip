// hipk_batch_gm.hip -- gmres_batch: restarted GMRES for S independent small systems with ONE sparsity pattern, one workgroup per system.
//
// hipk_gm_batch_kernel<T, PRE> runs the whole restarted solve of system s = blockIdx.x in one 256-thread workgroup: <b,b> and the
// tolerances, the initial residual, the restart cycles (Arnoldi steps with classical Gram-Schmidt of at most two passes, the small
// least-squares solve, x += V y, the residual), the final true residual and info.  The rules of hipk_batch.hip hold: no workgroup
// reads what another writes (the one exception is the atomic count of unfinished systems that only the host reads), and thread 0
// alone forms every scalar and takes every decision -- the second Gram-Schmidt pass, the `_safe_normalize` thresholds, breakdown,
// the `err > ptol` test of the incremental form, the loop test, the launch budget -- and publishes them through the LDS scalar
// block, so every barrier is reached by all 256 threads or by none.  The arithmetic is gmres_impl of oracle/krylov_oracle.c with
// gpu_tolerances = 1 per system, bit for bit (DESIGN.md 7c says which dot is which).
//
// Envelope: that of the batch kernels (1 <= n <= 4096, rows of at most 32 stored entries) and 1 <= restart <= 31.
//
// Layout.  Dynamic LDS: the batch kernels' reduction buffers and scalar block, the small dense arrays of a cycle (hipk_gmb_off:
// H or R, the Givens pairs, beta_vec, the packed normal-equation triangle, y; about 14 KB) and two vectors: the gather operand of
// the SpMV (v_k, or x while a residual is formed) and its output w.  w / ||w|| is written to basis column k + 1 and stays in LDS
// as the next gather operand (the two vectors swap roles; nothing is copied back in).  The basis (restart + 1 columns) lives in
// the system's slab of `work`, read and written in the virtual-thread layout of the plain dot with 16-byte accesses -- the thread
// that writes an element of a column is the thread that reads it; x lives in the caller's X.
//
// Bounded launches.  A launch ends a system's work at the first cycle boundary at or after `budget` Arnoldi steps of this launch
// (HIPK_BATCH_LAUNCH_ITS), so it runs at least one cycle.  What it leaves is a cycle about to start: x in X, the unit residual in
// basis column 0, res_norm, cycles, matvecs and happy in the record.  The bits do not depend on the budget.
#include "hipk_batch.h"

#define HIPK_GMB_MAXM 31   // = HIPK_GM_MAXM of hipk_gmres.hip: the restart bound of the LDS-resident small dense arrays
#define HIPK_GMB_LDH 32
#define HIPK_GMB_INV_SQRT2 0.7071067811865476   // TSL:63

// slots of the batch kernels' scalar block as this kernel uses them (doubles; the first GS_SAVED are a cycle boundary's state) ...
enum {
    GS_BS, GS_MB2, GS_ATOL_EFF, GS_PTOL, GS_RES_NORM, GS_SAVED,
    GS_SCALE = GS_SAVED, GS_NORM0, GS_QNORM, GS_QQ, GS_ERR, GS_BETA0, GS_RES2, GS_XX, GS_ND
};
static_assert(GS_ND <= BS_ND, "the scalar block of the record");
// ... and its words: cycles = BI_K, BI_MATVECS, happy = BI_CODE, BI_ITS (Arnoldi steps of this launch), BI_GO, and
enum { GI_FLAGS = BI_EXIT_EARLY, GI_FAIL = BI_NI };   // what thread 0 decided for the step; the Cholesky met a non-positive pivot
static_assert(GI_FAIL < 8, "the LDS scalar block has 8 words");
enum { GF_USE = 1, GF_PASS2 = 2, GF_CONT = 4 };

// the small dense arrays of a cycle, in doubles after the batch kernels' fixed LDS block
struct hipk_gmb_off {
    static constexpr int hs = 0;                                       // [32] h of the pass; diagonal of the Cholesky factor
    static constexpr int rv = hs + HIPK_GMB_LDH;                       // [32] rvec
    static constexpr int hc = rv + HIPK_GMB_LDH;                       // [34] the column the Givens rotations are applied to
    static constexpr int gv = hc + HIPK_GMB_LDH + 2;                   // [64] Givens pairs of the cycle
    static constexpr int bv = gv + 2 * HIPK_GMB_LDH;                   // [34] beta_vec
    static constexpr int hr = bv + HIPK_GMB_LDH + 2;                   // [33][32] H ('batched') or R ('incremental')
    static constexpr int lp = hr + (HIPK_GMB_LDH + 1) * HIPK_GMB_LDH;  // [528] packed lower triangle of H^T H, then of its factor
    static constexpr int yl = lp + HIPK_GMB_LDH * (HIPK_GMB_LDH + 1) / 2;   // [32] y
    static constexpr int zl = yl + HIPK_GMB_LDH;                       // [32] b2, then z
    static constexpr int total = zl + HIPK_GMB_LDH;
};
static_assert(hipk_gmb_off::total % 2 == 0, "the LDS vectors start 16-byte aligned");
static_assert(HIPK_GMB_MAXM * (HIPK_GMB_MAXM + 1) <= 4 * 256, "the elimination fallback's k x (k + 1) scratch fits the reduction buffers");

struct hipk_gm_batch_args {
    hipk_batch_args b;
    int m, incremental;
    double adaptive, atol_floor;   // atol_eff = max(adaptive * ||b||, atol_floor), TSL:735-748
};

static inline size_t hipk_gm_batch_lds_bytes(int n, size_t sv) {
    const size_t nvp = ((size_t)n + 3) & ~(size_t)3;
    return HIPK_BATCH_LDS_FIXED + (size_t)hipk_gmb_off::total * sizeof(double) + 2 * nvp * sv;
}

extern "C" size_t hipk_gmres_batch_work_bytes(int64_t n, int64_t nnz, int batch, int dtype, int restart, int precond) {
    (void)nnz;
    (void)precond;
    if (restart < 1 || restart > HIPK_GMB_MAXM) return 0;
    const size_t sv = (dtype == HIPK_F64) ? 8 : 4;
    const size_t vec = hipk_align_up((size_t)(n > 0 ? n : 1) * sv, 256);
    const size_t s = (size_t)(batch > 0 ? batch : 1);
    return HIPK_BATCH_HEAD + s * HIPK_BATCH_REC + s * (size_t)(restart + 1) * vec;
}

__device__ __forceinline__ double hipk_gmb_tmax(double a, double b) { return (a != a || b != b) ? __builtin_nan("") : (a > b ? a : b); }
__device__ __forceinline__ double hipk_gmb_tmin(double a, double b) { return (a != a || b != b) ? __builtin_nan("") : (a < b ? a : b); }
__device__ __forceinline__ double hipk_gmb_norm(double sq) { return sqrt(sq < 0.0 ? 0.0 : sq); }

template <typename T, bool PRE>
__global__ __launch_bounds__(HIPK_THREADS) HIPK_SGPR80 void hipk_gm_batch_kernel(hipk_gm_batch_args p) {
    using O = hipk_gmb_off;
    constexpr int VEC = hipk_vec<T>::VEC;
    constexpr double EPS = hipk_beps<T>::v;
    constexpr int LDH = HIPK_GMB_LDH;
    extern __shared__ __align__(16) unsigned char hipk_batch_raw[];
    const hipk_batch_args &a = p.b;
    const hipk_batch_lds l = hipk_batch_carve(hipk_batch_raw);
    const int t = threadIdx.x, n = a.n, g = a.g, m = p.m;
    const bool incremental = p.incremental != 0;
    const size_t s = blockIdx.x;
    hipk_batch_rec *rec = (hipk_batch_rec *)(a.recs + s * HIPK_BATCH_REC);
    double *sm = (double *)l.vec;
    double *hs = sm + O::hs, *rvec = sm + O::rv, *hc = sm + O::hc, *gv = sm + O::gv, *bv = sm + O::bv, *HR = sm + O::hr;
    double *Lp = sm + O::lp, *yl = sm + O::yl, *zl = sm + O::zl;
    T *ga = (T *)(sm + O::total), *wl = ga + a.nvp;   // the SpMV's gather operand and its output; they swap
    char *slab = a.slabs + s * a.slab_bytes;
    const T *vals = (const T *)a.vals + s * a.ldv, *b = (const T *)a.B + s * a.ldb;
    const T *dinv = PRE ? (const T *)a.dinv + s * a.ldd : nullptr;
    T *x = (T *)a.X + s * a.ldx;
    double *sd = l.sd;
    int64_t *si = l.si;

    if (!hipk_batch_enter(a, rec, l)) return;

    bool first = !a.resume, final = false, skip = a.resume != 0;
    if (!a.resume) {
        // <b,b> (PRE: and ||M b||^2, the scaled dot) plain while x0 moves to LDS
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        HIPK_B_FOR_OWN(T, c, base) {
            T bb[VEC], xv[VEC], dv[VEC];
            hipk_bld(b, base, n, bb);
            hipk_bld(x, base, n, xv);
            if (PRE) hipk_bld(dinv, base, n, dv);
#pragma unroll
            for (int e = 0; e < VEC; ++e)
                if (base + e < n) {
                    acc[c] = fma((double)bb[e], (double)bb[e], acc[c]);
                    if (PRE) {
                        const T mb = dv[e] * bb[e];
                        acc[2 + c] = fma((double)mb, (double)mb, acc[2 + c]);
                    }
                }
            hipk_bst(ga, base, n, xv);
        }
        hipk_bsums_t0<4>(acc, l.red);   // (its barrier also completes x in LDS)
        if (t == 0) {
            // TSL:735-753
            const double bs = hipk_bfold2(acc[0], acc[1], g);
            const double b_norm = hipk_gmb_norm(bs);
            const double atol_eff = hipk_gmb_tmax(p.adaptive * b_norm, p.atol_floor);
            const double mb_norm = PRE ? hipk_gmb_norm(hipk_bfold2(acc[2], acc[3], g)) : b_norm;
            sd[GS_BS] = bs;
            sd[GS_ATOL_EFF] = atol_eff;
            sd[GS_PTOL] = mb_norm * hipk_gmb_tmin(1.0, atol_eff / b_norm);
        }
    } else {
        // the unit residual a launch left in basis column 0
        const T *v0 = (const T *)slab;
        HIPK_B_FOR_OWN(T, c, base) {
            T rr[VEC];
            hipk_bld(v0, base, n, rr);
            hipk_bst(ga, base, n, rr);
        }
        if (t == 0) si[BI_GO] = GO_ITERATE;   // it was saved because its loop test said so
        __syncthreads();
    }

    for (;;) {
        if (!skip) {
            // ---- res = (M)(b - A x) with its tiled square, x in `ga` (TSL:791, 766)
            hipk_bspmv<T, 1>(a, vals, ga, l.sw, [&](int row, T sum, double(&pr)[1]) {
                T rr = b[row] - sum;
                if (PRE) rr = dinv[row] * rr;
                wl[row] = rr;
                pr[0] = (double)rr * (double)rr;
            });
            __syncthreads();
            if (t == 0) {
                const double r2 = hipk_btiled_t0(l.sw, a.ntile, g);
                si[BI_MATVECS] += 1;
                if (final) {
                    // TSL:766-773
                    rec->iterations = si[BI_K];
                    rec->matvecs = si[BI_MATVECS];
                    rec->breakdown = (int32_t)si[BI_CODE];
                    rec->b_norm = hipk_gmb_norm(sd[GS_BS]);
                    rec->residual_norm = hipk_gmb_norm(r2);
                    rec->x_norm = hipk_gmb_norm(sd[GS_XX]);
                    rec->threshold = sd[GS_ATOL_EFF] * 10;
                    rec->info = (rec->x_norm != rec->x_norm || rec->residual_norm > rec->threshold) ? -1 : 0;
                    rec->recurrence_rs = sd[GS_RES_NORM];
                    rec->status = BATCH_DONE;
                } else {
                    double res_norm = hipk_gmb_norm(r2);
                    const bool use = res_norm > EPS;
                    sd[GS_SCALE] = res_norm;
                    if (!use) res_norm = 0.0;
                    sd[GS_RES_NORM] = res_norm;
                    if (!first) si[BI_K] += 1;
                    // the loop test of TSL:754, then this launch's budget
                    const bool stop = si[BI_K] >= a.maxiter || !(res_norm > sd[GS_ATOL_EFF]);
                    si[BI_GO] = stop ? GO_FINISH : (si[BI_ITS] >= a.budget ? GO_SAVE : GO_ITERATE);
                    si[GI_FLAGS] = use ? GF_USE : 0;
                }
            }
            if (final) return;
            __syncthreads();
            first = false;
            if (si[BI_GO] != GO_FINISH) {
                // the unit residual: basis column 0, and in LDS the gather operand of step 0
                const bool use = (si[GI_FLAGS] & GF_USE) != 0;
                const T scale = (T)sd[GS_SCALE];
                T *v0 = (T *)slab;
                HIPK_B_FOR_OWN(T, c, base) {
                    T rr[VEC];
                    hipk_bld(wl, base, n, rr);
#pragma unroll
                    for (int e = 0; e < VEC; ++e) rr[e] = use ? rr[e] / scale : (T)0;
                    hipk_bst(wl, base, n, rr);
                    hipk_bst(v0, base, n, rr);
                }
                // no barrier here: the cycle's H clear below ends in one before anything gathers from `ga`
                T *tmp = ga;
                ga = wl;
                wl = tmp;
            }
            if (si[BI_GO] == GO_SAVE) {
                if (t == 0) hipk_batch_save(a, rec, l);
                return;
            }
            if (si[BI_GO] == GO_FINISH) {
                // <x,x> plain while x moves to LDS for the true residual
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
                if (t == 0) sd[GS_XX] = hipk_bfold2(ax[0], ax[1], g);
                __syncthreads();
                final = true;
                continue;
            }
        }
        skip = false;

        // ---- one restart cycle (TSL:557-638): H (or R) cleared, beta_vec = [res_norm, 0, ...]
        for (int i = t; i < (LDH + 1) * LDH; i += HIPK_THREADS) HR[i] = 0.0;
        if (t < LDH + 2) bv[t] = 0.0;
        __syncthreads();
        if (t == 0) {
            const double res_norm = sd[GS_RES_NORM];
            bv[0] = res_norm;
            sd[GS_BETA0] = res_norm;
            sd[GS_ERR] = res_norm;
            si[GI_FLAGS] = (m > 0 && (!incremental || res_norm > sd[GS_PTOL])) ? GF_CONT : 0;
        }
        __syncthreads();
        int k = 0;
        while (si[GI_FLAGS] & GF_CONT) {
            // -- `_kth_arnoldi_iteration` (TSL:331-388): w = (M) A v_k, ||w||^2 tiled
            hipk_bspmv<T, 1>(a, vals, ga, l.sw, [&](int row, T sum, double(&pr)[1]) {
                T wv = sum;
                if (PRE) wv = dinv[row] * wv;
                wl[row] = wv;
                pr[0] = (double)wv * (double)wv;
            });
            __syncthreads();
            if (t == 0) {
                double norm0 = hipk_gmb_norm(hipk_btiled_t0(l.sw, a.ntile, g));
                if (!(norm0 > EPS)) norm0 = 0.0;
                sd[GS_NORM0] = norm0;
                sd[GS_QNORM] = 0.0;
                si[BI_MATVECS] += 1;
                si[BI_ITS] += 1;
            }
            // -- classical Gram-Schmidt, at most two passes (TSL:284-328)
            for (int pass = 0; pass < 2; ++pass) {
                // h_j = <V_j, w>, j = 0 .. k: plain dots, eight columns at a time
                for (int j0 = 0; j0 <= k; j0 += 8) {
                    const int nj = k + 1 - j0 < 8 ? k + 1 - j0 : 8;
                    double acc[2][8];
#pragma unroll
                    for (int c = 0; c < 2; ++c)
#pragma unroll
                        for (int jj = 0; jj < 8; ++jj) acc[c][jj] = 0.0;
                    HIPK_B_FOR_OWN(T, c, base) {
                        T wv[VEC];
                        hipk_bld(wl, base, n, wv);
#pragma unroll
                        for (int jj = 0; jj < 8; ++jj) {
                            if (jj < nj) {
                                T vv[VEC];
                                hipk_bld((const T *)(slab + (size_t)(j0 + jj) * a.vec_bytes), base, n, vv);
#pragma unroll
                                for (int e = 0; e < VEC; ++e)
                                    if (base + e < n) acc[c][jj] = fma((double)vv[e], (double)wv[e], acc[c][jj]);
                            }
                        }
                    }
                    double part0[8];
#pragma unroll
                    for (int jj = 0; jj < 8; ++jj) part0[jj] = 0.0;
#pragma unroll
                    for (int c = 0; c < 2; ++c) {
#pragma unroll
                        for (int q = 0; q < 2; ++q) {
                            if (c < g && 4 * q < nj) {
                                double v4[4] = {acc[c][4 * q], acc[c][4 * q + 1], acc[c][4 * q + 2], acc[c][4 * q + 3]};
                                hipk_bsums_t0<4>(v4, l.red);
                                if (t == 0) {
#pragma unroll
                                    for (int i = 0; i < 4; ++i) {
                                        if (c == 0) part0[4 * q + i] = v4[i];
                                        if (c == g - 1 && 4 * q + i < nj)
                                            hs[j0 + 4 * q + i] = (c == 0) ? hipk_bfold2(v4[i], 0.0, 1) : hipk_bfold2(part0[4 * q + i], v4[i], 2);
                                    }
                                }
                                __syncthreads();
                            }
                        }
                    }
                }
                // w -= sum_j V_j h_j: per element an fp64 fma chain over ascending j, one rounding to T; ||w||^2 plain
                double aq[2] = {0.0, 0.0};
                HIPK_B_FOR_OWN(T, c, base) {
                    T wv[VEC];
                    double sacc[VEC];
                    hipk_bld(wl, base, n, wv);
#pragma unroll
                    for (int e = 0; e < VEC; ++e) sacc[e] = 0.0;
#pragma unroll 4
                    for (int j = 0; j <= k; ++j) {
                        T vv[VEC];
                        hipk_bld((const T *)(slab + (size_t)j * a.vec_bytes), base, n, vv);
                        const double hj = hs[j];
#pragma unroll
                        for (int e = 0; e < VEC; ++e) sacc[e] = fma((double)vv[e], hj, sacc[e]);
                    }
#pragma unroll
                    for (int e = 0; e < VEC; ++e) {
                        wv[e] = (T)((double)wv[e] - sacc[e]);
                        if (base + e < n) aq[c] = fma((double)wv[e], (double)wv[e], aq[c]);
                    }
                    hipk_bst(wl, base, n, wv);
                }
                hipk_bsums_t0<2>(aq, l.red);
                if (t == 0) {
                    const double qq = hipk_bfold2(aq[0], aq[1], g);
                    double qnorm = hipk_gmb_norm(qq);
                    if (!(qnorm > EPS)) qnorm = 0.0;   // `_safe_normalize(q)`, default threshold
                    for (int j = 0; j <= k; ++j) rvec[j] = (pass == 0 ? 0.0 : rvec[j]) + hs[j];
                    bool again = false;
                    if (pass == 0) {
                        // TSL:306-312: a second pass when the correction was not small against what is left
                        double rr = 0.0;
                        for (int j = 0; j <= k; ++j) rr = fma(rvec[j], rvec[j], rr);
                        double rnorm = hipk_gmb_norm(rr);
                        if (!(rnorm > EPS)) rnorm = 0.0;
                        again = rnorm < qnorm * HIPK_GMB_INV_SQRT2;
                    }
                    int flags = again ? GF_PASS2 : 0;
                    if (!again) {
                        // TSL:358-387: v_{k+1} = q / ||q|| unless ||q|| <= eps ||A v_k||; column k of H; breakdown
                        double norm1 = hipk_gmb_norm(qq);
                        const bool use = norm1 > EPS * sd[GS_NORM0];
                        sd[GS_SCALE] = norm1;
                        if (!use) norm1 = 0.0;
                        const bool breakdown = norm1 == 0.0;
                        if (breakdown) si[BI_CODE] = 1;
                        double err = sd[GS_ERR];
                        if (!incremental) {
                            for (int j = 0; j <= k; ++j) HR[j * LDH + k] = rvec[j];
                            HR[(k + 1) * LDH + k] = norm1;
                        } else {
                            // TSL:595-623: the rotations so far on the new column, its own rotation, beta_vec, the error estimate
                            for (int j = 0; j <= k; ++j) hc[j] = rvec[j];
                            hc[k + 1] = norm1;
                            for (int i = 0; i < k; ++i) {
                                const double cs = gv[2 * i], sn = gv[2 * i + 1];
                                const double p0 = cs * hc[i], p1 = sn * hc[i + 1];
                                const double t0 = p0 - p1;
                                const double p2 = sn * hc[i], p3 = cs * hc[i + 1];
                                hc[i + 1] = p2 + p3;
                                hc[i] = t0;
                            }
                            double cs, sn;
                            hipk_givens(hc[k], hc[k + 1], cs, sn);
                            gv[2 * k] = cs;
                            gv[2 * k + 1] = sn;
                            {
                                const double p0 = cs * hc[k], p1 = sn * hc[k + 1];
                                hc[k] = p0 - p1;
                            }
                            hc[k + 1] = 0.0;
                            for (int j = 0; j <= k; ++j) HR[j * LDH + k] = hc[j];
                            const double p0 = cs * bv[k], p1 = sn * bv[k + 1];
                            const double t0 = p0 - p1;
                            const double p2 = sn * bv[k], p3 = cs * bv[k + 1];
                            bv[k + 1] = p2 + p3;
                            bv[k] = t0;
                            err = fabs(bv[k + 1]);
                            sd[GS_ERR] = err;
                        }
                        const bool cont = k + 1 < m && !breakdown && (!incremental || err > sd[GS_PTOL]);
                        flags = (use ? GF_USE : 0) | (cont ? GF_CONT : 0);
                    }
                    si[GI_FLAGS] = flags;
                }
                __syncthreads();
                if (!(si[GI_FLAGS] & GF_PASS2)) break;
            }
            ++k;
            if (si[GI_FLAGS] & GF_CONT) {
                // v_k: basis column k, and in LDS the next gather operand
                const bool use = (si[GI_FLAGS] & GF_USE) != 0;
                const T scale = (T)sd[GS_SCALE];
                T *vk = (T *)(slab + (size_t)k * a.vec_bytes);
                HIPK_B_FOR_OWN(T, c, base) {
                    T wv[VEC];
                    hipk_bld(wl, base, n, wv);
#pragma unroll
                    for (int e = 0; e < VEC; ++e) wv[e] = use ? wv[e] / scale : (T)0;
                    hipk_bst(wl, base, n, wv);
                    hipk_bst(vk, base, n, wv);
                }
                __syncthreads();
                T *tmp = ga;
                ga = wl;
                wl = tmp;
            }
        }

        // ---- y: k steps were taken
        if (k > 0) {
            if (!incremental) {
                // `_lstsq` (TSL:391-428): the lower triangle of H^T H, each entry its own chain over p = 0 .. k; b2 = H[0][:] beta0
                const int nent = k * (k + 1) / 2;
                for (int idx = t; idx < nent; idx += HIPK_THREADS) {
                    int i = (int)((sqrt(8.0 * idx + 1.0) - 1.0) * 0.5);
                    while (i * (i + 1) / 2 > idx) --i;
                    while ((i + 1) * (i + 2) / 2 <= idx) ++i;
                    const int j = idx - i * (i + 1) / 2;
                    double sacc = 0.0;
                    for (int q = 0; q <= k; ++q) sacc = fma(HR[q * LDH + i], HR[q * LDH + j], sacc);
                    Lp[idx] = sacc;
                }
                if (t < k) zl[t] = HR[t] * sd[GS_BETA0];
                if (t == 0) si[GI_FAIL] = 0;
                __syncthreads();
                // Cholesky, one lane per row and one barrier per column j: entry (i, j) is lane i's chain over p < j, as in the
                // oracle; the diagonal of the factor goes to hs (the triangle keeps that of H^T H); the forward substitution
                // rides along: lane j finishes z_j, lanes i > j take the link of z_j at the next column.  Thread 0 forms every
                // pivot as well and alone says whether it is positive.
                const int ri = t * (t + 1) / 2;
                double fs = (t < k) ? zl[t] : 0.0, lprev = 0.0;
                for (int j = 0; j < k; ++j) {
                    const int rj = j * (j + 1) / 2;
                    const bool mine = t >= j && t < k;
                    if (mine || t == 0) {
                        if (mine && j > 0) fs = fma(-lprev, zl[j - 1], fs);
                        double d = Lp[rj + j];
                        for (int q = 0; q < j; ++q) d = fma(-Lp[rj + q], Lp[rj + q], d);
                        if (t == 0 && !(d > 0.0)) si[GI_FAIL] = 1;
                        if (mine) {
                            const double ljj = sqrt(d);
                            double lij = ljj;
                            if (t == j) {
                                hs[j] = ljj;
                                zl[j] = fs / ljj;
                            } else {
                                double sacc = Lp[ri + j];
                                for (int q = 0; q < j; ++q) sacc = fma(-Lp[ri + q], Lp[rj + q], sacc);
                                lij = sacc / ljj;
                                Lp[ri + j] = lij;
                            }
                            lprev = lij;
                        }
                    }
                    __syncthreads();
                    if (si[GI_FAIL]) break;
                }
                if (!si[GI_FAIL]) {
                    if (t == 0) {
                        for (int i = k - 1; i >= 0; --i) {
                            double sacc = zl[i];
                            for (int q = i + 1; q < k; ++q) sacc = fma(-Lp[q * (q + 1) / 2 + i], yl[q], sacc);
                            yl[i] = sacc / hs[i];
                        }
                    }
                } else {
                    // the `torch.linalg.solve` fallback (TSL:421-428): H^T H | b2 again, k x (k + 1) in the idle reduction buffers,
                    // then Gaussian elimination with partial pivoting by one thread
                    double *M = l.red;
                    const int ldm = k + 1;
                    for (int idx = t; idx < k * k; idx += HIPK_THREADS) {
                        const int i = idx / k, j = idx - i * k;
                        double sacc = 0.0;
                        for (int q = 0; q <= k; ++q) sacc = fma(HR[q * LDH + i], HR[q * LDH + j], sacc);
                        M[i * ldm + j] = sacc;
                    }
                    if (t < k) M[t * ldm + k] = HR[t] * sd[GS_BETA0];
                    __syncthreads();
                    if (t == 0) {
                        for (int c = 0; c < k; ++c) {
                            int piv = c;
                            for (int i = c + 1; i < k; ++i)
                                if (fabs(M[i * ldm + c]) > fabs(M[piv * ldm + c])) piv = i;
                            if (piv != c)
                                for (int j = 0; j <= k; ++j) {
                                    const double tmp = M[c * ldm + j];
                                    M[c * ldm + j] = M[piv * ldm + j];
                                    M[piv * ldm + j] = tmp;
                                }
                            for (int i = c + 1; i < k; ++i) {
                                const double f = M[i * ldm + c] / M[c * ldm + c];
                                for (int j = c; j <= k; ++j) M[i * ldm + j] = fma(-f, M[c * ldm + j], M[i * ldm + j]);
                            }
                        }
                        for (int i = k - 1; i >= 0; --i) {
                            double sacc = M[i * ldm + k];
                            for (int q = i + 1; q < k; ++q) sacc = fma(-M[i * ldm + q], yl[q], sacc);
                            yl[i] = sacc / M[i * ldm + i];
                        }
                    }
                }
            } else if (t == 0) {
                // solve_triangular (TSL:630)
                for (int i = k - 1; i >= 0; --i) {
                    double sacc = bv[i];
                    for (int q = i + 1; q < k; ++q) sacc = fma(-HR[i * LDH + q], yl[q], sacc);
                    yl[i] = sacc / HR[i * LDH + i];
                }
            }
            __syncthreads();
        }
        // ---- x += V y: the same chain, one rounding to T; x goes to X and, for the residual, to LDS
        HIPK_B_FOR_OWN(T, c, base) {
            T xv[VEC];
            double sacc[VEC];
            hipk_bld(x, base, n, xv);
            if (k > 0) {
#pragma unroll
                for (int e = 0; e < VEC; ++e) sacc[e] = 0.0;
#pragma unroll 4
                for (int j = 0; j < k; ++j) {
                    T vv[VEC];
                    hipk_bld((const T *)(slab + (size_t)j * a.vec_bytes), base, n, vv);
                    const double yj = yl[j];
#pragma unroll
                    for (int e = 0; e < VEC; ++e) sacc[e] = fma((double)vv[e], yj, sacc[e]);
                }
#pragma unroll
                for (int e = 0; e < VEC; ++e) xv[e] = (T)((double)xv[e] + sacc[e]);
                hipk_bst(x, base, n, xv);
            }
            hipk_bst(ga, base, n, xv);
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------------------- host
template <typename T, bool PRE>
static int hipk_gm_batch_launch(const hipk_gm_batch_args &p, int batch, size_t lds, hipStream_t s) {
    void (*kern)(hipk_gm_batch_args) = hipk_gm_batch_kernel<T, PRE>;
    if (lds > 64 * 1024)   // beyond the default limit of dynamic LDS; per launch: the attribute belongs to the current device
        HIPK_CHECK_HIP(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    kern<<<(unsigned)batch, HIPK_THREADS, lds, s>>>(p);
    HIPK_CHECK_HIP(hipGetLastError());
    return HIPK_OK;
}

extern "C" int hipk_gmres_solve_batch(int64_t n, int64_t nnz, const int32_t *crow_dev, const int32_t *col_dev, const void *vals, int64_t ldv,
                                      const void *dinv, int64_t ldd, int batch, const void *B, int64_t ldb, void *X, int64_t ldx, int dtype,
                                      void *work, size_t work_bytes, const hipk_params *prm, hipk_stats *st, hipk_stream_t stream) {
    static const char *names[2][2] = {{"hipk_gm_batch_kernel<float,false>", "hipk_gm_batch_kernel<float,true>"},
                                      {"hipk_gm_batch_kernel<double,false>", "hipk_gm_batch_kernel<double,true>"}};
    HIPK_REQUIRE(prm, HIPK_ERR_ARG, "null argument");
    HIPK_REQUIRE(prm->restart >= 1 && prm->restart <= HIPK_GMB_MAXM, HIPK_ERR_UNSUPPORTED,
                 "the GMRES batch kernel takes a restart in [1, 31]");
    HIPK_REQUIRE(prm->gmres_method == HIPK_GMRES_BATCHED || prm->gmres_method == HIPK_GMRES_INCREMENTAL, HIPK_ERR_ARG,
                 "gmres_method must be HIPK_GMRES_BATCHED or HIPK_GMRES_INCREMENTAL");
    const bool pre = dinv != nullptr;
    hipStream_t s = (hipStream_t)stream;
    HIPK_TRY(hipk_batch_check(dtype, n, nnz, crow_dev, col_dev, vals, ldv, dinv, ldd, batch, B, ldb, X, ldx, work, work_bytes,
                              hipk_gmres_batch_work_bytes(n, nnz, batch, dtype, prm->restart, pre), prm, st, s));
    hipk_gm_batch_args p;
    memset(&p, 0, sizeof(p));
    hipk_batch_fill(p.b, dtype, n, crow_dev, col_dev, vals, ldv, dinv, ldd, batch, B, ldb, X, ldx, work, prm->restart + 1, prm);
    p.m = prm->restart;
    p.incremental = prm->gmres_method == HIPK_GMRES_INCREMENTAL;
    {
        // TSL:735-748 (python floats become fp32 tensors; python max() keeps a float a float); the floor keeps the fp64 eps.  The two
        // factors of hipk_gm_atol_eff (hipk_gmres.hip), which multiplies by ||b|| on the host; here thread 0 does, with its own ||b||
        const double ng = (double)n;
        const double cand = (prm->gpu_tolerances ? 1e-12 : 1e-14) * sqrt(ng);
        p.adaptive = (cand > prm->tol) ? cand : (double)(float)prm->tol;
        const double base_atol = (double)(float)(HIPK_BATCH_EPS64 * (prm->gpu_tolerances ? 1000 : 100) * ng);
        p.atol_floor = hipk_tmax((double)(float)prm->atol, base_atol);
    }
    const size_t lds = hipk_gm_batch_lds_bytes((int)n, dtype == HIPK_F64 ? 8 : 4);
    hipk_set_solve_path(nullptr, names[dtype == HIPK_F64][pre]);
    return hipk_batch_drive(p.b, batch, st, s, [&]() {
        if (dtype == HIPK_F64) return pre ? hipk_gm_batch_launch<double, true>(p, batch, lds, s) : hipk_gm_batch_launch<double, false>(p, batch, lds, s);
        return pre ? hipk_gm_batch_launch<float, true>(p, batch, lds, s) : hipk_gm_batch_launch<float, false>(p, batch, lds, s);
    });
}
