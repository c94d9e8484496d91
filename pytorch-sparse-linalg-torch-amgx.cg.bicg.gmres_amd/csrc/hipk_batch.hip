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
#include "hipk_batch.h"

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
void hipk_batch_note_launches(int launches) { g_batch_launches = launches; }

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
    const bool pre = dinv != nullptr;
    hipStream_t s = (hipStream_t)stream;
    HIPK_TRY(hipk_batch_check(dtype, n, nnz, crow, col, vals, ldv, dinv, ldd, batch, B, ldb, X, ldx, work, work_bytes,
                              hipk_batch_work_bytes(n, nnz, batch, dtype, solver, pre), prm, st, s));
    hipk_batch_args a;
    hipk_batch_fill(a, dtype, n, crow, col, vals, ldv, dinv, ldd, batch, B, ldb, X, ldx, work, hipk_batch_nvec(solver, pre), prm);
    const size_t lds = hipk_batch_lds_bytes((int)n, dtype == HIPK_F64 ? 8 : 4, solver);
    hipk_set_solve_path(nullptr, hipk_batch_name(solver, dtype, pre));
    return hipk_batch_drive(a, batch, st, s, [&]() {
        if (dtype == HIPK_F64)
            return pre ? hipk_batch_launch<double, true>(solver, a, batch, lds, s) : hipk_batch_launch<double, false>(solver, a, batch, lds, s);
        return pre ? hipk_batch_launch<float, true>(solver, a, batch, lds, s) : hipk_batch_launch<float, false>(solver, a, batch, lds, s);
    });
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
