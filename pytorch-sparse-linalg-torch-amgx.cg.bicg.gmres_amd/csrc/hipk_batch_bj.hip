// hipk_batch_bj.hip -- cg_batch / bicgstab_batch with M = blockdiag(binv): the block-Jacobi forms of the one-workgroup-per-system
// kernels of hipk_batch.hip (whose rules hold here word for word: no workgroup reads what another writes, thread 0 alone forms
// scalars and decisions and publishes them through the LDS scalar block, every barrier is reached by all 256 threads or by none,
// bounded launches resume from the state of an iteration about to start).
//
// hipk_cg_bjbatch_kernel<T> is orc_pcg_blockjacobi per system, hipk_bi_bjbatch_kernel<T> the single solve's callback form
// (bicgstab_impl with phat = M p, shat = M s from the block apply and the final test the plain <z,z>, z = M (b - A x)).
//
// The apply.  z_i needs the bs elements of its block, which other threads own (a block straddles owners, 256-row tiles and the
// 2048-element chunk), so the input vector is complete in LDS behind a barrier before any thread forms a z_i (hipk_bbj_row); every
// thread forms z for the elements it owns.  block_size is a run-time value and the loop over a block's columns a run-time loop:
// no per-thread array is indexed with it, the kernels have no scratch.  binv streams from memory on every apply (n bs elements).
#include "hipk_batch.h"

static inline size_t hipk_bjbatch_lds_bytes(int n, size_t sv, int solver) {
    const size_t nvp = ((size_t)n + 3) & ~(size_t)3;
    return HIPK_BATCH_LDS_FIXED + (size_t)(solver == 0 ? 2 : 3) * nvp * sv;
}
static inline int hipk_bjbatch_nvec(int solver) { return solver == 0 ? 3 : 5; }

extern "C" size_t hipk_bj_batch_work_bytes(int64_t n, int64_t nnz, int batch, int dtype, int solver, int block_size) {
    (void)nnz;
    (void)block_size;
    const size_t sv = (dtype == HIPK_F64) ? 8 : 4;
    const size_t vec = hipk_align_up((size_t)(n > 0 ? n : 1) * sv, 256);
    const size_t s = (size_t)(batch > 0 ? batch : 1);
    return HIPK_BATCH_HEAD + s * HIPK_BATCH_REC + s * (size_t)hipk_bjbatch_nvec(solver ? 1 : 0) * vec;
}

// ---------------------------------------------------------------------------------------------------------------- block-Jacobi PCG
// orc_pcg_blockjacobi.  Slab: r | z (own-element layout, read back by the thread that wrote it) | p (saved between launches only).
// LDS vectors: p (x while a residual is formed) | Ap, then the new r: the input of the apply.
template <typename T>
__global__ __launch_bounds__(HIPK_THREADS) HIPK_SGPR80 void hipk_cg_bjbatch_kernel(hipk_bjbatch_args ba) {
    constexpr int VEC = hipk_vec<T>::VEC;
    extern __shared__ __align__(16) unsigned char hipk_batch_raw[];
    const hipk_batch_args &a = ba.a;
    const hipk_batch_lds l = hipk_batch_carve(hipk_batch_raw);
    const int t = threadIdx.x, n = a.n, g = a.g, bs = ba.bs;
    const size_t s = blockIdx.x;
    hipk_batch_rec *rec = (hipk_batch_rec *)(a.recs + s * HIPK_BATCH_REC);
    T *pl = (T *)l.vec, *yl = pl + a.nvp;
    T *r = (T *)(a.slabs + s * a.slab_bytes), *z = (T *)((char *)r + a.vec_bytes), *psave = (T *)((char *)r + 2 * a.vec_bytes);
    const T *vals = (const T *)a.vals + s * a.ldv, *b = (const T *)a.B + s * a.ldb;
    const T *binv = (const T *)ba.binv + s * ba.ldbinv;
    T *x = (T *)a.X + s * a.ldx;
    double *sd = l.sd;
    int64_t *si = l.si;

    if (!hipk_batch_enter(a, rec, l)) return;

    // thread 0: the loop condition of orc_pcg_blockjacobi at the top of iteration k, and this launch's budget
    auto decide = [&]() {
        const bool stop = si[BI_K] >= a.maxiter || sd[BS_RS] <= sd[BS_ATOL2];
        si[BI_GO] = stop ? GO_FINISH : (si[BI_ITS] >= a.budget ? GO_SAVE : GO_ITERATE);
    };

    if (!a.resume) {
        // <b,b> (plain) while x0 moves to LDS; r0 = b - A x0 with the tiled <r0,r0>, r0 to the slab and to LDS
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
            yl[row] = rv;
            pr[0] = (double)rv * (double)rv;
        });
        __syncthreads();
        if (t == 0) {
            const double bb = sd[BS_BS];
            const double a2 = a.tol2 * bb;
            sd[BS_ATOL2] = a2 > a.atol_sq ? a2 : a.atol_sq;
            sd[BS_RS] = hipk_btiled_t0(l.sw, a.ntile, g);
            si[BI_MATVECS] = 1;
        }
        // z0 = M r0, p = z0, gamma = <r0, z0> plain
        double az[2] = {0.0, 0.0};
        HIPK_B_FOR_OWN(T, c, base) {
            T rv[VEC], zv[VEC];
            hipk_bld(yl, base, n, rv);
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                zv[e] = (T)0;
                if (base + e < n) {
                    zv[e] = hipk_bbj_row(binv, yl, base + e, n, bs);
                    az[c] = fma((double)rv[e], (double)zv[e], az[c]);
                }
            }
            hipk_bst(pl, base, n, zv);
        }
        hipk_bsums_t0<2>(az, l.red + 512);
        if (t == 0) {
            sd[BS_GAMMA] = hipk_bfold2(az[0], az[1], g);
            decide();
        }
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
        // x += alpha p, r -= alpha Ap, <r,r> plain; the new r replaces the thread's own elements of Ap in LDS
        const T alpha = (T)sd[BS_ALPHA];
        double acc[2] = {0.0, 0.0};
        HIPK_B_FOR_OWN(T, c, base) {
            T rv[VEC], xv[VEC], pv[VEC], yv[VEC];
            hipk_bld(r, base, n, rv);
            hipk_bld(x, base, n, xv);
            hipk_bld(pl, base, n, pv);
            hipk_bld(yl, base, n, yv);
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const T m0 = alpha * pv[e];
                xv[e] = xv[e] + m0;
                const T m1 = alpha * yv[e];
                rv[e] = rv[e] - m1;
                if (base + e < n) acc[c] = fma((double)rv[e], (double)rv[e], acc[c]);
            }
            hipk_bst(r, base, n, rv);
            hipk_bst(x, base, n, xv);
            hipk_bst(yl, base, n, rv);
        }
        hipk_bsums_t0<2>(acc, l.red);   // (its barrier also completes r in LDS)
        // z = M r, stored; <r,z> plain
        double az[2] = {0.0, 0.0};
        HIPK_B_FOR_OWN(T, c, base) {
            T rv[VEC], zv[VEC];
            hipk_bld(yl, base, n, rv);
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                zv[e] = (T)0;
                if (base + e < n) {
                    zv[e] = hipk_bbj_row(binv, yl, base + e, n, bs);
                    az[c] = fma((double)rv[e], (double)zv[e], az[c]);
                }
            }
            hipk_bst(z, base, n, zv);
        }
        hipk_bsums_t0<2>(az, l.red + 512);   // the second half of red: wavefront 0 may still be reading the first
        if (t == 0) {
            const double rr = hipk_bfold2(acc[0], acc[1], g);
            const double rz = hipk_bfold2(az[0], az[1], g);
            sd[BS_BETA] = rz / sd[BS_GAMMA];
            sd[BS_GAMMA] = rz;
            sd[BS_RS] = rr;
            si[BI_K] += 1;
            si[BI_ITS] += 1;
            decide();
        }
        __syncthreads();
        // p = z + beta p (z: what this thread stored above)
        const T beta = (T)sd[BS_BETA];
        HIPK_B_FOR_OWN(T, c, base) {
            T zv[VEC], pv[VEC];
            hipk_bld(z, base, n, zv);
            hipk_bld(pl, base, n, pv);
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const T m = beta * pv[e];
                pv[e] = zv[e] + m;
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

    // TSL:1007-1016: t = b - A x, z = M t, the plain <z,z>; <x,x> plain
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
    hipk_bspmv<T, 0>(a, vals, pl, l.sw, [&](int row, T sum, double(&)[1]) { yl[row] = b[row] - sum; });
    __syncthreads();
    HIPK_B_FOR_OWN(T, c, base) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            if (base + e < n) {
                const T m = hipk_bbj_row(binv, yl, base + e, n, bs);
                ax[2 + c] = fma((double)m, (double)m, ax[2 + c]);
            }
        }
    }
    hipk_bsums_t0<4>(ax, l.red);
    if (t == 0) {
        sd[BS_XX] = hipk_bfold2(ax[0], ax[1], g);
        sd[BS_RES2] = hipk_bfold2(ax[2], ax[3], g);
        si[BI_MATVECS] += 1;
        hipk_bfinish(rec, a, sd, si);
    }
}

// ---------------------------------------------------------------------------------------------------------------- block-Jacobi BiCGStab
// bicgstab_impl with phat = M p, shat = M s.  Slab: r | rhat | q | p | s (the layout of hipk_bi_batch_kernel<T, true>).
// LDS vectors: ga = phat (x while a residual is formed) | gb = shat | yl = q, then t; between them the input of an apply (p, then s:
// t is dead at the direction step, and a thread replaces its own elements of q by s).
template <typename T>
__global__ __launch_bounds__(HIPK_THREADS) HIPK_SGPR80 void hipk_bi_bjbatch_kernel(hipk_bjbatch_args ba) {
    constexpr int VEC = hipk_vec<T>::VEC;
    constexpr double EPS = hipk_beps<T>::v;
    extern __shared__ __align__(16) unsigned char hipk_batch_raw[];
    const hipk_batch_args &a = ba.a;
    const hipk_batch_lds l = hipk_batch_carve(hipk_batch_raw);
    const int t = threadIdx.x, n = a.n, g = a.g, bs = ba.bs;
    const size_t s = blockIdx.x;
    hipk_batch_rec *rec = (hipk_batch_rec *)(a.recs + s * HIPK_BATCH_REC);
    T *ga = (T *)l.vec, *gb = ga + a.nvp, *yl = gb + a.nvp;
    char *slab = a.slabs + s * a.slab_bytes;
    T *r = (T *)slab, *rhat = (T *)(slab + a.vec_bytes), *q = (T *)(slab + 2 * a.vec_bytes), *pg = (T *)(slab + 3 * a.vec_bytes);
    T *sg = (T *)(slab + 4 * a.vec_bytes);
    const T *vals = (const T *)a.vals + s * a.ldv, *b = (const T *)a.B + s * a.ldb;
    const T *binv = (const T *)ba.binv + s * ba.ldbinv;
    T *x = (T *)a.X + s * a.ldx;
    double *sd = l.sd;
    int64_t *si = l.si;

    if (!hipk_batch_enter(a, rec, l)) return;

    // thread 0: the top of the oracle's loop (TSL:895-906) for iteration k, and this launch's budget (as hipk_bi_batch_kernel)
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
            const double bb = sd[BS_BS];
            const double a2 = a.tol2 * bb;
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
            hipk_bst(pg, base, n, rv);
        }
        __syncthreads();
    } else {
        if (t == 0) decide();
        __syncthreads();
    }

    while (si[BI_GO] == GO_ITERATE) {
        // p = r + beta (p - omega q), to the slab and to LDS (yl: t is dead)
        {
            const T beta = (T)sd[BS_BETA], omega = (T)sd[BS_OMEGA];
            HIPK_B_FOR_OWN(T, c, base) {
                T rv[VEC], pv[VEC], qv[VEC];
                hipk_bld(r, base, n, rv);
                hipk_bld(pg, base, n, pv);
                hipk_bld(q, base, n, qv);
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    const T t1 = omega * qv[e];
                    const T t2 = pv[e] - t1;
                    const T t3 = beta * t2;
                    pv[e] = rv[e] + t3;
                }
                hipk_bst(pg, base, n, pv);
                hipk_bst(yl, base, n, pv);
            }
        }
        __syncthreads();
        // phat = M p
        HIPK_B_FOR_OWN(T, c, base) {
            T hv[VEC];
#pragma unroll
            for (int e = 0; e < VEC; ++e) hv[e] = (base + e < n) ? hipk_bbj_row(binv, yl, base + e, n, bs) : (T)0;
            hipk_bst(ga, base, n, hv);
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
        // s = r - alpha q, to the slab and over the thread's own elements of q in LDS; <s,s> plain; shat = M s
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
                hipk_bst(sg, base, n, rv);
                hipk_bst(yl, base, n, rv);
            }
            hipk_bsums_t0<2>(acc, l.red);   // (its barrier also completes s in LDS)
            if (t == 0) si[BI_EXIT_EARLY] = hipk_bfold2(acc[0], acc[1], g) < sd[BS_ATOL2] ? 1 : 0;
            HIPK_B_FOR_OWN(T, c, base) {
                T hv[VEC];
#pragma unroll
                for (int e = 0; e < VEC; ++e) hv[e] = (base + e < n) ? hipk_bbj_row(binv, yl, base + e, n, bs) : (T)0;
                hipk_bst(gb, base, n, hv);
            }
        }
        __syncthreads();
        // t = A shat, <t,t> and <s,t> tiled
        hipk_bspmv<T, 2>(a, vals, gb, l.sw, [&](int row, T sum, double(&pr)[2]) {
            yl[row] = sum;
            const T sv = sg[row];
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
                hipk_bld(sg, base, n, sv);
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
        if (t == 0) hipk_batch_save(a, rec, l);
        return;
    }

    // TSL:1007-1016: t = b - A x, z = M t, the plain <z,z>; <x,x> plain
    double ax[4] = {0.0, 0.0, 0.0, 0.0};
    HIPK_B_FOR_OWN(T, c, base) {
        T xv[VEC];
        hipk_bld(x, base, n, xv);
#pragma unroll
        for (int e = 0; e < VEC; ++e)
            if (base + e < n) ax[c] = fma((double)xv[e], (double)xv[e], ax[c]);
        hipk_bst(ga, base, n, xv);
    }
    __syncthreads();
    hipk_bspmv<T, 0>(a, vals, ga, l.sw, [&](int row, T sum, double(&)[1]) { yl[row] = b[row] - sum; });
    __syncthreads();
    HIPK_B_FOR_OWN(T, c, base) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            if (base + e < n) {
                const T m = hipk_bbj_row(binv, yl, base + e, n, bs);
                ax[2 + c] = fma((double)m, (double)m, ax[2 + c]);
            }
        }
    }
    hipk_bsums_t0<4>(ax, l.red);
    if (t == 0) {
        sd[BS_XX] = hipk_bfold2(ax[0], ax[1], g);
        sd[BS_RES2] = hipk_bfold2(ax[2], ax[3], g);
        si[BI_MATVECS] += 1;
        hipk_bfinish(rec, a, sd, si);
    }
}

// ---------------------------------------------------------------------------------------------------------------- host
template <typename T>
static int hipk_bjbatch_launch(int solver, const hipk_bjbatch_args &ba, int batch, size_t lds, hipStream_t s) {
    void (*kern)(hipk_bjbatch_args) = solver == 0 ? hipk_cg_bjbatch_kernel<T> : hipk_bi_bjbatch_kernel<T>;
    if (lds > 64 * 1024)   // beyond the default limit of dynamic LDS; per launch: the attribute belongs to the current device
        HIPK_CHECK_HIP(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    kern<<<(unsigned)batch, HIPK_THREADS, lds, s>>>(ba);
    HIPK_CHECK_HIP(hipGetLastError());
    return HIPK_OK;
}

static const char *hipk_bjbatch_name(int solver, int dtype) {
    static const char *names[2][2] = {{"hipk_cg_bjbatch_kernel<float>", "hipk_cg_bjbatch_kernel<double>"},
                                      {"hipk_bi_bjbatch_kernel<float>", "hipk_bi_bjbatch_kernel<double>"}};
    return names[solver][dtype == HIPK_F64];
}

static int hipk_solve_bjbatch(int solver, int dtype, int64_t n, int64_t nnz, const int32_t *crow, const int32_t *col, const void *vals,
                              int64_t ldv, const void *binv, int64_t ldbinv, int block_size, int batch, const void *B, int64_t ldb,
                              void *X, int64_t ldx, void *work, size_t work_bytes, const hipk_params *prm, hipk_stats *st,
                              hipk_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    HIPK_REQUIRE(binv, HIPK_ERR_ARG, "null argument");
    HIPK_REQUIRE(block_size >= 1 && block_size <= 32, HIPK_ERR_UNSUPPORTED, "the block-Jacobi batch kernels take a block_size in [1, 32]");
    HIPK_TRY(hipk_batch_check(dtype, n, nnz, crow, col, vals, ldv, nullptr, 0, batch, B, ldb, X, ldx, work, work_bytes,
                              hipk_bj_batch_work_bytes(n, nnz, batch, dtype, solver, block_size), prm, st, s));
    const size_t sv = dtype == HIPK_F64 ? 8 : 4;
    const int64_t nb = (n + block_size - 1) / block_size;
    HIPK_REQUIRE(ldbinv >= nb * block_size * block_size, HIPK_ERR_ARG, "ldbinv is shorter than the blocks of one system");
    HIPK_REQUIRE(((uintptr_t)binv) % sv == 0, HIPK_ERR_ARG, "binv must be aligned to its element size");
    hipk_bjbatch_args ba;
    memset(&ba, 0, sizeof(ba));
    hipk_batch_fill(ba.a, dtype, n, crow, col, vals, ldv, nullptr, 0, batch, B, ldb, X, ldx, work, hipk_bjbatch_nvec(solver), prm);
    ba.binv = binv;
    ba.ldbinv = ldbinv;
    ba.bs = block_size;
    const size_t lds = hipk_bjbatch_lds_bytes((int)n, sv, solver);
    hipk_set_solve_path(nullptr, hipk_bjbatch_name(solver, dtype));
    return hipk_batch_drive(ba.a, batch, st, s, [&]() {
        return dtype == HIPK_F64 ? hipk_bjbatch_launch<double>(solver, ba, batch, lds, s) : hipk_bjbatch_launch<float>(solver, ba, batch, lds, s);
    });
}

extern "C" int hipk_cg_solve_batch_bj(int64_t n, int64_t nnz, const int32_t *crow_dev, const int32_t *col_dev, const void *vals,
                                      int64_t ldv, const void *binv, int64_t ldbinv, int block_size, int batch, const void *B,
                                      int64_t ldb, void *X, int64_t ldx, int dtype, void *work, size_t work_bytes,
                                      const hipk_params *prm, hipk_stats *st, hipk_stream_t stream) {
    return hipk_solve_bjbatch(0, dtype, n, nnz, crow_dev, col_dev, vals, ldv, binv, ldbinv, block_size, batch, B, ldb, X, ldx, work,
                              work_bytes, prm, st, stream);
}

extern "C" int hipk_bicgstab_solve_batch_bj(int64_t n, int64_t nnz, const int32_t *crow_dev, const int32_t *col_dev, const void *vals,
                                            int64_t ldv, const void *binv, int64_t ldbinv, int block_size, int batch, const void *B,
                                            int64_t ldb, void *X, int64_t ldx, int dtype, void *work, size_t work_bytes,
                                            const hipk_params *prm, hipk_stats *st, hipk_stream_t stream) {
    return hipk_solve_bjbatch(1, dtype, n, nnz, crow_dev, col_dev, vals, ldv, binv, ldbinv, block_size, batch, B, ldb, X, ldx, work,
                              work_bytes, prm, st, stream);
}
