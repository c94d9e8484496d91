// hipk_multi.hip -- CG and BiCGStab with k right-hand sides per matrix read (hipk_cg_solve_multi, hipk_bicgstab_solve_multi).
//
// Column j of a block solve is bit for bit the single solve of column j (the oracle's order, DESIGN.md "Many right-hand
// sides"): the block kernels run the launch sequence of hipk_cg.hip / hipk_bicgstab.hip once for all KP columns of a block,
// with every scalar (alpha, beta, omega, the stop tests, the breakdown tests) folded per column from that column's chunk partials.
//   block SpMV   y = A x (or b - A x, optionally row-scaled by dinv) for the active columns; per-tile sums of the fused dots
//   combine      per chunk, the tile sums folded into chunk partials (orc_dot_tiled_parts_ch)
//   vector steps one workgroup per reduction chunk, plain chunked dots per column (hipk_common.h reduction spec)
// Each column carries its own stop word; the deciding kernel of an iteration records when all columns have stopped
// (hipk_mblk::all_stop), which the host follows through the pinned signal word (hipk_pacer).
#include <math.h>
#include <stdlib.h>

#include "hipk_multi.h"
#include "hipk_solve.h"
#include "hipk_spmv.h"

#define HIPK_M_EPS64 2.220446049250313e-16
#define HIPK_M_EPS32 1.1920928955078125e-07

enum { HIPK_MS_RESID = 1, HIPK_MS_DOT_YY = 2, HIPK_MS_DOT_W = 4, HIPK_MS_SCALE = 8, HIPK_MS_ALL = 16 };

template <typename T>
struct hipk_meps {
    static constexpr double v = sizeof(T) == 8 ? HIPK_M_EPS64 : HIPK_M_EPS32;
};

static __device__ __forceinline__ unsigned hipk_mall(int k) { return (k >= 32) ? 0xffffffffu : ((1u << k) - 1u); }

// the column mask of iteration `it`, read by thread 0 and broadcast (every thread of the workgroup sees the same bits)
static __device__ __forceinline__ unsigned hipk_mmask(const hipk_mcol *cs, const hipk_mblk *blk, int k, int64_t it, bool all,
                                                      unsigned *s_act) {
    if (threadIdx.x == 0) {
        unsigned m = 0;
        if (all) {
            m = hipk_mall(k);
        } else if (it < blk->all_stop) {
            for (int c = 0; c < k; ++c)
                if (it < cs[c].stop_it) m |= 1u << c;
        }
        *s_act = m;
    }
    __syncthreads();
    return *s_act;
}

// ------------------------------------------------------------------ block SpMV
struct hipk_mspmv_args {
    const int *crow, *col;
    const void *val;
    int64_t n;
    int k, mode;
    const void *x, *bsub, *w, *dinv;  // (n, KP) blocks; dinv: n values (HIPK_MS_SCALE)
    void *y;
    double *tp0, *tp1;  // [tile * KP + c]: tile sums of <y,y> (DOT_YY) and <w,y> (DOT_W)
    hipk_mcol *cs;
    hipk_mblk *blk;
    int64_t it;
};

// One tile of 256 rows per workgroup, a row per thread.  Rows of <= 32 entries: products rounded, added in CSR order; longer rows
// (LONG): 64 strided lane sums per column, folded by the wavefront tree (row_sum, oracle/krylov_oracle.c), by the tile's wavefronts.
template <typename T, int KP, bool LONG>
__global__ __launch_bounds__(HIPK_THREADS) void hipk_mspmv_kernel(hipk_mspmv_args a) {
    __shared__ unsigned s_act;
    __shared__ double s_w[4 * 2 * KP];
    const unsigned act = hipk_mmask(a.cs, a.blk, a.k, a.it, (a.mode & HIPK_MS_ALL) != 0, &s_act);
    if (!act) return;
    const int t = threadIdx.x;
    const int64_t tile = blockIdx.x;
    const int64_t row = tile * HIPK_TILE + t;
    const T *__restrict__ x = (const T *)a.x;
    const T *__restrict__ val = (const T *)a.val;
    T s[KP];
#pragma unroll
    for (int c = 0; c < KP; ++c) s[c] = (T)0;
    int lo = 0, hi = 0;
    if (row < a.n) {
        lo = a.crow[row];
        hi = a.crow[row + 1];
    }
    const bool is_long = LONG && (hi - lo > HIPK_LONG_ROW);
    if (!is_long) {
        for (int j = lo; j < hi; ++j) {
            const T v = val[j];
            T xv[KP];
            hipk_mld<T, KP>(x + (size_t)a.col[j] * KP, act, xv);
#pragma unroll
            for (int c = 0; c < KP; ++c)
                if ((act >> c) & 1u) {
                    const T p = v * xv[c];
                    s[c] = s[c] + p;
                }
        }
    }
    if constexpr (LONG) {
        __shared__ T s_long[HIPK_TILE * KP];
        __shared__ int s_lo[HIPK_TILE], s_hi[HIPK_TILE];
        s_lo[t] = is_long ? lo : 0;
        s_hi[t] = is_long ? hi : 0;
        const int any = __syncthreads_or(is_long ? 1 : 0);
        if (any) {
            const int wv = t >> 6, lane = t & 63;
            for (int rr = wv; rr < HIPK_TILE; rr += 4) {
                const int l0 = s_lo[rr], h0 = s_hi[rr];
                if (h0 == 0) continue;  // wave-uniform
                T u[KP];
#pragma unroll
                for (int c = 0; c < KP; ++c) u[c] = (T)0;
                for (int j = l0 + lane; j < h0; j += 64) {
                    const T v = val[j];
                    T xv[KP];
                    hipk_mld<T, KP>(x + (size_t)a.col[j] * KP, act, xv);
#pragma unroll
                    for (int c = 0; c < KP; ++c)
                        if ((act >> c) & 1u) {
                            const T p = v * xv[c];
                            u[c] = u[c] + p;
                        }
                }
#pragma unroll
                for (int c = 0; c < KP; ++c)
                    if ((act >> c) & 1u) {
                        const T r = hipk_wave_sum(u[c]);
                        if (lane == 0) s_long[rr * KP + c] = r;
                    }
            }
            __syncthreads();
            if (is_long) {
#pragma unroll
                for (int c = 0; c < KP; ++c)
                    if ((act >> c) & 1u) s[c] = s_long[t * KP + c];
            }
        }
    }
    T y[KP];
#pragma unroll
    for (int c = 0; c < KP; ++c) y[c] = s[c];
    if (row < a.n) {
        if (a.mode & HIPK_MS_RESID) {
            T bv[KP];
            hipk_mld<T, KP>((const T *)a.bsub + (size_t)row * KP, act, bv);
#pragma unroll
            for (int c = 0; c < KP; ++c)
                if ((act >> c) & 1u) y[c] = bv[c] - s[c];
        }
        if (a.mode & HIPK_MS_SCALE) {
            const T d = ((const T *)a.dinv)[row];
#pragma unroll
            for (int c = 0; c < KP; ++c)
                if ((act >> c) & 1u) y[c] = d * y[c];
        }
        hipk_mst<T, KP>((T *)a.y + (size_t)row * KP, act, y);
    }
    // fused tile dots: per wavefront the tree of 64 rounded products, then ((w0 + w1) + (w2 + w3))
    const int wv = t >> 6, lane = t & 63;
    if (a.mode & HIPK_MS_DOT_YY) {
#pragma unroll
        for (int c = 0; c < KP; ++c)
            if ((act >> c) & 1u) {
                const double pr = (row < a.n) ? (double)y[c] * (double)y[c] : 0.0;
                const double sw = hipk_wave_sum(pr);
                if (lane == 0) s_w[wv * KP + c] = sw;
            }
    }
    if (a.mode & HIPK_MS_DOT_W) {
        T wv_[KP];
#pragma unroll
        for (int c = 0; c < KP; ++c) wv_[c] = (T)0;
        if (row < a.n) hipk_mld<T, KP>((const T *)a.w + (size_t)row * KP, act, wv_);
#pragma unroll
        for (int c = 0; c < KP; ++c)
            if ((act >> c) & 1u) {
                const double pr = (row < a.n) ? (double)wv_[c] * (double)y[c] : 0.0;
                const double sw = hipk_wave_sum(pr);
                if (lane == 0) s_w[4 * KP + wv * KP + c] = sw;
            }
    }
    __syncthreads();
    if (t < KP && ((act >> t) & 1u)) {
        if (a.mode & HIPK_MS_DOT_YY)
            a.tp0[tile * KP + t] = (s_w[t] + s_w[KP + t]) + (s_w[2 * KP + t] + s_w[3 * KP + t]);
        if (a.mode & HIPK_MS_DOT_W)
            a.tp1[tile * KP + t] = (s_w[4 * KP + t] + s_w[5 * KP + t]) + (s_w[6 * KP + t] + s_w[7 * KP + t]);
    }
    if (tile == 0 && t == 0) a.blk->spmvs += 1;
}

// per chunk: the tile sums of its tiles folded into the chunk partial (thread t takes tiles t, t + 256, .., then the tree)
template <int KP>
__global__ __launch_bounds__(HIPK_THREADS) void hipk_mcombine_kernel(int64_t ntiles, int tpc, int k, const hipk_mcol *cs,
                                                                     const hipk_mblk *blk, int64_t it, int all, const double *tp0,
                                                                     double *part0, const double *tp1, double *part1) {
    __shared__ unsigned s_act;
    __shared__ double lds[128 * KP];
    const unsigned act = hipk_mmask(cs, blk, k, it, all != 0, &s_act);
    if (!act) return;
    const int64_t t0 = (int64_t)blockIdx.x * tpc;
    const int cnt = (int)((ntiles - t0) < tpc ? (ntiles - t0) : tpc);
    double v[KP];
    for (int d = 0; d < 2; ++d) {
        const double *tp = d ? tp1 : tp0;
        double *part = d ? part1 : part0;
        if (!tp) continue;
        hipk_mfold<KP>(tp + t0 * KP, cnt, act, lds, v);
        if (threadIdx.x == 0) {
#pragma unroll
            for (int c = 0; c < KP; ++c)
                if ((act >> c) & 1u) part[(size_t)blockIdx.x * KP + c] = v[c];
        }
    }
}

// ------------------------------------------------------------------ chunk loops
// virtual thread t of chunk c owns rows {VEC t .. VEC t + VEC - 1} + 256 VEC j (VEC = 16 B / sizeof(T)), ascending
template <typename T, typename F>
__device__ __forceinline__ void hipk_mchunk(int64_t n, int ch, F &&f) {
    constexpr int VEC = hipk_vec<T>::VEC;
    const int64_t base = (int64_t)blockIdx.x * ch;
    const int64_t end = (base + ch < n) ? base + ch : n;
    for (int64_t i = base + (int64_t)threadIdx.x * VEC; i < end; i += (int64_t)HIPK_THREADS * VEC) {
#pragma unroll
        for (int v = 0; v < VEC; ++v)
            if (i + v < end) f(i + v);
    }
}

// plain chunked dot per column: mode 0 fma(a, b); mode 2 fma(m, m), m = dinv .* a (the Jacobi epilogue's ||M (b - A x)||^2)
template <typename T, int KP>
__global__ __launch_bounds__(HIPK_THREADS) void hipk_mdot_kernel(int64_t n, int ch, int k, const T *a, const T *b, const T *dinv,
                                                                 int mode, double *part) {
    __shared__ double lds[128 * KP];
    const unsigned act = hipk_mall(k);
    double acc[KP];
#pragma unroll
    for (int c = 0; c < KP; ++c) acc[c] = 0.0;
    hipk_mchunk<T>(n, ch, [&](int64_t i) {
        T av[KP], bv[KP];
        hipk_mld<T, KP>(a + i * KP, act, av);
        if (mode == 2) {
            const T d = dinv[i];
#pragma unroll
            for (int c = 0; c < KP; ++c)
                if ((act >> c) & 1u) {
                    const T m = d * av[c];
                    acc[c] = fma((double)m, (double)m, acc[c]);
                }
        } else {
            hipk_mld<T, KP>(b + i * KP, act, bv);
#pragma unroll
            for (int c = 0; c < KP; ++c)
                if ((act >> c) & 1u) acc[c] = fma((double)av[c], (double)bv[c], acc[c]);
        }
    });
    hipk_msum<KP>(acc, act, lds);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < KP; ++c)
            if ((act >> c) & 1u) part[(size_t)blockIdx.x * KP + c] = acc[c];
    }
}

// (n, ld) user block <-> (n, KP) work block, columns < k only
template <typename T, int KP>
__global__ __launch_bounds__(HIPK_THREADS) void hipk_mpack_kernel(int64_t n, int k, const T *src, int64_t lds_, T *dst, int64_t ldd,
                                                                  int to_user) {
    const int64_t i = (int64_t)blockIdx.x * HIPK_THREADS + threadIdx.x;
    if (i >= n) return;
    for (int c = 0; c < k; ++c) {
        if (to_user)
            dst[i * ldd + c] = src[i * KP + c];
        else
            dst[i * KP + c] = src[i * lds_ + c];
    }
}

// dst = src (or dinv .* src), up to three destinations; columns < k
template <typename T, int KP>
__global__ __launch_bounds__(HIPK_THREADS) void hipk_mcopy_kernel(int64_t n, int k, const T *src, const T *dinv, T *d0, T *d1, T *d2) {
    const int64_t i = (int64_t)blockIdx.x * HIPK_THREADS + threadIdx.x;
    if (i >= n) return;
    const unsigned act = hipk_mall(k);
    T v[KP];
    hipk_mld<T, KP>(src + i * KP, act, v);
    if (dinv) {
        const T d = dinv[i];
#pragma unroll
        for (int c = 0; c < KP; ++c)
            if ((act >> c) & 1u) v[c] = d * v[c];
    }
    hipk_mst<T, KP>(d0 + i * KP, act, v);
    if (d1) hipk_mst<T, KP>(d1 + i * KP, act, v);
    if (d2) hipk_mst<T, KP>(d2 + i * KP, act, v);
}

static __device__ __forceinline__ void hipk_mreport(hipk_mcol *cs, hipk_mblk *blk, int k, int64_t next) {
    bool all = true;
    for (int c = 0; c < k; ++c)
        if (cs[c].stop_it > next) all = false;
    if (all) blk->all_stop = next;
    hipk_signal(blk->host_sig, all ? (HIPK_SIG_STOP | next) : next);
}

// ------------------------------------------------------------------ CG (PRE: Jacobi, M = diag(dinv); orc_cg / orc_pcg_jacobi)
// <b,b>, the residual's tiled <r,r> (and PRE: <r,z>) -> per column bs, atol2, gamma0, stop word
template <int KP, bool PRE>
__global__ __launch_bounds__(HIPK_THREADS) void hipk_mcg_init_kernel(int g, int k, hipk_mcol *cs, hipk_mblk *blk, const double *part_bb,
                                                                     const double *part_rr, const double *part_rz, double tol2,
                                                                     double atol_sq, int64_t maxiter, int64_t *host_sig) {
    __shared__ double lds[128 * KP];
    const unsigned act = hipk_mall(k);
    double bs[KP], rr[KP], rz[KP];
    hipk_mfold<KP>(part_bb, g, act, lds, bs);
    hipk_mfold<KP>(part_rr, g, act, lds, rr);
    if (PRE) hipk_mfold<KP>(part_rz, g, act, lds, rz);
    if (threadIdx.x != 0) return;
    bool all = true;
#pragma unroll
    for (int c = 0; c < KP; ++c) {
        if (c >= k) continue;
        hipk_mcol &s = cs[c];
        const double a2 = tol2 * bs[c];
        s.atol2 = (a2 > atol_sq) ? a2 : atol_sq;
        s.bs = bs[c];
        s.gamma[0] = PRE ? rz[c] : rr[c];
        s.gamma[1] = 0.0;
        s.rs = rr[c];
        s.alpha = 0.0;
        s.iters = 0;
        s.code = 0;
        s.extra_mv = 0;
        const bool done = (maxiter <= 0 || rr[c] <= s.atol2);  // TSL:841 before the first SpMV
        s.stop_it = done ? 0 : INT64_MAX;
        if (!done) all = false;
    }
    blk->host_sig = host_sig;
    blk->all_stop = all ? 0 : INT64_MAX;
    if (all) hipk_signal(host_sig, HIPK_SIG_STOP);
}

// alpha = gamma / <p,Ap>; r -= alpha Ap; chunk partials of <r,r> (PRE: and <r,z>, z = dinv .* r)
template <typename T, int KP, bool PRE>
__global__ __launch_bounds__(HIPK_THREADS) void hipk_mcg_update_kernel(int64_t n, int ch, int g, int k, hipk_mcol *cs, const hipk_mblk *blk,
                                                                       int64_t it, const double *part_pap, const T *Ap, T *r,
                                                                       const T *dinv, double *part_rr, double *part_rz) {
    __shared__ unsigned s_act;
    __shared__ double lds[128 * KP];
    const unsigned act = hipk_mmask(cs, blk, k, it, false, &s_act);
    if (!act) return;
    double pap[KP];
    hipk_mfold<KP>(part_pap, g, act, lds, pap);
    T alpha[KP];
    double rr[KP], rz[KP];
#pragma unroll
    for (int c = 0; c < KP; ++c) {
        const double q = ((act >> c) & 1u) ? cs[c].gamma[it & 1] / pap[c] : 0.0;  // TSL:846
        alpha[c] = (T)q;
        rr[c] = 0.0;
        rz[c] = 0.0;
        if (blockIdx.x == 0 && threadIdx.x == 0 && ((act >> c) & 1u)) cs[c].alpha = q;
    }
    hipk_mchunk<T>(n, ch, [&](int64_t i) {
        T av[KP], rv[KP];
        hipk_mld<T, KP>(Ap + i * KP, act, av);
        hipk_mld<T, KP>(r + i * KP, act, rv);
        T d = (T)0;
        if (PRE) d = dinv[i];
#pragma unroll
        for (int c = 0; c < KP; ++c)
            if ((act >> c) & 1u) {
                const T m1 = alpha[c] * av[c];
                rv[c] = rv[c] - m1;  // TSL:848
                rr[c] = fma((double)rv[c], (double)rv[c], rr[c]);
                if (PRE) {
                    const T z = d * rv[c];
                    rz[c] = fma((double)rv[c], (double)z, rz[c]);
                }
            }
        hipk_mst<T, KP>(r + i * KP, act, rv);
    });
    hipk_msum<KP>(rr, act, lds);
    if (PRE) hipk_msum<KP>(rz, act, lds);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < KP; ++c)
            if ((act >> c) & 1u) {
                part_rr[(size_t)blockIdx.x * KP + c] = rr[c];
                if (PRE) part_rz[(size_t)blockIdx.x * KP + c] = rz[c];
            }
    }
}

// beta = <r,r> / gamma (PRE: <r,z> / gamma); x += alpha p; p = r + beta p (PRE: p = dinv .* r + beta p); stop test per column
template <typename T, int KP, bool PRE>
__global__ __launch_bounds__(HIPK_THREADS) void hipk_mcg_direction_kernel(int64_t n, int ch, int g, int k, hipk_mcol *cs, hipk_mblk *blk,
                                                                          int64_t it, int64_t maxiter, const double *part_rr,
                                                                          const double *part_rz, const T *r, T *p, T *x, const T *dinv) {
    __shared__ unsigned s_act;
    __shared__ double lds[128 * KP];
    const unsigned act = hipk_mmask(cs, blk, k, it, false, &s_act);
    if (!act) return;
    double rr[KP], rz[KP];
    hipk_mfold<KP>(part_rr, g, act, lds, rr);
    if (PRE) hipk_mfold<KP>(part_rz, g, act, lds, rz);
    T alpha[KP], beta[KP];
#pragma unroll
    for (int c = 0; c < KP; ++c) {
        const bool on = (act >> c) & 1u;
        const double gamma = on ? cs[c].gamma[it & 1] : 1.0;
        alpha[c] = on ? (T)cs[c].alpha : (T)0;
        beta[c] = (T)((PRE ? rz[c] : rr[c]) / gamma);  // TSL:851
    }
    hipk_mchunk<T>(n, ch, [&](int64_t i) {
        T rv[KP], pv[KP], xv[KP];
        hipk_mld<T, KP>(r + i * KP, act, rv);
        hipk_mld<T, KP>(p + i * KP, act, pv);
        hipk_mld<T, KP>(x + i * KP, act, xv);
        T d = (T)0;
        if (PRE) d = dinv[i];
#pragma unroll
        for (int c = 0; c < KP; ++c)
            if ((act >> c) & 1u) {
                const T m0 = alpha[c] * pv[c];
                xv[c] = xv[c] + m0;  // TSL:847
                const T z = PRE ? d * rv[c] : rv[c];
                const T m = beta[c] * pv[c];
                pv[c] = z + m;  // TSL:852
            }
        hipk_mst<T, KP>(x + i * KP, act, xv);
        hipk_mst<T, KP>(p + i * KP, act, pv);
    });
    if (blockIdx.x == 0 && threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < KP; ++c)
            if ((act >> c) & 1u) {
                hipk_mcol &s = cs[c];
                s.gamma[(it + 1) & 1] = PRE ? rz[c] : rr[c];  // TSL:853
                s.rs = rr[c];
                if (it + 1 >= maxiter || rr[c] <= s.atol2) s.stop_it = it + 1;  // TSL:841 for the next pass
            }
        hipk_mreport(cs, blk, k, it + 1);
    }
}

// epilogue: res2 and <x,x> per column (all columns)
template <int KP>
__global__ __launch_bounds__(HIPK_THREADS) void hipk_mfinal_kernel(int g, int k, hipk_mcol *cs, const double *part_res,
                                                                   const double *part_xx) {
    __shared__ double lds[128 * KP];
    const unsigned act = hipk_mall(k);
    double res[KP], xx[KP];
    hipk_mfold<KP>(part_res, g, act, lds, res);
    hipk_mfold<KP>(part_xx, g, act, lds, xx);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < KP; ++c)
            if (c < k) {
                cs[c].res2 = res[c];
                cs[c].xx = xx[c];
            }
    }
}

// ------------------------------------------------------------------ BiCGStab (PRE: Jacobi; bicgstab_impl of the oracle)
template <int KP>
__global__ __launch_bounds__(HIPK_THREADS) void hipk_mbi_init_kernel(int g, int k, hipk_mcol *cs, hipk_mblk *blk, const double *part_bb,
                                                                     double tol2, double atol_sq, int64_t maxiter, int64_t *host_sig) {
    __shared__ double lds[128 * KP];
    const unsigned act = hipk_mall(k);
    double bs[KP];
    hipk_mfold<KP>(part_bb, g, act, lds, bs);
    if (threadIdx.x != 0) return;
#pragma unroll
    for (int c = 0; c < KP; ++c) {
        if (c >= k) continue;
        hipk_mcol &s = cs[c];
        const double a2 = tol2 * bs[c];
        s.atol2 = (a2 > atol_sq) ? a2 : atol_sq;
        s.bs = bs[c];
        s.rho = 1.0;
        s.alpha = 1.0;
        s.omega = 1.0;
        s.rs = 0.0;
        s.iters = 0;
        s.code = 0;
        s.extra_mv = 0;
        s.stop_it = (maxiter <= 0) ? 0 : INT64_MAX;
    }
    blk->host_sig = host_sig;
    blk->all_stop = (maxiter <= 0) ? 0 : INT64_MAX;
    if (maxiter <= 0) hipk_signal(host_sig, HIPK_SIG_STOP);
}

// rs, rho' -> convergence and rho breakdown tests; beta; p = r + beta (p - omega q) (PRE: phat = dinv .* p)
template <typename T, int KP, bool PRE>
__global__ __launch_bounds__(HIPK_THREADS) void hipk_mbi_direction_kernel(int64_t n, int ch, int g, int k, hipk_mcol *cs, const hipk_mblk *blk,
                                                                          int64_t it, const double *part_rr, const double *part_rhr,
                                                                          const T *r, const T *q, T *p, const T *dinv, T *phat) {
    __shared__ unsigned s_act;
    __shared__ double lds[128 * KP];
    const unsigned act = hipk_mmask(cs, blk, k, it, false, &s_act);
    if (!act) return;
    double rs[KP], rhn[KP];
    hipk_mfold<KP>(part_rr, g, act, lds, rs);
    hipk_mfold<KP>(part_rhr, g, act, lds, rhn);
    constexpr double EPS = hipk_meps<T>::v;
    unsigned live = 0;
    T beta[KP], om[KP];
#pragma unroll
    for (int c = 0; c < KP; ++c) {
        beta[c] = (T)0;
        om[c] = (T)0;
        if (!((act >> c) & 1u)) continue;
        const hipk_mcol &s = cs[c];
        int code = 1;                                              // 1: goes on
        if (rs[c] <= s.atol2) code = 0;                            // TSL:894-896
        else if (fabs(rhn[c]) < EPS * fabs(s.rho)) code = -10;     // TSL:902-904
        if (code == 1) {
            live |= 1u << c;
            beta[c] = (T)(rhn[c] / s.rho * s.alpha / s.omega);     // TSL:906, left to right
            om[c] = (T)s.omega;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < KP; ++c)
            if ((act >> c) & 1u) {
                hipk_mcol &s = cs[c];
                s.rs = rs[c];
                if ((live >> c) & 1u) {
                    s.rho_new = rhn[c];
                } else {
                    s.code = (rs[c] <= s.atol2) ? 0 : -10;
                    s.stop_it = it;
                }
            }
    }
    if (!live) return;
    hipk_mchunk<T>(n, ch, [&](int64_t i) {
        T rv[KP], qv[KP], pv[KP];
        hipk_mld<T, KP>(r + i * KP, live, rv);
        hipk_mld<T, KP>(q + i * KP, live, qv);
        hipk_mld<T, KP>(p + i * KP, live, pv);
#pragma unroll
        for (int c = 0; c < KP; ++c)
            if ((live >> c) & 1u) {  // TSL:907
                const T t1 = om[c] * qv[c];
                const T t2 = pv[c] - t1;
                const T t3 = beta[c] * t2;
                pv[c] = rv[c] + t3;
            }
        hipk_mst<T, KP>(p + i * KP, live, pv);
        if (PRE) {
            const T d = dinv[i];
#pragma unroll
            for (int c = 0; c < KP; ++c)
                if ((live >> c) & 1u) pv[c] = d * pv[c];  // TSL:908
            hipk_mst<T, KP>(phat + i * KP, live, pv);
        }
    });
}

// alpha' = rho' / <rhat,q> -> alpha breakdown test; s = r - alpha' q (PRE: shat = dinv .* s); chunk partials of <s,s>
template <typename T, int KP, bool PRE>
__global__ __launch_bounds__(HIPK_THREADS) void hipk_mbi_supdate_kernel(int64_t n, int ch, int g, int k, hipk_mcol *cs, const hipk_mblk *blk,
                                                                        int64_t it, const double *part_rq, const T *r, const T *q, T *s,
                                                                        const T *dinv, T *shat, double *part_ss) {
    __shared__ unsigned s_act;
    __shared__ double lds[128 * KP];
    const unsigned act = hipk_mmask(cs, blk, k, it, false, &s_act);
    if (!act) return;
    double rq[KP];
    hipk_mfold<KP>(part_rq, g, act, lds, rq);
    constexpr double EPS = hipk_meps<T>::v;
    unsigned live = 0;
    T al[KP];
    double an[KP];
#pragma unroll
    for (int c = 0; c < KP; ++c) {
        al[c] = (T)0;
        an[c] = 0.0;
        if (!((act >> c) & 1u)) continue;
        an[c] = cs[c].rho_new / rq[c];  // TSL:910
        if (!(fabs(an[c]) < EPS)) {     // TSL:913-915
            live |= 1u << c;
            al[c] = (T)an[c];
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < KP; ++c)
            if ((act >> c) & 1u) {
                hipk_mcol &st = cs[c];
                if ((live >> c) & 1u) {
                    st.alpha_new = an[c];
                } else {
                    st.code = -11;
                    st.extra_mv = 1;
                    st.stop_it = it;
                }
            }
    }
    if (!live) return;
    double acc[KP];
#pragma unroll
    for (int c = 0; c < KP; ++c) acc[c] = 0.0;
    hipk_mchunk<T>(n, ch, [&](int64_t i) {
        T rv[KP], qv[KP];
        hipk_mld<T, KP>(r + i * KP, live, rv);
        hipk_mld<T, KP>(q + i * KP, live, qv);
#pragma unroll
        for (int c = 0; c < KP; ++c)
            if ((live >> c) & 1u) {
                const T m = al[c] * qv[c];
                rv[c] = rv[c] - m;  // TSL:917
                acc[c] = fma((double)rv[c], (double)rv[c], acc[c]);
            }
        hipk_mst<T, KP>(s + i * KP, live, rv);
        if (PRE) {
            const T d = dinv[i];
#pragma unroll
            for (int c = 0; c < KP; ++c)
                if ((live >> c) & 1u) rv[c] = d * rv[c];  // TSL:922
            hipk_mst<T, KP>(shat + i * KP, live, rv);
        }
    });
    hipk_msum<KP>(acc, live, lds);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < KP; ++c)
            if ((live >> c) & 1u) part_ss[(size_t)blockIdx.x * KP + c] = acc[c];
    }
}

// omega' -> early exit and omega breakdown tests; x += alpha' phat (+ omega' shat); r = s (- omega' t); partials of <r,r>, <rhat,r>;
// the iteration's bookkeeping (workgroup 0, also when no column is left: it reports the block's stop)
template <typename T, int KP, bool PRE>
__global__ __launch_bounds__(HIPK_THREADS) void hipk_mbi_xupdate_kernel(int64_t n, int ch, int g, int k, hipk_mcol *cs, hipk_mblk *blk,
                                                                        int64_t it, int64_t maxiter, const double *part_ss,
                                                                        const double *part_ts, const double *part_tt, const T *ph,
                                                                        const T *s, const T *t, const T *shat, const T *rhat, T *x, T *r,
                                                                        double *part_rr, double *part_rhr) {
    __shared__ unsigned s_act, s_go;
    __shared__ double lds[128 * KP];
    if (threadIdx.x == 0) s_go = (it < blk->all_stop) ? 1u : 0u;
    const unsigned act = hipk_mmask(cs, blk, k, it, false, &s_act);
    if (!s_go) return;
    constexpr double EPS = hipk_meps<T>::v;
    unsigned live = 0, early = 0;
    T al[KP], om[KP];
    double on[KP];
#pragma unroll
    for (int c = 0; c < KP; ++c) {
        al[c] = (T)0;
        om[c] = (T)0;
        on[c] = 0.0;
    }
    if (act) {
        double ss[KP], ts[KP], tt[KP];
        hipk_mfold<KP>(part_ss, g, act, lds, ss);
        hipk_mfold<KP>(part_ts, g, act, lds, ts);
        hipk_mfold<KP>(part_tt, g, act, lds, tt);
#pragma unroll
        for (int c = 0; c < KP; ++c) {
            if (!((act >> c) & 1u)) continue;
            const bool ee = ss[c] < cs[c].atol2;                            // TSL:920 (strict)
            on[c] = (fabs(tt[c]) < EPS) ? 0.0 : ts[c] / tt[c];              // TSL:926-930
            if (fabs(on[c]) < EPS && !ee) continue;                         // TSL:934-936
            live |= 1u << c;
            if (ee) early |= 1u << c;
            al[c] = (T)cs[c].alpha_new;
            om[c] = (T)on[c];
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < KP; ++c)
            if ((act >> c) & 1u) {
                hipk_mcol &st = cs[c];
                if ((live >> c) & 1u) {
                    st.rho = st.rho_new;
                    st.alpha = st.alpha_new;
                    st.omega = on[c];
                    st.iters = it + 1;
                    if (((early >> c) & 1u) || it + 1 >= maxiter) st.stop_it = it + 1;  // TSL:961, loop bound :892
                } else {
                    st.code = -11;
                    st.extra_mv = 2;
                    st.stop_it = it;
                }
            }
        hipk_mreport(cs, blk, k, it + 1);
    }
    if (!live) return;
    double a0[KP], a1[KP];
#pragma unroll
    for (int c = 0; c < KP; ++c) {
        a0[c] = 0.0;
        a1[c] = 0.0;
    }
    const unsigned full = live & ~early;
    hipk_mchunk<T>(n, ch, [&](int64_t i) {
        T sv[KP], pv[KP], xv[KP], hv[KP], tv[KP], shv[KP], rv[KP];
        hipk_mld<T, KP>(s + i * KP, live, sv);
        hipk_mld<T, KP>(ph + i * KP, live, pv);
        hipk_mld<T, KP>(x + i * KP, live, xv);
        hipk_mld<T, KP>(rhat + i * KP, live, hv);
        if (full) {
            hipk_mld<T, KP>(t + i * KP, full, tv);
            if (PRE) hipk_mld<T, KP>(shat + i * KP, full, shv);
        }
#pragma unroll
        for (int c = 0; c < KP; ++c)
            if ((live >> c) & 1u) {
                const T m0 = al[c] * pv[c];
                if ((early >> c) & 1u) {  // TSL:942-950 with exit_early true
                    xv[c] = xv[c] + m0;
                    rv[c] = sv[c];
                } else {
                    const T m1 = om[c] * (PRE ? shv[c] : sv[c]);  // TSL:942: omega * shat
                    const T m2 = m0 + m1;
                    xv[c] = xv[c] + m2;
                    const T m3 = om[c] * tv[c];
                    rv[c] = sv[c] - m3;
                }
                a0[c] = fma((double)rv[c], (double)rv[c], a0[c]);
                a1[c] = fma((double)hv[c], (double)rv[c], a1[c]);
            }
        hipk_mst<T, KP>(x + i * KP, live, xv);
        hipk_mst<T, KP>(r + i * KP, live, rv);
    });
    hipk_msum<KP>(a0, live, lds);
    hipk_msum<KP>(a1, live, lds);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < KP; ++c)
            if ((live >> c) & 1u) {
                part_rr[(size_t)blockIdx.x * KP + c] = a0[c];
                part_rhr[(size_t)blockIdx.x * KP + c] = a1[c];
            }
    }
}

// ------------------------------------------------------------------ host
static int hipk_mkp(int k) { return k <= 2 ? 2 : k <= 4 ? 4 : k <= 8 ? 8 : 16; }
static int hipk_mnvec(int solver, int precond) { return solver == 0 ? 5 : (precond ? 10 : 8); }  // incl. the packed b and x
static constexpr int kMParts = 6;   // chunk-partial slots
static constexpr size_t kMHead = 4096;  // hipk_mblk + HIPK_MULTI_MAXK hipk_mcol

struct hipk_mlayout {
    size_t parts, tiles, vec, total;
};
static hipk_mlayout hipk_mlayout_of(int64_t n, int kp, int dtype, int solver, int precond) {
    hipk_mlayout L;
    const hipk_geom gm = hipk_make_geom(n > 0 ? n : 1);
    const int64_t ntiles = ((n > 0 ? n : 1) + HIPK_TILE - 1) / HIPK_TILE;
    const size_t sv = (dtype == HIPK_F64) ? 8 : 4;
    L.parts = hipk_align_up((size_t)gm.g * kp * sizeof(double), 256);
    L.tiles = hipk_align_up((size_t)ntiles * kp * sizeof(double), 256);
    L.vec = hipk_align_up((size_t)(n > 0 ? n : 1) * kp * sv, 256);
    L.total = kMHead + kMParts * L.parts + 2 * L.tiles + (size_t)hipk_mnvec(solver, precond) * L.vec;
    return L;
}

extern "C" size_t hipk_multi_work_bytes(int64_t n, int k, int dtype, int solver, int precond) {
    const int kb = k < 1 ? 1 : (k > HIPK_MULTI_MAXK ? HIPK_MULTI_MAXK : k);
    return hipk_mlayout_of(n, hipk_mkp(kb), dtype, solver, precond ? 1 : 0).total;
}

template <typename T, int KP>
struct hipk_mctx {
    hipk_csr_s *A;
    hipStream_t s;
    int64_t n, ntiles;
    hipk_geom gm;
    int k;
    hipk_mcol *cs;
    hipk_mblk *blk;
    double *part[kMParts];
    double *tp0, *tp1;
    // block SpMV y = A x (mode flags) + the combine launch of its fused dots into part0 / part1
    void spmv(const T *x, T *y, int mode, int64_t it, const T *bsub, const T *w, const T *dinv, double *part0, double *part1) {
        hipk_mspmv_args a;
        a.crow = A->crow;
        a.col = A->col;
        a.val = A->val;
        a.n = n;
        a.k = k;
        a.mode = mode;
        a.x = x;
        a.bsub = bsub;
        a.w = w;
        a.dinv = dinv;
        a.y = y;
        a.tp0 = tp0;
        a.tp1 = tp1;
        a.cs = cs;
        a.blk = blk;
        a.it = it;
        if (A->max_row_len > HIPK_LONG_ROW)
            hipk_mspmv_kernel<T, KP, true><<<(unsigned)ntiles, HIPK_THREADS, 0, s>>>(a);
        else
            hipk_mspmv_kernel<T, KP, false><<<(unsigned)ntiles, HIPK_THREADS, 0, s>>>(a);
        if (part0 || part1)
            hipk_mcombine_kernel<KP><<<gm.g, HIPK_THREADS, 0, s>>>(ntiles, gm.ch / HIPK_TILE, k, cs, blk, it, (mode & HIPK_MS_ALL) ? 1 : 0,
                                                                  (mode & HIPK_MS_DOT_YY) ? tp0 : nullptr, part0,
                                                                  (mode & HIPK_MS_DOT_W) ? tp1 : nullptr, part1);
    }
};

// one block of k <= 16 columns: B, X user blocks (n, ldb) / (n, ldx), st: k entries; *spmvs += the block's working SpMV launches
template <typename T, int KP>
static int hipk_multi_block(hipk_csr_s *A, int solver, const T *dinv, int k, const T *B, int64_t ldb, T *X, int64_t ldx, char *work,
                            const hipk_params *prm, hipk_stats *st, int64_t *spmvs, double *ms_out, hipStream_t s) {
    const int64_t n = A->n_rows;
    const hipk_geom gm = A->geom;
    const bool pre = dinv != nullptr;
    const hipk_mlayout L = hipk_mlayout_of(n, KP, A->dtype, solver, pre ? 1 : 0);
    hipk_mctx<T, KP> cx;
    cx.A = A;
    cx.s = s;
    cx.n = n;
    cx.ntiles = (n + HIPK_TILE - 1) / HIPK_TILE;
    cx.gm = gm;
    cx.k = k;
    cx.blk = (hipk_mblk *)work;
    cx.cs = (hipk_mcol *)(work + 256);
    for (int i = 0; i < kMParts; ++i) cx.part[i] = (double *)(work + kMHead + i * L.parts);
    cx.tp0 = (double *)(work + kMHead + kMParts * L.parts);
    cx.tp1 = (double *)((char *)cx.tp0 + L.tiles);
    char *vb = (char *)cx.tp1 + L.tiles;
    auto V = [&](int i) { return (T *)(vb + (size_t)i * L.vec); };
    T *bw = V(0), *xw = V(1), *r = V(2);
    double **P = cx.part;
    hipk_mcol *cs = cx.cs;
    hipk_mblk *blk = cx.blk;
    const unsigned flat = (unsigned)((n + HIPK_THREADS - 1) / HIPK_THREADS);

    const int64_t maxiter = (prm->maxiter < 0) ? 10 * n : prm->maxiter;  // TSL:982-984
    const float tolf = (float)prm->tol, atolf = (float)prm->atol;       // torch.tensor(python float) is fp32 (TSL:816-817)
    const double tol2 = (double)(tolf * tolf), atol_sq = (double)(atolf * atolf);
    const int64_t check = prm->check_every > 0 ? prm->check_every : 64;

    hipk_event_pair whole;
    HIPK_CHECK_HIP(whole.create());
    HIPK_CHECK_HIP(hipEventRecord(whole.a, s));
    HIPK_CHECK_HIP(hipMemsetAsync(blk, 0, sizeof(hipk_mblk), s));
    hipk_mpack_kernel<T, KP><<<flat, HIPK_THREADS, 0, s>>>(n, k, B, ldb, bw, KP, 0);
    hipk_mpack_kernel<T, KP><<<flat, HIPK_THREADS, 0, s>>>(n, k, X, ldx, xw, KP, 0);
    hipk_pacer pace(A->host_poll, &blk->all_stop, check);
    int64_t it = 0, stop = INT64_MAX;
    const int ALL = HIPK_MS_ALL;

    if (solver == 0) {  // ---------------------------------------------------------------- CG / Jacobi PCG
        T *p = V(3), *Ap = V(4);
        // r0 = b - A x0 with the tiled <r0,r0> (TSL:820, 826); <b,b> (TSL:815); p = r0 (PRE: dinv .* r0) and <r0, z0>
        cx.spmv(xw, r, HIPK_MS_RESID | HIPK_MS_DOT_YY | ALL, 0, bw, nullptr, nullptr, P[1], nullptr);
        hipk_mdot_kernel<T, KP><<<gm.g, HIPK_THREADS, 0, s>>>(n, gm.ch, k, bw, bw, nullptr, 0, P[0]);
        hipk_mcopy_kernel<T, KP><<<flat, HIPK_THREADS, 0, s>>>(n, k, r, dinv, p, nullptr, nullptr);
        if (pre) hipk_mdot_kernel<T, KP><<<gm.g, HIPK_THREADS, 0, s>>>(n, gm.ch, k, r, p, nullptr, 0, P[2]);
        HIPK_CHECK_HIP(pace.create());
        if (pre)
            hipk_mcg_init_kernel<KP, true><<<1, HIPK_THREADS, 0, s>>>(gm.g, k, cs, blk, P[0], P[1], P[2], tol2, atol_sq, maxiter,
                                                                     pace.device_sig());
        else
            hipk_mcg_init_kernel<KP, false><<<1, HIPK_THREADS, 0, s>>>(gm.g, k, cs, blk, P[0], P[1], nullptr, tol2, atol_sq, maxiter,
                                                                      pace.device_sig());
        HIPK_CHECK_HIP(hipGetLastError());
        for (; it < maxiter; ++it) {
            HIPK_CHECK_HIP(pace.gate(it, s, &stop));
            if (stop <= it) break;
            cx.spmv(p, Ap, HIPK_MS_DOT_W, it, nullptr, p, nullptr, nullptr, P[3]);
            if (pre) {
                hipk_mcg_update_kernel<T, KP, true><<<gm.g, HIPK_THREADS, 0, s>>>(n, gm.ch, gm.g, k, cs, blk, it, P[3], Ap, r, dinv, P[1], P[2]);
                hipk_mcg_direction_kernel<T, KP, true><<<gm.g, HIPK_THREADS, 0, s>>>(n, gm.ch, gm.g, k, cs, blk, it, maxiter, P[1], P[2], r, p,
                                                                                     xw, dinv);
            } else {
                hipk_mcg_update_kernel<T, KP, false><<<gm.g, HIPK_THREADS, 0, s>>>(n, gm.ch, gm.g, k, cs, blk, it, P[3], Ap, r, nullptr, P[1],
                                                                                   nullptr);
                hipk_mcg_direction_kernel<T, KP, false><<<gm.g, HIPK_THREADS, 0, s>>>(n, gm.ch, gm.g, k, cs, blk, it, maxiter, P[1], nullptr, r,
                                                                                      p, xw, nullptr);
            }
            if ((it & 63) == 63) HIPK_CHECK_HIP(hipGetLastError());
        }
        // TSL:1007-1014: the true residual (PRE: ||M (b - A x)||, a plain dot of the scaled residual), ||x||
        cx.spmv(xw, Ap, HIPK_MS_RESID | ALL | (pre ? 0 : HIPK_MS_DOT_YY), 0, bw, nullptr, nullptr, pre ? nullptr : P[4], nullptr);
        if (pre) hipk_mdot_kernel<T, KP><<<gm.g, HIPK_THREADS, 0, s>>>(n, gm.ch, k, Ap, nullptr, dinv, 2, P[4]);
    } else {  // ---------------------------------------------------------------------------- BiCGStab / Jacobi BiCGStab
        T *rhat = V(3), *p = V(4), *q = V(5), *sv = V(6), *t = V(7);
        T *phat = pre ? V(8) : p, *shat = pre ? V(9) : sv;
        // r0 with the tiled <r0,r0> (= <rhat, r0>); rhat = p = q = r0 (TSL:876, 890)
        cx.spmv(xw, r, HIPK_MS_RESID | HIPK_MS_DOT_YY | ALL, 0, bw, nullptr, nullptr, P[0], nullptr);
        hipk_mdot_kernel<T, KP><<<gm.g, HIPK_THREADS, 0, s>>>(n, gm.ch, k, bw, bw, nullptr, 0, P[5]);
        hipk_mcopy_kernel<T, KP><<<flat, HIPK_THREADS, 0, s>>>(n, k, r, nullptr, rhat, p, q);
        HIPK_CHECK_HIP(pace.create());
        hipk_mbi_init_kernel<KP><<<1, HIPK_THREADS, 0, s>>>(gm.g, k, cs, blk, P[5], tol2, atol_sq, maxiter, pace.device_sig());
        HIPK_CHECK_HIP(hipGetLastError());
        for (; it < maxiter; ++it) {
            HIPK_CHECK_HIP(pace.gate(it, s, &stop));
            if (stop <= it) break;
            const double *prhr = it == 0 ? P[0] : P[1];
            if (pre)
                hipk_mbi_direction_kernel<T, KP, true><<<gm.g, HIPK_THREADS, 0, s>>>(n, gm.ch, gm.g, k, cs, blk, it, P[0], prhr, r, q, p, dinv,
                                                                                     phat);
            else
                hipk_mbi_direction_kernel<T, KP, false><<<gm.g, HIPK_THREADS, 0, s>>>(n, gm.ch, gm.g, k, cs, blk, it, P[0], prhr, r, q, p,
                                                                                      nullptr, nullptr);
            cx.spmv(phat, q, HIPK_MS_DOT_W, it, nullptr, rhat, nullptr, nullptr, P[2]);  // q = A phat, <rhat,q>
            if (pre)
                hipk_mbi_supdate_kernel<T, KP, true><<<gm.g, HIPK_THREADS, 0, s>>>(n, gm.ch, gm.g, k, cs, blk, it, P[2], r, q, sv, dinv, shat,
                                                                                   P[3]);
            else
                hipk_mbi_supdate_kernel<T, KP, false><<<gm.g, HIPK_THREADS, 0, s>>>(n, gm.ch, gm.g, k, cs, blk, it, P[2], r, q, sv, nullptr,
                                                                                    nullptr, P[3]);
            cx.spmv(shat, t, HIPK_MS_DOT_YY | HIPK_MS_DOT_W, it, nullptr, sv, nullptr, P[4], P[5]);  // t = A shat, <t,t>, <s,t>
            if (pre)
                hipk_mbi_xupdate_kernel<T, KP, true><<<gm.g, HIPK_THREADS, 0, s>>>(n, gm.ch, gm.g, k, cs, blk, it, maxiter, P[3], P[5], P[4],
                                                                                   phat, sv, t, shat, rhat, xw, r, P[0], P[1]);
            else
                hipk_mbi_xupdate_kernel<T, KP, false><<<gm.g, HIPK_THREADS, 0, s>>>(n, gm.ch, gm.g, k, cs, blk, it, maxiter, P[3], P[5], P[4],
                                                                                    p, sv, t, nullptr, rhat, xw, r, P[0], P[1]);
            if ((it & 63) == 63) HIPK_CHECK_HIP(hipGetLastError());
        }
        // TSL:1007-1014 (PRE: M (b - A x), the row scaling after the product)
        cx.spmv(xw, t, HIPK_MS_RESID | HIPK_MS_DOT_YY | ALL | (pre ? HIPK_MS_SCALE : 0), 0, bw, nullptr, dinv, P[4], nullptr);
    }
    hipk_mdot_kernel<T, KP><<<gm.g, HIPK_THREADS, 0, s>>>(n, gm.ch, k, xw, xw, nullptr, 0, P[5]);
    hipk_mfinal_kernel<KP><<<1, HIPK_THREADS, 0, s>>>(gm.g, k, cs, P[4], P[5]);
    hipk_mpack_kernel<T, KP><<<flat, HIPK_THREADS, 0, s>>>(n, k, xw, KP, X, ldx, 1);
    HIPK_CHECK_HIP(hipGetLastError());
    HIPK_CHECK_HIP(hipEventRecord(whole.b, s));
    hipk_mcol hc[HIPK_MULTI_MAXK];
    hipk_mblk hb;
    HIPK_CHECK_HIP(hipMemcpyAsync(hc, cs, sizeof(hipk_mcol) * k, hipMemcpyDeviceToHost, s));
    HIPK_CHECK_HIP(hipMemcpyAsync(&hb, blk, sizeof(hb), hipMemcpyDeviceToHost, s));
    HIPK_CHECK_HIP(hipStreamSynchronize(s));
    float ms = 0.f;
    HIPK_CHECK_HIP(hipEventElapsedTime(&ms, whole.a, whole.b));
    for (int c = 0; c < k; ++c) {
        const hipk_mcol &h = hc[c];
        hipk_stats *o = st + c;
        memset(o, 0, sizeof(*o));
        int64_t iters, mv;
        if (solver == 0) {
            iters = h.stop_it < it ? h.stop_it : it;  // the device's stop word is authoritative
            mv = iters + 2;
        } else {
            iters = h.iters;
            mv = 1 + 2 * iters + h.extra_mv + 1;
            o->breakdown = h.code;
        }
        hipk_finish_isolve_stats(o, prm, h.bs, h.res2, h.xx, iters, mv);
        o->recurrence_rs = h.rs;
        o->solve_ms = ms;
    }
    *spmvs += hb.spmvs;
    *ms_out += ms;
    return HIPK_OK;
}

template <typename T>
static int hipk_multi_run(hipk_csr_s *A, int solver, const T *dinv, int k, const T *B, int64_t ldb, T *X, int64_t ldx, char *work,
                          const hipk_params *prm, hipk_stats *st, int64_t *spmvs, hipStream_t s) {
    double ms = 0.0;
    for (int j0 = 0; j0 < k; j0 += HIPK_MULTI_MAXK) {
        const int kb = (k - j0) < HIPK_MULTI_MAXK ? (k - j0) : HIPK_MULTI_MAXK;
        int rc;
        switch (hipk_mkp(kb)) {
            case 2: rc = hipk_multi_block<T, 2>(A, solver, dinv, kb, B + j0, ldb, X + j0, ldx, work, prm, st + j0, spmvs, &ms, s); break;
            case 4: rc = hipk_multi_block<T, 4>(A, solver, dinv, kb, B + j0, ldb, X + j0, ldx, work, prm, st + j0, spmvs, &ms, s); break;
            case 8: rc = hipk_multi_block<T, 8>(A, solver, dinv, kb, B + j0, ldb, X + j0, ldx, work, prm, st + j0, spmvs, &ms, s); break;
            default: rc = hipk_multi_block<T, 16>(A, solver, dinv, kb, B + j0, ldb, X + j0, ldx, work, prm, st + j0, spmvs, &ms, s); break;
        }
        if (rc != HIPK_OK) return rc;
    }
    return HIPK_OK;
}

static int hipk_solve_multi(int solver, hipk_csr_t A, const void *dinv, int k, const void *B, int64_t ldb, void *X, int64_t ldx,
                            void *work, size_t work_bytes, const hipk_params *prm, hipk_stats *st, int64_t *block_spmvs,
                            hipk_stream_t stream) {
    HIPK_REQUIRE(A && B && X && work && prm && st && block_spmvs, HIPK_ERR_ARG, "null argument");
    HIPK_REQUIRE(A->n_rows == A->n_cols, HIPK_ERR_ARG, "linear operator must be a square matrix");
    HIPK_REQUIRE(A->n_rows > 0, HIPK_ERR_ARG, "empty system");
    HIPK_REQUIRE(A->crow != nullptr && A->op_cb == nullptr, HIPK_ERR_ARG, "the block solves need a CSR matrix handle");
    HIPK_REQUIRE(k >= 1, HIPK_ERR_ARG, "k must be at least 1");
    HIPK_REQUIRE(ldb >= k && ldx >= k, HIPK_ERR_ARG, "ldb and ldx must be at least k");
    HIPK_REQUIRE((((uintptr_t)work) & 255u) == 0, HIPK_ERR_ALIGN, "work must be 256-byte aligned");
    HIPK_REQUIRE(work_bytes >= hipk_multi_work_bytes(A->n_rows, k, A->dtype, solver, dinv != nullptr), HIPK_ERR_WORKSPACE,
                 "work too small");
    HIPK_REQUIRE(B != X, HIPK_ERR_ARG, "B and X must not alias");
    *block_spmvs = 0;
    hipk_set_solve_path(nullptr, solver == 0 ? "hipk_cg_multi launch sequence" : "hipk_bicgstab_multi launch sequence");
    if (A->dtype == HIPK_F64)
        return hipk_multi_run<double>(A, solver, (const double *)dinv, k, (const double *)B, ldb, (double *)X, ldx, (char *)work, prm, st,
                                      block_spmvs, (hipStream_t)stream);
    return hipk_multi_run<float>(A, solver, (const float *)dinv, k, (const float *)B, ldb, (float *)X, ldx, (char *)work, prm, st,
                                 block_spmvs, (hipStream_t)stream);
}

extern "C" int hipk_cg_solve_multi(hipk_csr_t A, const void *dinv, int k, const void *B, int64_t ldb, void *X, int64_t ldx, void *work,
                                   size_t work_bytes, const hipk_params *prm, hipk_stats *st, int64_t *block_spmvs, hipk_stream_t stream) {
    return hipk_solve_multi(0, A, dinv, k, B, ldb, X, ldx, work, work_bytes, prm, st, block_spmvs, stream);
}

extern "C" int hipk_bicgstab_solve_multi(hipk_csr_t A, const void *dinv, int k, const void *B, int64_t ldb, void *X, int64_t ldx,
                                         void *work, size_t work_bytes, const hipk_params *prm, hipk_stats *st, int64_t *block_spmvs,
                                         hipk_stream_t stream) {
    return hipk_solve_multi(1, A, dinv, k, B, ldb, X, ldx, work, work_bytes, prm, st, block_spmvs, stream);
}
