// hipk_mg_tail.h -- the device steps shared by the two one-workgroup tail kernels of the aggregation multigrid preconditioner:
// hipk_mg_tail_kernel (hipk_mg.hip, levels that are boxes) and hipk_mg_gtail_kernel (hipk_mg_graph.hip, levels whose aggregates are
// index arrays).  LV is the level descriptor, hipk_mg_level or hipk_mg_glevel (include/hipk.h): the steps read its CSR arrays,
// dinv, n and the smoother's coefficients, which both have.
//
// The rules of the batch kernels (hipk_batch.h) hold: no other workgroup exists; every barrier stands outside the loops over rows
// and is reached by all threads; a gather reads a vector that is complete in LDS behind a barrier; a row is summed in stored order,
// s = 0, s = s + a_ij x_j, which for rows of at most 32 entries is the summation order of every SpMV kernel.
//   LDS : xs[4096] of T, the gather vector (32 KiB fp64, 16 KiB fp32, static).
//   slab: per level five vectors of (n + 3) & ~3 elements -- r | z | t | d | w -- in `work`, levels back to back; level 0 reads the
//         caller's r and writes the caller's z instead of its first two.  r and z of a level wait there for the coarse correction;
//         t is the residual, d the post-smoother's output, w the Chebyshev recurrence's own vector.
// Thread t owns rows t, t + 256, ...: every element-wise step touches own rows only, and every slab element a thread reads
// outside a staging copy is one it wrote itself.  Every slab element is written before it is read: `work` need not be initialised.
#pragma once
#include "hipk_common.h"

// the tail kernels' envelope, that of the batch kernels (HIPK_BATCH_MAX_N / HIPK_BATCH_MAX_ROW in hipk_batch.h)
#define HIPK_MG_TAIL_MAX_N 4096
#define HIPK_MG_TAIL_MAX_ROW 32

#ifdef __HIPCC__
template <typename T>
struct hipk_mg_vecs {
    T *r, *z, *t, *d, *w;
};

template <typename T, typename LV>
__device__ __forceinline__ hipk_mg_vecs<T> hipk_mg_level_vecs(const LV *lv, int j, const T *rin, T *zout, T *slab) {
    int64_t off = 0;
    for (int i = 0; i < j; ++i) off += 5 * (int64_t)((lv[i].n + 3) & ~3);
    const int nvp = (lv[j].n + 3) & ~3;
    T *b = slab + off;
    hipk_mg_vecs<T> v;
    v.r = j ? b : const_cast<T *>(rin);   // level 0's r is the caller's: read only
    v.z = j ? b + nvp : zout;
    v.t = b + 2 * nvp;
    v.d = b + 3 * nvp;
    v.w = b + 4 * nvp;
    return v;
}

template <typename T, typename LV>
__device__ __forceinline__ T hipk_mg_rowsum(const LV &L, const T *xs, int row) {
    const T *__restrict__ val = (const T *)L.val;
    const int lo = L.crow[row], hi = L.crow[row + 1];
    T s = (T)0;
    for (int j = lo; j < hi; ++j) {
        const T p = val[j] * xs[L.col[j]];
        s = s + p;
    }
    return s;
}

// xs = v (own rows), complete behind the barrier
template <typename T>
__device__ __forceinline__ void hipk_mg_stage(int n, const T *v, T *xs) {
    for (int row = threadIdx.x; row < n; row += HIPK_THREADS) xs[row] = v[row];
    __syncthreads();
}

// out = b - A x
template <typename T, typename LV>
__device__ __forceinline__ void hipk_mg_residual(const LV &L, const T *x, const T *b, T *out, T *xs) {
    hipk_mg_stage(L.n, x, xs);
    for (int row = threadIdx.x; row < L.n; row += HIPK_THREADS) out[row] = b[row] - hipk_mg_rowsum<T>(L, xs, row);
    __syncthreads();
}

// z = S(r): the Chebyshev recurrence of hipk_cheb_apply with scale 1; w is its vector d
template <typename T, typename LV>
__device__ __forceinline__ void hipk_mg_smooth(const LV &L, int m, const T *r, T *z, T *w, T *xs) {
    const T *__restrict__ dinv = (const T *)L.dinv;
    const T c0 = (T)L.c0;
    for (int row = threadIdx.x; row < L.n; row += HIPK_THREADS) {
        const T d = c0 * (dinv[row] * r[row]);
        w[row] = d;
        z[row] = d;
    }
    for (int k = 0; k < m; ++k) {
        const T c1 = (T)L.c1[k], c2 = (T)L.c2[k];
        hipk_mg_stage(L.n, z, xs);
        for (int row = threadIdx.x; row < L.n; row += HIPK_THREADS) {
            const T res = dinv[row] * (r[row] - hipk_mg_rowsum<T>(L, xs, row));
            const T d = (c1 * w[row]) + (c2 * res);
            w[row] = d;
            z[row] = z[row] + d;
        }
        __syncthreads();
    }
}

// the bytes of `work` for levels of n_j unknowns: five vectors per level, rounded up to 256
template <typename LV>
static inline size_t hipk_mg_slab_bytes(const LV *lv, int nlev, int dtype) {
    size_t el = 0;
    for (int j = 0; j < nlev; ++j) el += 5 * (size_t)(((int64_t)lv[j].n + 3) & ~(int64_t)3);
    return (el * (dtype == HIPK_F64 ? 8 : 4) + 255) & ~(size_t)255;
}
#endif
