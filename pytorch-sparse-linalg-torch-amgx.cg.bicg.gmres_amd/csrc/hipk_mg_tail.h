// hipk_mg_tail.h -- the one-workgroup tail of the aggregation multigrid preconditioner: the device steps, the walk down and up the
// levels and the host side that the three tail kernels share -- hipk_mg_tail_kernel (hipk_mg.hip, levels that are boxes),
// hipk_mg_gtail_kernel (hipk_mg_graph.hip, levels whose aggregates are index arrays) and hipk_mg_gtail_dense_kernel
// (hipk_mg_dense.hip, the same with a dense last level).  LV is the level descriptor, hipk_mg_level or hipk_mg_glevel
// (include/hipk.h): the steps read its CSR arrays, dinv, n and the smoother's coefficients, which both have.  XF is the transfer
// policy of LV, hipk_mg_box_xf or hipk_mg_index_xf: it alone knows the members of an aggregate and the aggregate of a row.
//
// The rules of the batch kernels (hipk_batch.h) hold: no other workgroup exists; every barrier stands outside the loops over rows
// and is reached by all threads; a gather reads a vector that is complete in LDS behind a barrier; a row is summed in stored order,
// s = 0, s = s + a_ij x_j, which for rows of at most 32 entries is the summation order of every SpMV kernel.
//   LDS : xs[4096] of T, the gather vector (32 KiB fp64, 16 KiB fp32, static).
//   slab: per level five vectors of (n + 3) & ~3 elements -- r | z | t | d | w -- in `work`, levels back to back; level 0 reads the
//         caller's r and writes the caller's z instead of its first two.  r and z of a level wait there for the coarse correction;
//         t is the residual, d the post-smoother's output, w the Chebyshev recurrence's own vector.
// Thread t owns rows t, t + 256, ... and, of the coarse level, aggregates t, t + 256, ...: every element-wise step touches own rows
// only, rc[I] is written by the thread that reads it next, and every slab element a thread reads outside a staging copy is one it
// wrote itself.  Every slab element is written before it is read: `work` need not be initialised.
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

// The transfer policies.  restrict_to: rc[I] = the sum of the staged xs over the members of aggregate I of level L in ascending
// fine index, the first member starting the sum, for the thread's own I = t, t + 256, ... < nc.  prolong_add: z[row] = z[row] +
// (omega * xs[the aggregate of row]) over the staged coarse xs, for the thread's own rows.  Neither holds a barrier: the walks do.
struct hipk_mg_box_xf {   // a box of n0 x n1 x n2 points: every index follows from the dimensions (hipk_mg.hip)
    template <typename T>
    static __device__ __forceinline__ void restrict_to(const hipk_mg_level &L, int nc, const T *xs, T *rc) {
        const int n0 = L.n0, n1 = L.n1, n2 = L.n2, m1 = (n1 + 1) >> 1, m2 = (n2 + 1) >> 1;
        for (int I = threadIdx.x; I < nc; I += HIPK_THREADS) {
            const int I2 = I % m2, q = I / m2, I1 = q % m1, I0 = q / m1;
            const bool has2 = 2 * I2 + 1 < n2;
            T s = (T)0;
#pragma unroll
            for (int d0 = 0; d0 < 2; ++d0) {
#pragma unroll
                for (int d1 = 0; d1 < 2; ++d1) {
                    const int i0 = 2 * I0 + d0, i1 = 2 * I1 + d1;
                    if (i0 < n0 && i1 < n1) {
                        const int f = (i0 * n1 + i1) * n2 + 2 * I2;
                        s = (d0 == 0 && d1 == 0) ? xs[f] : s + xs[f];
                        if (has2) s = s + xs[f + 1];
                    }
                }
            }
            rc[I] = s;
        }
    }
    template <typename T>
    static __device__ __forceinline__ void prolong_add(const hipk_mg_level &L, const T *xs, T omega, T *z) {
        const int n1 = L.n1, n2 = L.n2, m1 = (n1 + 1) >> 1, m2 = (n2 + 1) >> 1;
        for (int row = threadIdx.x; row < L.n; row += HIPK_THREADS) {
            const int i2 = row % n2, q = row / n2, i1 = q % n1, i0 = q / n1;
            z[row] = z[row] + (omega * xs[((i0 >> 1) * m1 + (i1 >> 1)) * m2 + (i2 >> 1)]);
        }
    }
};

struct hipk_mg_index_xf {   // index arrays: amem[aptr[I] .. aptr[I + 1]) the members of aggregate I, agg[row] the aggregate of a row
    template <typename T>
    static __device__ __forceinline__ void restrict_to(const hipk_mg_glevel &L, int nc, const T *xs, T *rc) {
        for (int I = threadIdx.x; I < nc; I += HIPK_THREADS) {
            const int lo = L.aptr[I], hi = L.aptr[I + 1];
            T s = xs[L.amem[lo]];
            for (int k = lo + 1; k < hi; ++k) s = s + xs[L.amem[k]];
            rc[I] = s;
        }
    }
    template <typename T>
    static __device__ __forceinline__ void prolong_add(const hipk_mg_glevel &L, const T *xs, T omega, T *z) {
        for (int row = threadIdx.x; row < L.n; row += HIPK_THREADS) z[row] = z[row] + (omega * xs[L.agg[row]]);
    }
};

// The walks leave and expect the last level's r and z in its slab (the caller's vectors when nlev == 1), every element written
// and read by the thread that owns its row.
// down: steps 1 - 3 on levels 0 .. nlev - 2
template <typename T, typename LV, typename XF>
__device__ __forceinline__ void hipk_mg_walk_down(const LV *lv, int nlev, int m, const T *rin, T *zout, T *slab, T *xs) {
    for (int j = 0; j + 1 < nlev; ++j) {
        const LV &L = lv[j];
        const hipk_mg_vecs<T> v = hipk_mg_level_vecs<T>(lv, j, rin, zout, slab);
        T *rc = hipk_mg_level_vecs<T>(lv, j + 1, rin, zout, slab).r;
        hipk_mg_smooth<T>(L, m, v.r, v.z, v.w, xs);
        hipk_mg_residual<T>(L, v.z, v.r, v.t, xs);
        hipk_mg_stage(L.n, v.t, xs);
        XF::template restrict_to<T>(L, lv[j + 1].n, xs, rc);
        __syncthreads();
    }
}

// the last level where no off-diagonal entry is left: z = dinv r on any number of rows
template <typename T, typename LV>
__device__ __forceinline__ void hipk_mg_last_diag(const LV *lv, int nlev, T scale, const T *rin, T *zout, T *slab) {
    const hipk_mg_vecs<T> v = hipk_mg_level_vecs<T>(lv, nlev - 1, rin, zout, slab);
    const T *__restrict__ dinv = (const T *)lv[nlev - 1].dinv;
    for (int row = threadIdx.x; row < lv[nlev - 1].n; row += HIPK_THREADS) {
        const T zz = dinv[row] * v.r[row];
        v.z[row] = (nlev == 1) ? scale * zz : zz;
    }
}

// up: steps 5 - 6 on levels nlev - 2 .. 0
template <typename T, typename LV, typename XF>
__device__ __forceinline__ void hipk_mg_walk_up(const LV *lv, int nlev, int m, T omega, T scale, const T *rin, T *zout, T *slab, T *xs) {
    for (int j = nlev - 2; j >= 0; --j) {
        const LV &L = lv[j];
        const hipk_mg_vecs<T> v = hipk_mg_level_vecs<T>(lv, j, rin, zout, slab);
        const T *e = hipk_mg_level_vecs<T>(lv, j + 1, rin, zout, slab).z;
        hipk_mg_stage(lv[j + 1].n, e, xs);
        XF::template prolong_add<T>(L, xs, omega, v.z);
        __syncthreads();
        hipk_mg_residual<T>(L, v.z, v.r, v.t, xs);
        hipk_mg_smooth<T>(L, m, v.t, v.d, v.w, xs);
        for (int row = threadIdx.x; row < L.n; row += HIPK_THREADS) {
            const T zz = v.z[row] + v.d[row];
            v.z[row] = (j == 0) ? scale * zz : zz;
        }
    }
}
#endif

// ------------------------------------------------------------------------------------------------------------- the host side
// the level counts the entry points take: hipk_mg_tail_apply, and the two over index-array levels
#define HIPK_MG_TAIL_MAX_LEVELS 16
#define HIPK_MG_GTAIL_MAX_LEVELS 32

// The checks of an entry over nlev index-array levels before it looks at the caller's vectors: the count (`too_many` names the
// entry), degree and dtype, then for levels [0, nsparse) -- those that are smoothed or end in z = dinv r -- the envelope
// (`envelope` names the entry) and the pointers.
static inline int hipk_mg_gtail_check(const hipk_mg_glevel *lv, int nsparse, int nlev, int degree, int dtype, const char *too_many,
                                      const char *envelope) {
    HIPK_REQUIRE(lv && nlev >= 1, HIPK_ERR_ARG, "at least one level");
    HIPK_REQUIRE(nlev <= HIPK_MG_GTAIL_MAX_LEVELS, HIPK_ERR_UNSUPPORTED, too_many);
    HIPK_REQUIRE(degree >= 1 && degree <= 32, HIPK_ERR_ARG, "degree must be in [1, 32]");
    HIPK_REQUIRE(dtype == HIPK_F64 || dtype == HIPK_F32, HIPK_ERR_UNSUPPORTED, "dtype must be HIPK_F32 or HIPK_F64");
    for (int j = 0; j < nsparse; ++j) {
        const hipk_mg_glevel &L = lv[j];
        HIPK_REQUIRE(L.n >= 1, HIPK_ERR_ARG, "a level has no unknowns");
        HIPK_REQUIRE(L.n <= HIPK_MG_TAIL_MAX_N && L.max_row <= HIPK_MG_TAIL_MAX_ROW, HIPK_ERR_UNSUPPORTED, envelope);
        HIPK_REQUIRE(L.crow && L.col && L.val && L.dinv, HIPK_ERR_ARG, "null pointer in a level");
        if (j + 1 < nlev) {
            HIPK_REQUIRE(L.agg && L.aptr && L.amem, HIPK_ERR_ARG, "null index array in a level that has a next one");
            HIPK_REQUIRE(lv[j + 1].n <= L.n, HIPK_ERR_ARG, "a level has more unknowns than the level above");
        }
    }
    return HIPK_OK;
}

// the bytes of `work` for levels of n_j unknowns: five vectors per level, rounded up to 256; 0 for bad arguments
template <typename LV>
static inline size_t hipk_mg_work_bytes(const LV *lv, int nlev, int max_levels, int dtype) {
    if (!lv || nlev < 1 || nlev > max_levels) return 0;
    size_t el = 0;
    for (int j = 0; j < nlev; ++j) el += 5 * (size_t)(((int64_t)lv[j].n + 3) & ~(int64_t)3);
    return (el * (dtype == HIPK_F64 ? 8 : 4) + 255) & ~(size_t)255;
}

// What every tail entry point does once its levels are checked (nlev in [1, max_levels], dtype valid): the checks of the
// caller's pointers, then launch(T()) with T = double or float, which starts the one workgroup of the entry's kernel<T>.
template <typename LV, typename F>
static inline int hipk_mg_tail_launch(const LV *levels_host, const void *levels_dev, int nlev, int max_levels, const void *r, void *z, int dtype,
                                      void *work, size_t work_bytes, F launch) {
    HIPK_REQUIRE(levels_dev && r && z && work, HIPK_ERR_ARG, "null argument");
    HIPK_REQUIRE(hipk_aligned16(r) && hipk_aligned16(z) && hipk_aligned16(levels_dev) && (((uintptr_t)work) & 255u) == 0, HIPK_ERR_ALIGN,
                 "r, z and the level blob must be 16-byte aligned, work 256-byte aligned");
    HIPK_REQUIRE(r != z, HIPK_ERR_ARG, "r and z must be distinct");
    HIPK_REQUIRE(work_bytes >= hipk_mg_work_bytes(levels_host, nlev, max_levels, dtype), HIPK_ERR_WORKSPACE, "work buffer too small");
    if (dtype == HIPK_F64)
        launch(double());
    else
        launch(float());
    HIPK_CHECK_HIP(hipGetLastError());
    return HIPK_OK;
}
