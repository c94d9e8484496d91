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

// the dense last level (hipk_mg_dense.hip): its envelope as a launch and inside a tail, and the segments of its rounding spec
#define HIPK_MG_DENSE_MAX_N 2048
#define HIPK_MG_DENSE_TAIL_N 512
#define HIPK_MG_DENSE_SEG 64
#define HIPK_MG_DENSE_BATCH 16   // loads of cinv a thread has in flight (it divides the segment)

#ifdef __HIPCC__
template <typename T>
struct hipk_mg_vecs {
    T *r, *z, *t, *d, *w;
    T *e;   // the W walk's sixth vector (NV == 6): the first visit's z, kept while the second runs
};

// NV: the vectors a level has in the slab, 5 for the V walks and 6 for the W walk
template <typename T, typename LV, int NV = 5>
__device__ __forceinline__ hipk_mg_vecs<T> hipk_mg_level_vecs(const LV *lv, int j, const T *rin, T *zout, T *slab) {
    int64_t off = 0;
    for (int i = 0; i < j; ++i) off += NV * (int64_t)((lv[i].n + 3) & ~3);
    const int nvp = (lv[j].n + 3) & ~3;
    T *b = slab + off;
    hipk_mg_vecs<T> v;
    v.r = j ? b : const_cast<T *>(rin);   // level 0's r is the caller's: read only
    v.z = j ? b + nvp : zout;
    v.t = b + 2 * nvp;
    v.d = b + 3 * nvp;
    v.w = b + 4 * nvp;
    v.e = (NV > 5) ? b + 5 * nvp : nullptr;
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

// Rows [row0, row0 + nr) of z = cinv rs by the workgroup: rs holds r, complete in LDS behind a barrier; ps takes the
// nr * ceil(n / 64) partials, p_q of row i at ps[q nr + i].  Thread t owns rows t, t + 256, ... of the block in the last step.
template <typename T>
__device__ __forceinline__ void hipk_mg_dense_rows(int n, int ld, const T *__restrict__ cinv, int row0, int nr, bool scaled, T scale, const T *rs,
                                                   T *ps, T *z) {
    const int nseg = (n + HIPK_MG_DENSE_SEG - 1) / HIPK_MG_DENSE_SEG;
    const int items = nr * nseg;
    for (int w = threadIdx.x; w < items; w += HIPK_THREADS) {
        const int q = w / nr, i = w - q * nr;
        const int j0 = q * HIPK_MG_DENSE_SEG;
        const T *__restrict__ c = cinv + (int64_t)j0 * ld + (row0 + i);
        T p = (T)0;
        if (j0 + HIPK_MG_DENSE_SEG <= n) {   // a whole segment: HIPK_MG_DENSE_BATCH loads in flight, then their sums in order
#pragma unroll 1
            for (int j = 0; j < HIPK_MG_DENSE_SEG; j += HIPK_MG_DENSE_BATCH, c += (int64_t)HIPK_MG_DENSE_BATCH * ld) {
                T a[HIPK_MG_DENSE_BATCH];
#pragma unroll
                for (int k = 0; k < HIPK_MG_DENSE_BATCH; ++k) a[k] = c[(int64_t)k * ld];
#pragma unroll
                for (int k = 0; k < HIPK_MG_DENSE_BATCH; ++k) {
                    const T prod = a[k] * rs[j0 + j + k];
                    p = p + prod;
                }
            }
        } else {
            for (int j = j0; j < n; ++j, c += ld) {
                const T prod = *c * rs[j];
                p = p + prod;
            }
        }
        ps[w] = p;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nr; i += HIPK_THREADS) {
        T s = (T)0;
        for (int q = 0; q < nseg; ++q) s = s + ps[q * nr + i];
        z[row0 + i] = scaled ? scale * s : s;
    }
}

// The walks leave and expect the last level's r and z in its slab (the caller's vectors when nlev == 1), every element written
// and read by the thread that owns its row.
// steps 1 - 3 on level j < nlev - 1: r of level j + 1 is complete behind the barrier it ends in
template <typename T, typename LV, typename XF, int NV = 5>
__device__ __forceinline__ void hipk_mg_step_down(const LV *lv, int j, int m, const T *rin, T *zout, T *slab, T *xs) {
    const LV &L = lv[j];
    const hipk_mg_vecs<T> v = hipk_mg_level_vecs<T, LV, NV>(lv, j, rin, zout, slab);
    T *rc = hipk_mg_level_vecs<T, LV, NV>(lv, j + 1, rin, zout, slab).r;
    hipk_mg_smooth<T>(L, m, v.r, v.z, v.w, xs);
    hipk_mg_residual<T>(L, v.z, v.r, v.t, xs);
    hipk_mg_stage(L.n, v.t, xs);
    XF::template restrict_to<T>(L, lv[j + 1].n, xs, rc);
    __syncthreads();
}

// down: steps 1 - 3 on levels 0 .. nlev - 2
template <typename T, typename LV, typename XF>
__device__ __forceinline__ void hipk_mg_walk_down(const LV *lv, int nlev, int m, const T *rin, T *zout, T *slab, T *xs) {
    for (int j = 0; j + 1 < nlev; ++j) hipk_mg_step_down<T, LV, XF>(lv, j, m, rin, zout, slab, xs);
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

// steps 5 - 6 on level j < nlev - 1 from z of level j + 1; no barrier behind the last loop, which touches own rows only
template <typename T, typename LV, typename XF, int NV = 5>
__device__ __forceinline__ void hipk_mg_step_up(const LV *lv, int j, int m, T omega, T scale, const T *rin, T *zout, T *slab, T *xs) {
    const LV &L = lv[j];
    const hipk_mg_vecs<T> v = hipk_mg_level_vecs<T, LV, NV>(lv, j, rin, zout, slab);
    const T *e = hipk_mg_level_vecs<T, LV, NV>(lv, j + 1, rin, zout, slab).z;
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

// up: steps 5 - 6 on levels nlev - 2 .. 0
template <typename T, typename LV, typename XF>
__device__ __forceinline__ void hipk_mg_walk_up(const LV *lv, int nlev, int m, T omega, T scale, const T *rin, T *zout, T *slab, T *xs) {
    for (int j = nlev - 2; j >= 0; --j) hipk_mg_step_up<T, LV, XF>(lv, j, m, omega, scale, rin, zout, slab, xs);
}

// The W walk (cycle = "W"): V(j, r) with step 4 done twice wherever level j + 1 is smoothed, that is j + 1 < nlev - 1:
//     e = V(j + 1, rc);  rc2 = rc - A_{j+1} e;  e2 = V(j + 1, rc2);  e = e + e2
// and once where level j + 1 is the last one.  No recursion: j is the level the workgroup stands on and bit j of `second` says
// that level j is on the second of its two visits -- both live in SGPRs, uniform across the workgroup, so every barrier is
// reached by all threads.  The slab has SIX vectors per level, r | z | t | d | w | e: when the first visit of level j ends, z is
// saved in e and rc2 OVERWRITES r (out[row] = r[row] - (A z)[row], own rows, z staged in LDS), so the second visit is the
// first one's code on the same vectors; when it ends, z = e + z.  Level 0 is visited once, so the caller's r is only read.
// `last(NV-vectors of level nlev - 1)` is the kernel's last level -- z = dinv r or the dense step --; it is entered by all threads
// with every earlier reader of xs behind a barrier, and must leave xs free in the same way.  nlev <= 2 is the V walk bit for bit.
// A level j >= 1 of nlev is visited 2^(min(j, nlev - 2)) times: the entries refuse more than HIPK_MG_TAIL_W_MAX_LEVELS levels.
template <typename T, typename LV, typename XF, typename LAST>
__device__ __forceinline__ void hipk_mg_walk_w(const LV *lv, int nlev, int m, T omega, T scale, const T *rin, T *zout, T *slab, T *xs,
                                               LAST last) {
    unsigned second = 0u;
    int j = 0;
    for (;;) {
        for (; j + 1 < nlev; ++j) hipk_mg_step_down<T, LV, XF, 6>(lv, j, m, rin, zout, slab, xs);
        last(hipk_mg_level_vecs<T, LV, 6>(lv, nlev - 1, rin, zout, slab));
        // level j is complete: up, until a smoothed level ends its first visit
        bool again = false;
        while (j > 0) {
            if (j + 1 < nlev) {
                const hipk_mg_vecs<T> v = hipk_mg_level_vecs<T, LV, 6>(lv, j, rin, zout, slab);
                if (!(second & (1u << j))) {
                    for (int row = threadIdx.x; row < lv[j].n; row += HIPK_THREADS) v.e[row] = v.z[row];
                    hipk_mg_residual<T>(lv[j], v.z, v.r, v.r, xs);
                    second |= 1u << j;
                    again = true;
                    break;
                }
                for (int row = threadIdx.x; row < lv[j].n; row += HIPK_THREADS) v.z[row] = v.e[row] + v.z[row];
                second &= ~(1u << j);
            }
            --j;
            hipk_mg_step_up<T, LV, XF, 6>(lv, j, m, omega, scale, rin, zout, slab, xs);
        }
        if (!again) break;
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

// the same for nlev box levels (hipk_mg_tail_apply and its W twin; `envelope` names the entry)
static inline int hipk_mg_tail_check(const hipk_mg_level *lv, int nlev, int degree, int dtype, const char *envelope) {
    HIPK_REQUIRE(lv && nlev >= 1 && nlev <= HIPK_MG_TAIL_MAX_LEVELS, HIPK_ERR_ARG, "1 .. 16 levels");
    HIPK_REQUIRE(degree >= 1 && degree <= 32, HIPK_ERR_ARG, "degree must be in [1, 32]");
    HIPK_REQUIRE(dtype == HIPK_F64 || dtype == HIPK_F32, HIPK_ERR_UNSUPPORTED, "dtype must be HIPK_F32 or HIPK_F64");
    for (int j = 0; j < nlev; ++j) {
        const hipk_mg_level &L = lv[j];
        HIPK_REQUIRE(L.n0 >= 1 && L.n1 >= 1 && L.n2 >= 1 && L.n >= 1 && (int64_t)L.n0 * L.n1 * L.n2 == L.n, HIPK_ERR_ARG,
                     "a level's n is not the product of its dimensions");
        HIPK_REQUIRE(L.n <= HIPK_MG_TAIL_MAX_N && L.max_row <= HIPK_MG_TAIL_MAX_ROW, HIPK_ERR_UNSUPPORTED, envelope);
        HIPK_REQUIRE(L.crow && L.col && L.val && L.dinv, HIPK_ERR_ARG, "null pointer in a level");
        if (j + 1 < nlev)
            HIPK_REQUIRE(lv[j + 1].n0 == (L.n0 + 1) / 2 && lv[j + 1].n1 == (L.n1 + 1) / 2 && lv[j + 1].n2 == (L.n2 + 1) / 2, HIPK_ERR_ARG,
                         "a level's dimensions are not ceil(d / 2) of the level above");
    }
    HIPK_REQUIRE(lv[nlev - 1].n == 1, HIPK_ERR_ARG, "the last level must have one unknown");
    return HIPK_OK;
}

// the dense last level of hipk_mg_dense_apply (max_n 2048) and of the tails that end in one (512); `envelope` names the entry
static inline int hipk_mg_dense_check(int64_t n, int64_t max_n, int64_t ld, const void *cinv, int dtype, const char *envelope) {
    HIPK_REQUIRE(dtype == HIPK_F64 || dtype == HIPK_F32, HIPK_ERR_UNSUPPORTED, "dtype must be HIPK_F32 or HIPK_F64");
    HIPK_REQUIRE(n >= 1, HIPK_ERR_ARG, "the dense level has no unknowns");
    HIPK_REQUIRE(n <= max_n, HIPK_ERR_UNSUPPORTED, envelope);
    HIPK_REQUIRE(cinv, HIPK_ERR_ARG, "null argument");
    HIPK_REQUIRE(ld >= n && ld <= INT32_MAX, HIPK_ERR_ARG, "ld >= n is required");
    HIPK_REQUIRE(ld % 4 == 0 && hipk_aligned16(cinv), HIPK_ERR_ALIGN, "cinv must be 16-byte aligned and ld a multiple of 4");
    return HIPK_OK;
}

// the W entries (hipk_mg_w.hip) take fewer levels: the last one of nlev is visited 2^(nlev - 2) times in one launch
#define HIPK_MG_TAIL_W_MAX_LEVELS 12

// the bytes of `work` for levels of n_j unknowns: `nv` vectors per level -- five, six for the W walk --, rounded up to 256; 0 for
// bad arguments
template <typename LV>
static inline size_t hipk_mg_work_bytes(const LV *lv, int nlev, int max_levels, int dtype, int nv = 5) {
    if (!lv || nlev < 1 || nlev > max_levels) return 0;
    size_t el = 0;
    for (int j = 0; j < nlev; ++j) el += (size_t)nv * (size_t)(((int64_t)lv[j].n + 3) & ~(int64_t)3);
    return (el * (dtype == HIPK_F64 ? 8 : 4) + 255) & ~(size_t)255;
}

// What every tail entry point does once its levels are checked (nlev in [1, max_levels], dtype valid): the checks of the
// caller's pointers, then launch(T()) with T = double or float, which starts the one workgroup of the entry's kernel<T>.
template <typename LV, typename F>
static inline int hipk_mg_tail_launch(const LV *levels_host, const void *levels_dev, int nlev, int max_levels, const void *r, void *z, int dtype,
                                      void *work, size_t work_bytes, F launch, int nv = 5) {
    HIPK_REQUIRE(levels_dev && r && z && work, HIPK_ERR_ARG, "null argument");
    HIPK_REQUIRE(hipk_aligned16(r) && hipk_aligned16(z) && hipk_aligned16(levels_dev) && (((uintptr_t)work) & 255u) == 0, HIPK_ERR_ALIGN,
                 "r, z and the level blob must be 16-byte aligned, work 256-byte aligned");
    HIPK_REQUIRE(r != z, HIPK_ERR_ARG, "r and z must be distinct");
    HIPK_REQUIRE(work_bytes >= hipk_mg_work_bytes(levels_host, nlev, max_levels, dtype, nv), HIPK_ERR_WORKSPACE, "work buffer too small");
    if (dtype == HIPK_F64)
        launch(double());
    else
        launch(float());
    HIPK_CHECK_HIP(hipGetLastError());
    return HIPK_OK;
}
