// hipk_mg_graph.hip -- the transfer and tail kernels of the aggregation multigrid preconditioner for levels whose aggregates are
// index arrays (include/hipk.h, "aggregation multigrid on a matrix graph"; `AggregationMultigridPreconditioner.from_graph` of
// module_a/multigrid.py drives them).  hipk_mg.hip is the form for boxes, where every index follows from the dimensions.
//
// A fine level of n rows and a coarse one of nc are linked by int32 arrays: agg[i] the aggregate of row i; amem[aptr[I] ..
// aptr[I + 1]) the members of aggregate I in ascending fine index.  As in hipk_mg.hip every streaming kernel walks the vector it
// WRITES in the library's chunk form (hipk_blas1.h: a reduction chunk of the vector's own geometry per workgroup, hipk_xcd_chunk
// placing the k-th eighth of the chunks on XCD k) in 16-byte groups; only the group that holds the last element may be ragged.
// The reads of the OTHER level are gathers through the index arrays -- aggregates are built from graph neighbours, so for a
// matrix in a banded order the members of consecutive aggregates are near each other, but nothing is assumed.  Elements at and
// beyond a vector's length are never read or written.  One rounding per operation, no fma (the file is built with
// -ffp-contract=off), no atomics, no hand-off between workgroups.
#include "hipk_blas1.h"
#include "hipk_common.h"
#include "hipk_mg_tail.h"

// rc[I] = t[first member], then + t[member] over the others in ascending fine index.  A thread owns VEC consecutive aggregates:
// their member lists are one contiguous run of amem.
template <typename T>
__global__ __launch_bounds__(HIPK_THREADS) void hipk_mg_restrict_agg_kernel(int64_t nc, int ch, int ng, const int32_t *__restrict__ aptr,
                                                                            const int32_t *__restrict__ amem, const T *__restrict__ t,
                                                                            T *__restrict__ rc) {
    constexpr int VEC = hipk_vec<T>::VEC;
    const int c = hipk_xcd_chunk(blockIdx.x, ng);
    if (c < 0) return;
    hipk_chunk_loop<T, 1>(nc, ch, c, [&](int64_t I, int nv) {
        T acc[VEC];
        int lo = aptr[I];
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            acc[k] = (T)0;
            if (k < nv) {
                const int hi = aptr[I + k + 1];
                T s = t[amem[lo]];
                for (int j = lo + 1; j < hi; ++j) s = s + t[amem[j]];
                acc[k] = s;
                lo = hi;
            }
        }
        hipk_st<T>(rc, I, nv, acc);
    });
}

// z[i] = z[i] + (omega * e[agg[i]]).  A thread owns VEC consecutive fine elements and reads their VEC aggregates in one load.
template <typename T>
__global__ __launch_bounds__(HIPK_THREADS) void hipk_mg_prolong_add_agg_kernel(int64_t n, int ch, int ng, const int32_t *__restrict__ agg, T omega,
                                                                               const T *__restrict__ e, T *__restrict__ z) {
    constexpr int VEC = hipk_vec<T>::VEC;
    typedef int32_t ivec __attribute__((ext_vector_type(VEC)));
    const int c = hipk_xcd_chunk(blockIdx.x, ng);
    if (c < 0) return;
    hipk_chunk_loop<T, 1>(n, ch, c, [&](int64_t i, int nv) {
        T zv[VEC];
        int32_t a[VEC];
        hipk_ld<T>(z, i, nv, zv);
        if (nv == VEC) {   // i is a multiple of VEC and agg 16-byte aligned: an aligned 8- or 16-byte load
            const ivec av = *reinterpret_cast<const ivec *>(agg + i);
#pragma unroll
            for (int k = 0; k < VEC; ++k) a[k] = av[k];
        } else {
#pragma unroll
            for (int k = 0; k < VEC; ++k) a[k] = (k < nv) ? agg[i + k] : 0;
        }
#pragma unroll
        for (int k = 0; k < VEC; ++k)
            if (k < nv) zv[k] = zv[k] + (omega * e[a[k]]);
        hipk_st<T>(z, i, nv, zv);
    });
}

static int hipk_mg_agg_check(int64_t n, int64_t nc, const void *i0, const void *i1, const void *a, const void *b, int dtype) {
    HIPK_REQUIRE(i0 && i1 && a && b, HIPK_ERR_ARG, "null argument");
    HIPK_REQUIRE(nc >= 1 && nc <= n && n <= INT32_MAX, HIPK_ERR_ARG, "1 <= nc <= n < 2^31 is required");
    HIPK_REQUIRE(dtype == HIPK_F64 || dtype == HIPK_F32, HIPK_ERR_UNSUPPORTED, "dtype must be HIPK_F32 or HIPK_F64");
    HIPK_REQUIRE(hipk_aligned16(i0) && hipk_aligned16(i1) && hipk_aligned16(a) && hipk_aligned16(b), HIPK_ERR_ALIGN,
                 "vectors and index arrays must be 16-byte aligned");
    HIPK_REQUIRE(a != b, HIPK_ERR_ARG, "the two vectors must be distinct");
    return HIPK_OK;
}

extern "C" int hipk_mg_restrict_agg(int64_t n, int64_t nc, const int32_t *aptr, const int32_t *amem, const void *t, void *rc, int dtype,
                                    hipk_stream_t stream) {
    HIPK_TRY(hipk_mg_agg_check(n, nc, aptr, amem, t, rc, dtype));
    const hipk_geom gm = hipk_make_geom(nc);   // the coarse vector's chunks
    if (dtype == HIPK_F64)
        hipk_mg_restrict_agg_kernel<double><<<hipk_xcd_grid(gm.g), HIPK_THREADS, 0, (hipStream_t)stream>>>(nc, gm.ch, gm.g, aptr, amem, (const double *)t,
                                                                                                         (double *)rc);
    else
        hipk_mg_restrict_agg_kernel<float><<<hipk_xcd_grid(gm.g), HIPK_THREADS, 0, (hipStream_t)stream>>>(nc, gm.ch, gm.g, aptr, amem, (const float *)t,
                                                                                                        (float *)rc);
    HIPK_CHECK_HIP(hipGetLastError());
    return HIPK_OK;
}

extern "C" int hipk_mg_prolong_add_agg(int64_t n, int64_t nc, const int32_t *agg, double omega, const void *e, void *z, int dtype,
                                       hipk_stream_t stream) {
    HIPK_TRY(hipk_mg_agg_check(n, nc, agg, agg, e, z, dtype));
    const hipk_geom gm = hipk_make_geom(n);
    if (dtype == HIPK_F64)
        hipk_mg_prolong_add_agg_kernel<double><<<hipk_xcd_grid(gm.g), HIPK_THREADS, 0, (hipStream_t)stream>>>(n, gm.ch, gm.g, agg, omega, (const double *)e,
                                                                                                            (double *)z);
    else
        hipk_mg_prolong_add_agg_kernel<float><<<hipk_xcd_grid(gm.g), HIPK_THREADS, 0, (hipStream_t)stream>>>(n, gm.ch, gm.g, agg, (float)omega,
                                                                                                           (const float *)e, (float *)z);
    HIPK_CHECK_HIP(hipGetLastError());
    return HIPK_OK;
}

// ------------------------------------------------------------------------------------------------------------- the tail kernel
// hipk_mg_tail_kernel (hipk_mg.hip) for index-array levels: one launch, ONE 256-thread workgroup walks levels j = 0 .. nlev - 1 down
// and back up with the steps, the walks, the slab and the rules of hipk_mg_tail.h; the two transfers are its hipk_mg_index_xf.
// The last level is z = dinv r on any number of rows.  Bit for bit the launch sequence's result.
template <typename T>
__global__ __launch_bounds__(HIPK_THREADS) void hipk_mg_gtail_kernel(const hipk_mg_glevel *__restrict__ lv, int nlev, int m, T omega, T scale,
                                                                     const T *rin, T *zout, T *slab) {
    __shared__ T xs[HIPK_MG_TAIL_MAX_N];
    hipk_mg_walk_down<T, hipk_mg_glevel, hipk_mg_index_xf>(lv, nlev, m, rin, zout, slab, xs);
    hipk_mg_last_diag<T>(lv, nlev, scale, rin, zout, slab);
    hipk_mg_walk_up<T, hipk_mg_glevel, hipk_mg_index_xf>(lv, nlev, m, omega, scale, rin, zout, slab, xs);
}

extern "C" size_t hipk_mg_gtail_work_bytes(const hipk_mg_glevel *levels_host, int nlev, int dtype) {
    return hipk_mg_work_bytes(levels_host, nlev, HIPK_MG_GTAIL_MAX_LEVELS, dtype);
}

extern "C" int hipk_mg_gtail_apply(const hipk_mg_glevel *levels_host, const void *levels_dev, int nlev, int degree, double omega,
                                   double scale, const void *r, void *z, int dtype, void *work, size_t work_bytes, hipk_stream_t stream) {
    HIPK_TRY(hipk_mg_gtail_check(levels_host, nlev, nlev, degree, dtype, "hipk_mg_gtail_apply takes at most 32 levels",
                                 "hipk_mg_gtail_apply takes levels of at most 4096 unknowns and 32 stored entries per row"));
    return hipk_mg_tail_launch(levels_host, levels_dev, nlev, HIPK_MG_GTAIL_MAX_LEVELS, r, z, dtype, work, work_bytes, [&](auto tag) {
        typedef decltype(tag) T;
        hipk_mg_gtail_kernel<T><<<1, HIPK_THREADS, 0, (hipStream_t)stream>>>((const hipk_mg_glevel *)levels_dev, nlev, degree, (T)omega, (T)scale,
                                                                             (const T *)r, (T *)z, (T *)work);
    });
}
