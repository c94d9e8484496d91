// hipk_mg_dense.hip -- the dense coarsest level of the aggregation multigrid preconditioner on a matrix graph (include/hipk.h,
// "aggregation multigrid: a dense coarsest level"; `AggregationMultigridPreconditioner.from_graph(coarse_rows=K)` of
// module_a/multigrid.py drives it): z = cinv r for the stored inverse of the last level's matrix, as a launch of its own and as
// the last level of the one-workgroup tail.
//
// cinv is n x n of the storage dtype, column by column: element (i, j) at cinv[j ld + i], ld >= n a multiple of 4; the padding
// rows are never read.  The rounding spec, in segments of 64 columns:
//     p_q = 0;  p_q = p_q + (cinv[i, j] * r[j])  for j = 64 q .. min(64 q + 64, n) - 1 ascending
//     s   = 0;  s   = s + p_q                    for q ascending
//     z[i] = s                                   (scale * s on level 0)
// one rounding per operation, no fma (the file is built with -ffp-contract=off).  A work item is (segment q, row i); the items of
// a block of rows are dealt to the threads row fastest, so for a fixed column consecutive lanes read consecutive rows.  r is
// staged in LDS, the p_q meet in LDS behind a barrier and the thread that owns row i adds them in ascending q.  No atomics, no
// hand-off between workgroups; nothing at or beyond n is read or written in r and z.
#include "hipk_common.h"
#include "hipk_mg_tail.h"

// z = scale * (cinv r): a workgroup owns 128 bytes of every column (16 rows fp64, 32 fp32), so a 2048-row fp64 inverse (32 MB) is
// read by 128 workgroups, each line once.
template <typename T>
__global__ __launch_bounds__(HIPK_THREADS) void hipk_mg_dense_kernel(int n, int ld, const T *__restrict__ cinv, T scale, const T *__restrict__ r,
                                                                     T *__restrict__ z) {
    constexpr int RB = 128 / (int)sizeof(T);
    __shared__ T rs[HIPK_MG_DENSE_MAX_N];
    __shared__ T ps[RB * (HIPK_MG_DENSE_MAX_N / HIPK_MG_DENSE_SEG)];
    hipk_mg_stage(n, r, rs);
    const int row0 = blockIdx.x * RB;
    hipk_mg_dense_rows<T>(n, ld, cinv, row0, min(RB, n - row0), true, scale, rs, ps, z);
}

// hipk_mg_gtail_kernel (hipk_mg_graph.hip) with a dense last level of at most 512 rows: the same walks, and between them all 256
// threads on the rows x segments of z = cinv r.  The partials take the gather vector xs (512 rows x 8 segments fill it), r of
// the last level its own 512 elements of LDS; the barrier behind the step frees xs for the way up.
template <typename T>
__global__ __launch_bounds__(HIPK_THREADS) void hipk_mg_gtail_dense_kernel(const hipk_mg_glevel *__restrict__ lv, int nlev, int m, T omega, T scale,
                                                                           const T *__restrict__ cinv, int ld, const T *rin, T *zout, T *slab) {
    __shared__ T xs[HIPK_MG_TAIL_MAX_N];
    __shared__ T rs[HIPK_MG_DENSE_TAIL_N];
    static_assert(HIPK_MG_DENSE_TAIL_N * (HIPK_MG_DENSE_TAIL_N / HIPK_MG_DENSE_SEG) <= HIPK_MG_TAIL_MAX_N, "the partials must fit xs");
    hipk_mg_walk_down<T, hipk_mg_glevel, hipk_mg_index_xf>(lv, nlev, m, rin, zout, slab, xs);
    {
        const int n = lv[nlev - 1].n;
        const hipk_mg_vecs<T> v = hipk_mg_level_vecs<T>(lv, nlev - 1, rin, zout, slab);
        hipk_mg_stage(n, v.r, rs);
        hipk_mg_dense_rows<T>(n, ld, cinv, 0, n, nlev == 1, scale, rs, xs, v.z);
        __syncthreads();
    }
    hipk_mg_walk_up<T, hipk_mg_glevel, hipk_mg_index_xf>(lv, nlev, m, omega, scale, rin, zout, slab, xs);
}

extern "C" int hipk_mg_dense_apply(int64_t n, int64_t ld, const void *cinv, double scale, const void *r, void *z, int dtype, hipk_stream_t stream) {
    HIPK_TRY(hipk_mg_dense_check(n, HIPK_MG_DENSE_MAX_N, ld, cinv, dtype, "hipk_mg_dense_apply takes at most 2048 unknowns"));
    HIPK_REQUIRE(r && z, HIPK_ERR_ARG, "null argument");
    HIPK_REQUIRE(hipk_aligned16(r) && hipk_aligned16(z), HIPK_ERR_ALIGN, "r and z must be 16-byte aligned");
    HIPK_REQUIRE(r != z, HIPK_ERR_ARG, "r and z must be distinct");
    if (dtype == HIPK_F64) {
        const int rb = 128 / (int)sizeof(double);
        hipk_mg_dense_kernel<double><<<((int)n + rb - 1) / rb, HIPK_THREADS, 0, (hipStream_t)stream>>>((int)n, (int)ld, (const double *)cinv, scale,
                                                                                                     (const double *)r, (double *)z);
    } else {
        const int rb = 128 / (int)sizeof(float);
        hipk_mg_dense_kernel<float><<<((int)n + rb - 1) / rb, HIPK_THREADS, 0, (hipStream_t)stream>>>((int)n, (int)ld, (const float *)cinv, (float)scale,
                                                                                                    (const float *)r, (float *)z);
    }
    HIPK_CHECK_HIP(hipGetLastError());
    return HIPK_OK;
}

extern "C" size_t hipk_mg_gtail_dense_work_bytes(const hipk_mg_glevel *levels_host, int nlev, int dtype) {
    return hipk_mg_work_bytes(levels_host, nlev, HIPK_MG_GTAIL_MAX_LEVELS, dtype);
}

extern "C" int hipk_mg_gtail_dense_apply(const hipk_mg_glevel *levels_host, const void *levels_dev, int nlev, int degree, double omega, double scale,
                                         const void *cinv, int64_t ld, const void *r, void *z, int dtype, void *work, size_t work_bytes,
                                         hipk_stream_t stream) {
    HIPK_TRY(hipk_mg_gtail_check(levels_host, nlev - 1, nlev, degree, dtype, "hipk_mg_gtail_dense_apply takes at most 32 levels",
                                 "hipk_mg_gtail_dense_apply takes sparse levels of at most 4096 unknowns and 32 stored entries per row"));
    HIPK_TRY(hipk_mg_dense_check(levels_host[nlev - 1].n, HIPK_MG_DENSE_TAIL_N, ld, cinv, dtype,
                                 "hipk_mg_gtail_dense_apply takes a dense level of at most 512 unknowns"));
    return hipk_mg_tail_launch(levels_host, levels_dev, nlev, HIPK_MG_GTAIL_MAX_LEVELS, r, z, dtype, work, work_bytes, [&](auto tag) {
        typedef decltype(tag) T;
        hipk_mg_gtail_dense_kernel<T><<<1, HIPK_THREADS, 0, (hipStream_t)stream>>>((const hipk_mg_glevel *)levels_dev, nlev, degree, (T)omega, (T)scale,
                                                                                   (const T *)cinv, (int)ld, (const T *)r, (T *)z, (T *)work);
    });
}
