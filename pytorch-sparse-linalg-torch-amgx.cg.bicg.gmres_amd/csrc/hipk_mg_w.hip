// hipk_mg_w.hip -- the W-cycle of the aggregation multigrid preconditioner (include/hipk.h, "aggregation multigrid: the W-cycle";
// `AggregationMultigridPreconditioner(cycle="W")` of module_a/multigrid.py drives it): the element-wise sum of the two coarse
// corrections, and the W twins of the three one-workgroup tail kernels.
//
// W(l, r) is V(l, r) with step 4 done twice where level l + 1 is smoothed:
//     e = W(l + 1, rc);  rc2 = rc - A_{l+1} e;  e2 = W(l + 1, rc2);  e = e + e2
// and once where level l + 1 is the last level (z = dinv r or the dense step, exact or diagonal).  A level l is then visited
// 2^l times per apply -- as launches that is launch overhead only --, so each tail kernel runs its whole W sub-walk in ONE launch
// of one workgroup: hipk_mg_walk_w of hipk_mg_tail.h, iterative, over the steps the V walks are made of, with six vectors per
// level in the slab.  The kernels live here and not beside their V twins so that those translation units keep exactly their
// kernels.  One rounding per operation, no fma (the file is built with -ffp-contract=off).
#include "hipk_blas1.h"
#include "hipk_common.h"
#include "hipk_mg_tail.h"

// e = e + e2: step 4c, in the chunk form of hipk_mg_correct_kernel
template <typename T>
__global__ __launch_bounds__(HIPK_THREADS) void hipk_mg_add_kernel(int64_t n, int ch, int ng, const T *__restrict__ e2, T *__restrict__ e) {
    constexpr int VEC = hipk_vec<T>::VEC;
    const int c = hipk_xcd_chunk(blockIdx.x, ng);
    if (c < 0) return;
    hipk_chunk_loop<T>(n, ch, c, [&](int64_t i, int nv) {
        T ev[VEC], dv[VEC];
        hipk_ld<T>(e, i, nv, ev);
        hipk_ld<T>(e2, i, nv, dv);
#pragma unroll
        for (int k = 0; k < VEC; ++k) ev[k] = ev[k] + dv[k];
        hipk_st<T>(e, i, nv, ev);
    });
}

extern "C" int hipk_mg_add(int64_t n, const void *e2, void *e, int dtype, hipk_stream_t stream) {
    HIPK_REQUIRE(n >= 1, HIPK_ERR_ARG, "n must be at least 1");
    HIPK_REQUIRE(e2 && e, HIPK_ERR_ARG, "null argument");
    HIPK_REQUIRE(dtype == HIPK_F64 || dtype == HIPK_F32, HIPK_ERR_UNSUPPORTED, "dtype must be HIPK_F32 or HIPK_F64");
    HIPK_REQUIRE(hipk_aligned16(e2) && hipk_aligned16(e), HIPK_ERR_ALIGN, "vectors must be 16-byte aligned");
    HIPK_REQUIRE(e2 != e, HIPK_ERR_ARG, "the two vectors must be distinct");
    const hipk_geom gm = hipk_make_geom(n);
    if (dtype == HIPK_F64)
        hipk_mg_add_kernel<double><<<hipk_xcd_grid(gm.g), HIPK_THREADS, 0, (hipStream_t)stream>>>(n, gm.ch, gm.g, (const double *)e2, (double *)e);
    else
        hipk_mg_add_kernel<float><<<hipk_xcd_grid(gm.g), HIPK_THREADS, 0, (hipStream_t)stream>>>(n, gm.ch, gm.g, (const float *)e2, (float *)e);
    HIPK_CHECK_HIP(hipGetLastError());
    return HIPK_OK;
}

// ------------------------------------------------------------------------------------------------------------- the tail kernels
// hipk_mg_tail_kernel / hipk_mg_gtail_kernel with the W walk: XF is the transfer policy of the level descriptor LV, the last level
// is z = dinv r.  Bit for bit the W launch sequence's result.
template <typename T, typename LV, typename XF>
__global__ __launch_bounds__(HIPK_THREADS) void hipk_mg_tail_w_kernel(const LV *__restrict__ lv, int nlev, int m, T omega, T scale, const T *rin,
                                                                      T *zout, T *slab) {
    __shared__ T xs[HIPK_MG_TAIL_MAX_N];
    hipk_mg_walk_w<T, LV, XF>(lv, nlev, m, omega, scale, rin, zout, slab, xs, [&](const hipk_mg_vecs<T> &v) {
        const T *__restrict__ dinv = (const T *)lv[nlev - 1].dinv;
        for (int row = threadIdx.x; row < lv[nlev - 1].n; row += HIPK_THREADS) {   // own rows: no barrier
            const T zz = dinv[row] * v.r[row];
            v.z[row] = (nlev == 1) ? scale * zz : zz;
        }
    });
}

// hipk_mg_gtail_dense_kernel with the W walk: the dense step is entered once per visit of level nlev - 2.  Its partials take xs,
// which the barrier behind it frees; rs is written again only behind that barrier.
template <typename T>
__global__ __launch_bounds__(HIPK_THREADS) void hipk_mg_gtail_dense_w_kernel(const hipk_mg_glevel *__restrict__ lv, int nlev, int m, T omega, T scale,
                                                                             const T *__restrict__ cinv, int ld, const T *rin, T *zout, T *slab) {
    __shared__ T xs[HIPK_MG_TAIL_MAX_N];
    __shared__ T rs[HIPK_MG_DENSE_TAIL_N];
    static_assert(HIPK_MG_DENSE_TAIL_N * (HIPK_MG_DENSE_TAIL_N / HIPK_MG_DENSE_SEG) <= HIPK_MG_TAIL_MAX_N, "the partials must fit xs");
    hipk_mg_walk_w<T, hipk_mg_glevel, hipk_mg_index_xf>(lv, nlev, m, omega, scale, rin, zout, slab, xs, [&](const hipk_mg_vecs<T> &v) {
        const int n = lv[nlev - 1].n;
        hipk_mg_stage(n, v.r, rs);
        hipk_mg_dense_rows<T>(n, ld, cinv, 0, n, nlev == 1, scale, rs, xs, v.z);
        __syncthreads();
    });
}

#define HIPK_MG_W_TOO_MANY "a W tail takes at most 12 levels: the last of them is visited 2^(nlev - 2) times in one launch"

extern "C" size_t hipk_mg_tail_work_bytes_w(const hipk_mg_level *levels_host, int nlev, int dtype) {
    return hipk_mg_work_bytes(levels_host, nlev, HIPK_MG_TAIL_W_MAX_LEVELS, dtype, 6);
}

extern "C" size_t hipk_mg_gtail_work_bytes_w(const hipk_mg_glevel *levels_host, int nlev, int dtype) {
    return hipk_mg_work_bytes(levels_host, nlev, HIPK_MG_TAIL_W_MAX_LEVELS, dtype, 6);
}

extern "C" size_t hipk_mg_gtail_dense_work_bytes_w(const hipk_mg_glevel *levels_host, int nlev, int dtype) {
    return hipk_mg_work_bytes(levels_host, nlev, HIPK_MG_TAIL_W_MAX_LEVELS, dtype, 6);
}

extern "C" int hipk_mg_tail_apply_w(const hipk_mg_level *levels_host, const void *levels_dev, int nlev, int degree, double omega,
                                    double scale, const void *r, void *z, int dtype, void *work, size_t work_bytes, hipk_stream_t stream) {
    HIPK_REQUIRE(!levels_host || nlev <= HIPK_MG_TAIL_W_MAX_LEVELS, HIPK_ERR_UNSUPPORTED, HIPK_MG_W_TOO_MANY);
    HIPK_TRY(hipk_mg_tail_check(levels_host, nlev, degree, dtype,
                                "hipk_mg_tail_apply_w takes levels of at most 4096 unknowns and 32 stored entries per row"));
    return hipk_mg_tail_launch(levels_host, levels_dev, nlev, HIPK_MG_TAIL_W_MAX_LEVELS, r, z, dtype, work, work_bytes, [&](auto tag) {
        typedef decltype(tag) T;
        hipk_mg_tail_w_kernel<T, hipk_mg_level, hipk_mg_box_xf><<<1, HIPK_THREADS, 0, (hipStream_t)stream>>>(
            (const hipk_mg_level *)levels_dev, nlev, degree, (T)omega, (T)scale, (const T *)r, (T *)z, (T *)work);
    }, 6);
}

extern "C" int hipk_mg_gtail_apply_w(const hipk_mg_glevel *levels_host, const void *levels_dev, int nlev, int degree, double omega,
                                     double scale, const void *r, void *z, int dtype, void *work, size_t work_bytes, hipk_stream_t stream) {
    HIPK_REQUIRE(!levels_host || nlev <= HIPK_MG_TAIL_W_MAX_LEVELS, HIPK_ERR_UNSUPPORTED, HIPK_MG_W_TOO_MANY);
    HIPK_TRY(hipk_mg_gtail_check(levels_host, nlev, nlev, degree, dtype, HIPK_MG_W_TOO_MANY,
                                 "hipk_mg_gtail_apply_w takes levels of at most 4096 unknowns and 32 stored entries per row"));
    return hipk_mg_tail_launch(levels_host, levels_dev, nlev, HIPK_MG_TAIL_W_MAX_LEVELS, r, z, dtype, work, work_bytes, [&](auto tag) {
        typedef decltype(tag) T;
        hipk_mg_tail_w_kernel<T, hipk_mg_glevel, hipk_mg_index_xf><<<1, HIPK_THREADS, 0, (hipStream_t)stream>>>(
            (const hipk_mg_glevel *)levels_dev, nlev, degree, (T)omega, (T)scale, (const T *)r, (T *)z, (T *)work);
    }, 6);
}

extern "C" int hipk_mg_gtail_dense_apply_w(const hipk_mg_glevel *levels_host, const void *levels_dev, int nlev, int degree, double omega,
                                           double scale, const void *cinv, int64_t ld, const void *r, void *z, int dtype, void *work,
                                           size_t work_bytes, hipk_stream_t stream) {
    HIPK_REQUIRE(!levels_host || nlev <= HIPK_MG_TAIL_W_MAX_LEVELS, HIPK_ERR_UNSUPPORTED, HIPK_MG_W_TOO_MANY);
    HIPK_TRY(hipk_mg_gtail_check(levels_host, nlev - 1, nlev, degree, dtype, HIPK_MG_W_TOO_MANY,
                                 "hipk_mg_gtail_dense_apply_w takes sparse levels of at most 4096 unknowns and 32 stored entries per row"));
    HIPK_TRY(hipk_mg_dense_check(levels_host[nlev - 1].n, HIPK_MG_DENSE_TAIL_N, ld, cinv, dtype,
                                 "hipk_mg_gtail_dense_apply_w takes a dense level of at most 512 unknowns"));
    return hipk_mg_tail_launch(levels_host, levels_dev, nlev, HIPK_MG_TAIL_W_MAX_LEVELS, r, z, dtype, work, work_bytes, [&](auto tag) {
        typedef decltype(tag) T;
        hipk_mg_gtail_dense_w_kernel<T><<<1, HIPK_THREADS, 0, (hipStream_t)stream>>>((const hipk_mg_glevel *)levels_dev, nlev, degree, (T)omega,
                                                                                     (T)scale, (const T *)cinv, (int)ld, (const T *)r, (T *)z,
                                                                                     (T *)work);
    }, 6);
}
