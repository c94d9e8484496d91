// hipk_mg.hip -- grid transfer kernels of the aggregation multigrid preconditioner (include/hipk.h, "aggregation multigrid";
// module_a/multigrid.py drives them).
//
// A level is a box of n0 x n1 x n2 points, row index (i0 n1 + i1) n2 + i2 (a two-dimensional grid is n0 = 1); the next level has
// m_d = ceil(n_d / 2) points per dimension and the aggregate of fine point (i0, i1, i2) is coarse point (i0 / 2, i1 / 2, i2 / 2).
// All indices come from the dimensions: there are no index arrays.  Every kernel walks the vector it WRITES in the library's chunk
// form (hipk_blas1.h: a reduction chunk of the vector's own geometry per workgroup, hipk_xcd_chunk placing the k-th eighth of the
// chunks on XCD k), in 16-byte groups (VEC = 2 doubles / 4 floats).  A group starts at a multiple of VEC elements, so the stores
// (and the loads of the same vector) are aligned 16-byte accesses whatever the parity of the dimensions; only the group that holds
// element n - 1 may be ragged and goes element by element.  Elements at and beyond n are never read or written.  The placement is
// that of the Chebyshev and CG vector kernels on both sides: the part of z, d or rc a workgroup touches is the part the same XCD
// wrote or reads next.  (A plain grid-stride form, blocks interleaved over the XCDs, ran level 0 of a 2000 x 2000 grid at
// 36 - 42 us per kernel -- 2 - 2.7 TB/s -- with 512 and with 2048 workgroups alike.)  The gathers from the OTHER grid go pair by
// pair: lane-consecutive groups read lane-consecutive addresses, fp64 pairs as one 16-byte load where the pair is aligned.
// One rounding per operation, no fma (the file is built with -ffp-contract=off).
#include "hipk_blas1.h"
#include "hipk_common.h"
#include "hipk_mg_tail.h"

struct hipk_mg_dims {
    int64_t n0, n1, n2;   // the fine level
    int64_t m0, m1, m2;   // the coarse level
};

static inline hipk_mg_dims hipk_mg_make_dims(int64_t n0, int64_t n1, int64_t n2) {
    hipk_mg_dims d;
    d.n0 = n0, d.n1 = n1, d.n2 = n2;
    d.m0 = (n0 + 1) / 2, d.m1 = (n1 + 1) / 2, d.m2 = (n2 + 1) / 2;
    return d;
}

// rc[I] = the sum of t over the members of aggregate I in ascending fine index, left to right; the first member (always present)
// starts the sum.  A thread owns VEC consecutive coarse elements.
template <typename T>
__global__ __launch_bounds__(HIPK_THREADS) void hipk_mg_restrict_kernel(hipk_mg_dims g, int ch, int ng, const T *__restrict__ t,
                                                                        T *__restrict__ rc) {
    constexpr int VEC = hipk_vec<T>::VEC;
    typedef typename hipk_vec<T>::type V;
    const int c = hipk_xcd_chunk(blockIdx.x, ng);
    if (c < 0) return;
    hipk_chunk_loop<T, 1>(g.m0 * g.m1 * g.m2, ch, c, [&](int64_t J, int nv) {
        int64_t I2 = J % g.m2, line = J / g.m2;
        int64_t I1 = line % g.m1, I0 = line / g.m1;
        T acc[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            if (k < nv) {
                const bool has2 = 2 * I2 + 1 < g.n2;
                T s = (T)0;
#pragma unroll
                for (int d0 = 0; d0 < 2; ++d0) {
#pragma unroll
                    for (int d1 = 0; d1 < 2; ++d1) {
                        const int64_t i0 = 2 * I0 + d0, i1 = 2 * I1 + d1;
                        if (i0 < g.n0 && i1 < g.n1) {
                            const int64_t f = (i0 * g.n1 + i1) * g.n2 + 2 * I2;
                            T a, b = (T)0;
                            if (sizeof(T) == 8 && has2 && (f & 1) == 0) {   // an aligned 16-byte pair
                                const V p = *reinterpret_cast<const V *>(t + f);
                                a = ((const T *)&p)[0];
                                b = ((const T *)&p)[1];
                            } else {
                                a = t[f];
                                if (has2) b = t[f + 1];
                            }
                            s = (d0 == 0 && d1 == 0) ? a : s + a;
                            if (has2) s = s + b;
                        }
                    }
                }
                acc[k] = s;
                if (++I2 == g.m2) {
                    I2 = 0;
                    if (++I1 == g.m1) I1 = 0, ++I0;
                }
            }
        }
        hipk_st<T>(rc, J, nv, acc);
    });
}

// z[i] = z[i] + (omega * e[agg(i)]).  A thread owns VEC consecutive fine elements.
template <typename T>
__global__ __launch_bounds__(HIPK_THREADS) void hipk_mg_prolong_add_kernel(hipk_mg_dims g, int ch, int ng, T omega, const T *__restrict__ e,
                                                                           T *__restrict__ z) {
    constexpr int VEC = hipk_vec<T>::VEC;
    const int c = hipk_xcd_chunk(blockIdx.x, ng);
    if (c < 0) return;
    hipk_chunk_loop<T, 1>(g.n0 * g.n1 * g.n2, ch, c, [&](int64_t i, int nv) {
        int64_t i2 = i % g.n2, line = i / g.n2;
        int64_t i1 = line % g.n1, i0 = line / g.n1;
        T zv[VEC];
        hipk_ld<T>(z, i, nv, zv);
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            if (k < nv) {
                const T ev = e[((i0 >> 1) * g.m1 + (i1 >> 1)) * g.m2 + (i2 >> 1)];
                zv[k] = zv[k] + (omega * ev);
                if (++i2 == g.n2) {
                    i2 = 0;
                    if (++i1 == g.n1) i1 = 0, ++i0;
                }
            }
        }
        hipk_st<T>(z, i, nv, zv);
    });
}

// z = scale * (z + d): the end of a level's post-smoothing (scale = 1 below level 0)
template <typename T>
__global__ __launch_bounds__(HIPK_THREADS) void hipk_mg_correct_kernel(int64_t n, int ch, int ng, T scale, const T *__restrict__ d, T *__restrict__ z) {
    constexpr int VEC = hipk_vec<T>::VEC;
    const int c = hipk_xcd_chunk(blockIdx.x, ng);
    if (c < 0) return;
    hipk_chunk_loop<T>(n, ch, c, [&](int64_t i, int nv) {
        T zv[VEC], dv[VEC];
        hipk_ld<T>(z, i, nv, zv);
        hipk_ld<T>(d, i, nv, dv);
#pragma unroll
        for (int k = 0; k < VEC; ++k) zv[k] = scale * (zv[k] + dv[k]);
        hipk_st<T>(z, i, nv, zv);
    });
}

// z = scale * (dinv * r): the level with one unknown
template <typename T>
__global__ __launch_bounds__(HIPK_THREADS) void hipk_mg_diag_kernel(int64_t n, T scale, const T *__restrict__ dinv, const T *__restrict__ r,
                                                                    T *__restrict__ z) {
    for (int64_t i = (int64_t)blockIdx.x * HIPK_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * HIPK_THREADS)
        z[i] = scale * (dinv[i] * r[i]);
}

static inline int hipk_mg_diag_grid(int64_t n) {
    const int64_t b = (n + HIPK_THREADS - 1) / HIPK_THREADS;
    return (int)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}

static int hipk_mg_check(int64_t n0, int64_t n1, int64_t n2, const void *a, const void *b, int dtype) {
    HIPK_REQUIRE(a && b, HIPK_ERR_ARG, "null argument");
    HIPK_REQUIRE(n0 >= 1 && n1 >= 1 && n2 >= 1, HIPK_ERR_ARG, "every grid dimension must be at least 1");
    HIPK_REQUIRE(n0 <= (INT64_MAX / n1) / n2, HIPK_ERR_ARG, "the grid has more than 2^63 points");
    HIPK_REQUIRE(dtype == HIPK_F64 || dtype == HIPK_F32, HIPK_ERR_UNSUPPORTED, "dtype must be HIPK_F32 or HIPK_F64");
    HIPK_REQUIRE(hipk_aligned16(a) && hipk_aligned16(b), HIPK_ERR_ALIGN, "vectors must be 16-byte aligned");
    HIPK_REQUIRE(a != b, HIPK_ERR_ARG, "the two vectors must be distinct");
    return HIPK_OK;
}

extern "C" int hipk_mg_restrict(int64_t n0, int64_t n1, int64_t n2, const void *t, void *rc, int dtype, hipk_stream_t stream) {
    HIPK_TRY(hipk_mg_check(n0, n1, n2, t, rc, dtype));
    const hipk_mg_dims g = hipk_mg_make_dims(n0, n1, n2);
    const hipk_geom gm = hipk_make_geom(g.m0 * g.m1 * g.m2);   // the coarse vector's chunks
    if (dtype == HIPK_F64)
        hipk_mg_restrict_kernel<double><<<hipk_xcd_grid(gm.g), HIPK_THREADS, 0, (hipStream_t)stream>>>(g, gm.ch, gm.g, (const double *)t, (double *)rc);
    else
        hipk_mg_restrict_kernel<float><<<hipk_xcd_grid(gm.g), HIPK_THREADS, 0, (hipStream_t)stream>>>(g, gm.ch, gm.g, (const float *)t, (float *)rc);
    HIPK_CHECK_HIP(hipGetLastError());
    return HIPK_OK;
}

extern "C" int hipk_mg_prolong_add(int64_t n0, int64_t n1, int64_t n2, double omega, const void *e, void *z, int dtype,
                                   hipk_stream_t stream) {
    HIPK_TRY(hipk_mg_check(n0, n1, n2, e, z, dtype));
    const hipk_mg_dims g = hipk_mg_make_dims(n0, n1, n2);
    const hipk_geom gm = hipk_make_geom(n0 * n1 * n2);
    if (dtype == HIPK_F64)
        hipk_mg_prolong_add_kernel<double><<<hipk_xcd_grid(gm.g), HIPK_THREADS, 0, (hipStream_t)stream>>>(g, gm.ch, gm.g, omega, (const double *)e, (double *)z);
    else
        hipk_mg_prolong_add_kernel<float><<<hipk_xcd_grid(gm.g), HIPK_THREADS, 0, (hipStream_t)stream>>>(g, gm.ch, gm.g, (float)omega, (const float *)e, (float *)z);
    HIPK_CHECK_HIP(hipGetLastError());
    return HIPK_OK;
}

extern "C" int hipk_mg_correct(int64_t n, double scale, const void *d, void *z, int dtype, hipk_stream_t stream) {
    HIPK_REQUIRE(n >= 1, HIPK_ERR_ARG, "n must be at least 1");
    HIPK_TRY(hipk_mg_check(1, 1, n, d, z, dtype));
    const hipk_geom gm = hipk_make_geom(n);
    if (dtype == HIPK_F64)
        hipk_mg_correct_kernel<double><<<hipk_xcd_grid(gm.g), HIPK_THREADS, 0, (hipStream_t)stream>>>(n, gm.ch, gm.g, scale, (const double *)d, (double *)z);
    else
        hipk_mg_correct_kernel<float><<<hipk_xcd_grid(gm.g), HIPK_THREADS, 0, (hipStream_t)stream>>>(n, gm.ch, gm.g, (float)scale, (const float *)d, (float *)z);
    HIPK_CHECK_HIP(hipGetLastError());
    return HIPK_OK;
}

extern "C" int hipk_mg_diag(int64_t n, double scale, const void *dinv, const void *r, void *z, int dtype, hipk_stream_t stream) {
    HIPK_REQUIRE(n >= 1 && dinv, HIPK_ERR_ARG, "n must be at least 1 and dinv not null");
    HIPK_TRY(hipk_mg_check(1, 1, n, r, z, dtype));
    HIPK_REQUIRE(dinv != z, HIPK_ERR_ARG, "dinv and z must be distinct");
    if (dtype == HIPK_F64)
        hipk_mg_diag_kernel<double><<<hipk_mg_diag_grid(n), HIPK_THREADS, 0, (hipStream_t)stream>>>(n, scale, (const double *)dinv, (const double *)r, (double *)z);
    else
        hipk_mg_diag_kernel<float><<<hipk_mg_diag_grid(n), HIPK_THREADS, 0, (hipStream_t)stream>>>(n, (float)scale, (const float *)dinv, (const float *)r, (float *)z);
    HIPK_CHECK_HIP(hipGetLastError());
    return HIPK_OK;
}

// ------------------------------------------------------------------------------------------------------------- the tail kernel
// One launch, ONE 256-thread workgroup: V(l, .) for the run of small levels j = 0 .. nlev - 1 of the descriptor array (level
// nlev - 1 has one unknown), down and back up -- what the launch sequence spends 2 degree + 7 launches per level on.  The steps,
// the walks, the slab layout and the rules they keep are hipk_mg_tail.h's, shared with the tail kernels of the index-array levels
// (hipk_mg_graph.hip, hipk_mg_dense.hip); the box arithmetic of the two transfers is its hipk_mg_box_xf.  The result is bit for
// bit the launch sequence's.
template <typename T>
__global__ __launch_bounds__(HIPK_THREADS) void hipk_mg_tail_kernel(const hipk_mg_level *__restrict__ lv, int nlev, int m, T omega, T scale,
                                                                    const T *rin, T *zout, T *slab) {
    __shared__ T xs[HIPK_MG_TAIL_MAX_N];
    hipk_mg_walk_down<T, hipk_mg_level, hipk_mg_box_xf>(lv, nlev, m, rin, zout, slab, xs);
    hipk_mg_last_diag<T>(lv, nlev, scale, rin, zout, slab);   // the level with one unknown
    hipk_mg_walk_up<T, hipk_mg_level, hipk_mg_box_xf>(lv, nlev, m, omega, scale, rin, zout, slab, xs);
}

extern "C" size_t hipk_mg_tail_work_bytes(const hipk_mg_level *levels_host, int nlev, int dtype) {
    return hipk_mg_work_bytes(levels_host, nlev, HIPK_MG_TAIL_MAX_LEVELS, dtype);
}

extern "C" int hipk_mg_tail_apply(const hipk_mg_level *levels_host, const void *levels_dev, int nlev, int degree, double omega,
                                  double scale, const void *r, void *z, int dtype, void *work, size_t work_bytes, hipk_stream_t stream) {
    HIPK_TRY(hipk_mg_tail_check(levels_host, nlev, degree, dtype,
                                "hipk_mg_tail_apply takes levels of at most 4096 unknowns and 32 stored entries per row"));
    return hipk_mg_tail_launch(levels_host, levels_dev, nlev, HIPK_MG_TAIL_MAX_LEVELS, r, z, dtype, work, work_bytes, [&](auto tag) {
        typedef decltype(tag) T;
        hipk_mg_tail_kernel<T><<<1, HIPK_THREADS, 0, (hipStream_t)stream>>>((const hipk_mg_level *)levels_dev, nlev, degree, (T)omega, (T)scale,
                                                                            (const T *)r, (T *)z, (T *)work);
    });
}
