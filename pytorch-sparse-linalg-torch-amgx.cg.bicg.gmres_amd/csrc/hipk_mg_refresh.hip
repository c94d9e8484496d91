// hipk_mg_refresh.hip -- the level scan of `AggregationMultigridPreconditioner.update` (include/hipk.h, "aggregation multigrid: the
// refresh of a hierarchy"; module_a/multigrid.py drives it).  A refresh keeps the aggregates and every index array of a hierarchy and
// recomputes the numbers: the Galerkin values are hipk_mg_restrict_agg over the stored sort order (hipk_mg_graph.hip), and what
// every level then needs from its new values -- the reciprocal diagonal, the Gershgorin bound of D^-1 A and the number of
// non-positive diagonal entries -- is ONE pass over the level's CSR arrays here.
//
// The scan walks the vector it WRITES, dinv, in the library's chunk form (hipk_blas1.h: a reduction chunk of the row space per
// workgroup, hipk_xcd_chunk placing the k-th eighth of the chunks on XCD k) in 16-byte groups: a thread owns VEC consecutive rows,
// whose entries are one contiguous run of col / val, and sums each row in stored order, so a row may have any length.  The maximum
// and the count are order-independent; the workgroup's pair goes to its own slot of the workspace and a second launch of one
// workgroup folds the slots: no atomics, no hand-off between workgroups, every slot read has been written by the launch before.
// One rounding per operation, no fma (the file is built with -ffp-contract=off).
#include <math.h>

#include "hipk_blas1.h"
#include "hipk_common.h"

// (m, nan, bad) of the 256 threads -> thread 0: the maximum of the m, whether any thread saw a NaN, the sum of the counts
__device__ __forceinline__ void hipk_mg_scan_fold(double &m, int &nan, double &bad, double *sm, int *sn, double *sb) {
    const int t = threadIdx.x;
    sm[t] = m;
    sn[t] = nan;
    sb[t] = bad;
    __syncthreads();
    for (int s = HIPK_THREADS / 2; s >= 1; s >>= 1) {
        if (t < s) {
            if (sm[t + s] > sm[t]) sm[t] = sm[t + s];
            sn[t] |= sn[t + s];
            sb[t] = sb[t] + sb[t + s];   // integers far below 2^53: exact in any order
        }
        __syncthreads();
    }
    m = sm[0];
    nan = sn[0];
    bad = sb[0];
}

// per row i: d = the sum of the stored diagonal entries, s = the sum of |a| over the row, both from 0 in stored order in T;
// dinv[i] = 1 / d; part[2 c] = max_i (double)s / (double)d over the chunk's rows (NaN when one of them is), part[2 c + 1] = the
// number of its rows with d <= 0.  want == 0: s is not formed and part[2 c] = 0.
template <typename T>
__global__ __launch_bounds__(HIPK_THREADS) void hipk_mg_level_scan_kernel(int64_t n, int ch, int ng, int want, const int32_t *__restrict__ crow,
                                                                          const int32_t *__restrict__ col, const T *__restrict__ val,
                                                                          T *__restrict__ dinv, double *__restrict__ part) {
    constexpr int VEC = hipk_vec<T>::VEC;
    __shared__ double sm[HIPK_THREADS], sb[HIPK_THREADS];
    __shared__ int sn[HIPK_THREADS];
    const int c = hipk_xcd_chunk(blockIdx.x, ng);
    if (c < 0) return;
    double m = -INFINITY, bad = 0.0;
    int nan = 0;
    hipk_chunk_loop<T, 1>(n, ch, c, [&](int64_t i, int nv) {
        T out[VEC];
        int lo = crow[i];
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            out[k] = (T)0;
            if (k < nv) {
                const int row = (int)(i + k);
                const int hi = crow[i + k + 1];
                T d = (T)0, s = (T)0;
                if (want) {
                    for (int j = lo; j < hi; ++j) {
                        const T a = val[j];
                        if (col[j] == row) d = d + a;
                        s = s + fabs(a);
                    }
                    const double q = (double)s / (double)d;
                    if (q > m) m = q;
                    if (q != q) nan = 1;
                } else {
                    for (int j = lo; j < hi; ++j)
                        if (col[j] == row) d = d + val[j];
                }
                if (d <= (T)0) bad = bad + 1.0;
                out[k] = (T)1 / d;
                lo = hi;
            }
        }
        hipk_st<T>(dinv, i, nv, out);
    });
    hipk_mg_scan_fold(m, nan, bad, sm, sn, sb);
    if (threadIdx.x == 0) {
        part[2 * c] = want ? (nan ? (double)NAN : m) : 0.0;
        part[2 * c + 1] = bad;
    }
}

// out[0] = the maximum of part[2 c], NaN when one of them is; out[1] = the sum of part[2 c + 1]; c < g, one workgroup
__global__ __launch_bounds__(HIPK_THREADS) void hipk_mg_level_fold_kernel(const double *__restrict__ part, int g, int want, double *__restrict__ out) {
    __shared__ double sm[HIPK_THREADS], sb[HIPK_THREADS];
    __shared__ int sn[HIPK_THREADS];
    double m = -INFINITY, bad = 0.0;
    int nan = 0;
    for (int c = threadIdx.x; c < g; c += HIPK_THREADS) {
        const double q = part[2 * c];
        if (q > m) m = q;
        if (q != q) nan = 1;
        bad = bad + part[2 * c + 1];
    }
    hipk_mg_scan_fold(m, nan, bad, sm, sn, sb);
    if (threadIdx.x == 0) {
        out[0] = want ? (nan ? (double)NAN : m) : 0.0;
        out[1] = bad;
    }
}

extern "C" size_t hipk_mg_level_scan_work_bytes(int64_t n) {
    if (n < 1 || n > INT32_MAX) return 0;
    return (size_t)hipk_make_geom(n).g * 2 * sizeof(double);
}

extern "C" int hipk_mg_level_scan(int64_t n, const int32_t *crow, const int32_t *col, const void *val, int dtype, int want_lmax, void *dinv,
                                  double *out, void *work, size_t work_bytes, hipk_stream_t stream) {
    HIPK_REQUIRE(crow && col && val && dinv && out && work, HIPK_ERR_ARG, "null argument");
    HIPK_REQUIRE(n >= 1 && n <= INT32_MAX, HIPK_ERR_ARG, "1 <= n < 2^31 is required");
    HIPK_REQUIRE(want_lmax == 0 || want_lmax == 1, HIPK_ERR_ARG, "want_lmax must be 0 or 1");
    HIPK_REQUIRE(dtype == HIPK_F64 || dtype == HIPK_F32, HIPK_ERR_UNSUPPORTED, "dtype must be HIPK_F32 or HIPK_F64");
    HIPK_REQUIRE(hipk_aligned16(crow) && hipk_aligned16(col) && hipk_aligned16(val) && hipk_aligned16(dinv) && hipk_aligned16(out) &&
                     hipk_aligned16(work),
                 HIPK_ERR_ALIGN, "the CSR arrays, dinv, out and work must be 16-byte aligned");
    HIPK_REQUIRE(val != dinv, HIPK_ERR_ARG, "val and dinv must be distinct");
    HIPK_REQUIRE(work_bytes >= hipk_mg_level_scan_work_bytes(n), HIPK_ERR_WORKSPACE, "work is smaller than hipk_mg_level_scan_work_bytes");
    const hipk_geom gm = hipk_make_geom(n);
    double *part = (double *)work;
    if (dtype == HIPK_F64)
        hipk_mg_level_scan_kernel<double><<<hipk_xcd_grid(gm.g), HIPK_THREADS, 0, (hipStream_t)stream>>>(n, gm.ch, gm.g, want_lmax, crow, col,
                                                                                                       (const double *)val, (double *)dinv, part);
    else
        hipk_mg_level_scan_kernel<float><<<hipk_xcd_grid(gm.g), HIPK_THREADS, 0, (hipStream_t)stream>>>(n, gm.ch, gm.g, want_lmax, crow, col,
                                                                                                      (const float *)val, (float *)dinv, part);
    HIPK_CHECK_HIP(hipGetLastError());
    hipk_mg_level_fold_kernel<<<1, HIPK_THREADS, 0, (hipStream_t)stream>>>(part, gm.g, want_lmax, out);
    HIPK_CHECK_HIP(hipGetLastError());
    return HIPK_OK;
}
