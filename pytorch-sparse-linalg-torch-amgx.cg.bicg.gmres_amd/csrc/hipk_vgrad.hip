// hipk_vgrad.hip -- the matrix gradient of a solve (include/hipk.h, "matrix gradient of a solve"; module_a/matrix_grad.py and
// module_a/batch.py drive it).  With x = A^-1 b, g = dL/dx and lam = A^-T g, the gradient with respect to the stored entry k of A is
//     G[k] = -(lam[row(k)] * x[col(k)])
// one multiplication in T and a negation, per stored entry: a column stored twice gives both entries the same value, a stored zero
// gets a gradient like any other entry.  The output has A's pattern (nothing is summed, so there are no atomics and nothing to
// order), which makes this an entry-parallel stream: 4 bytes of col in, sizeof(T) of G out, a gather of x and a near-broadcast of lam.
//
// One kernel template, hipk_csr_vgrad_kernel<T>, behind both entries (the handle form is the batch form with batch = 1):
//   * grid x: tiles of HIPK_THREADS = 256 consecutive rows.  The tile's 257 row pointers go to LDS; its entries are the contiguous
//     range [crow[t0], crow[t1]) of col / G, walked by the 256 threads in strides of 256 (coalesced col loads and G stores), 4
//     entries per thread and pass.  A row of any length is just a longer range: no envelope, no special path for a dense row.
//   * row(k) = the last row r of the tile with crow[r] <= k: an upper-bound search in the LDS slice, which skips empty rows.
//   * grid y: slices of at most HIPK_VG_SLICE = 8 systems.  A thread keeps the (row, col) pairs of its 4 entries in registers and
//     loops over the systems of the slice, so the search is paid once per slice; the slice's lam tiles (8 x 256 values) sit in LDS.
//   * every G[s ldg + k], k < nnz, is written exactly once by an ordinary store; offsets into L, X and G are 64-bit.
// No communication between workgroups, no polling, no scratch.  The file is built with -ffp-contract=off like the rest.
#include "hipk_common.h"

#define HIPK_VG_SLICE 8   // systems per grid-y slice: their lam tiles share the LDS block
#define HIPK_VG_UNROLL 4  // entries per thread and pass over the tile's entry range

template <typename T>
__global__ __launch_bounds__(HIPK_THREADS) void hipk_csr_vgrad_kernel(int64_t n, const int32_t *__restrict__ crow, const int32_t *__restrict__ col,
                                                                      int batch, int spb, const T *__restrict__ L, int64_t ldl,
                                                                      const T *__restrict__ X, int64_t ldx, T *__restrict__ G, int64_t ldg) {
    __shared__ int s_crow[HIPK_THREADS + 1];
    __shared__ T s_lam[HIPK_VG_SLICE][HIPK_THREADS];
    const int tid = threadIdx.x;
    const int64_t t0 = (int64_t)blockIdx.x * HIPK_THREADS;
    const int rows = (int)((n - t0) < HIPK_THREADS ? (n - t0) : HIPK_THREADS);   // >= 1: the grid has ceil(n / 256) tiles
    if (tid < rows) s_crow[tid] = crow[t0 + tid];
    if (tid == 0) s_crow[rows] = crow[t0 + rows];
    __syncthreads();
    const int64_t e0 = s_crow[0], e1 = s_crow[rows];
    if (e0 == e1) return;   // a tile of empty rows (the same in every thread: no barrier is skipped by some)
    const int nsl = (batch + spb - 1) / spb;
    for (int sl = blockIdx.y; sl < nsl; sl += gridDim.y) {
        const int s0 = sl * spb;
        const int cnt = (batch - s0) < spb ? (batch - s0) : spb;
        if (sl != (int)blockIdx.y) __syncthreads();   // the previous slice's readers of s_lam are done
        for (int i = tid; i < cnt * HIPK_THREADS; i += HIPK_THREADS) {
            const int j = i / HIPK_THREADS, r = i % HIPK_THREADS;   // r == tid
            if (r < rows) s_lam[j][r] = L[(int64_t)(s0 + j) * ldl + t0 + r];
        }
        __syncthreads();
        for (int64_t base = e0; base < e1; base += (int64_t)HIPK_THREADS * HIPK_VG_UNROLL) {
            int rk[HIPK_VG_UNROLL], ck[HIPK_VG_UNROLL];
#pragma unroll
            for (int u = 0; u < HIPK_VG_UNROLL; ++u) {
                const int64_t k = base + (int64_t)u * HIPK_THREADS + tid;
                rk[u] = -1;
                ck[u] = 0;
                if (k < e1) {
                    ck[u] = col[k];
                    int lo = 0, hi = rows;   // invariant: s_crow[lo] <= k < s_crow[hi]
                    while (hi - lo > 1) {
                        const int mid = (lo + hi) >> 1;
                        if ((int64_t)s_crow[mid] <= k) lo = mid; else hi = mid;
                    }
                    rk[u] = lo;
                }
            }
            for (int j = 0; j < cnt; ++j) {
                const T *__restrict__ xs = X + (int64_t)(s0 + j) * ldx;
                T *__restrict__ gs = G + (int64_t)(s0 + j) * ldg;
#pragma unroll
                for (int u = 0; u < HIPK_VG_UNROLL; ++u) {
                    if (rk[u] >= 0) {
                        const int64_t k = base + (int64_t)u * HIPK_THREADS + tid;
                        const T p = s_lam[j][rk[u]] * xs[ck[u]];
                        gs[k] = -p;
                    }
                }
            }
        }
    }
}

static thread_local int hipk_vg_launches = 0;

extern "C" int hipk_last_grad_values_launches(void) { return hipk_vg_launches; }

// the shared launcher: operands validated by the two entries
template <typename T>
static int hipk_vgrad_launch(int64_t n, const int32_t *crow, const int32_t *col, int batch, const void *lam, int64_t ldl, const void *x,
                             int64_t ldx, void *g, int64_t ldg, hipStream_t stream) {
    const int64_t tiles = (n + HIPK_THREADS - 1) / HIPK_THREADS;
    // systems per slice: 1 for one system; else as few as keep about 1024 workgroups in the grid (256 CUs x 4), at most 8
    int64_t slices = batch;
    const int64_t want = (1024 + tiles - 1) / tiles;
    if (slices > want) slices = want;
    int spb = (int)((batch + slices - 1) / slices);
    if (spb > HIPK_VG_SLICE) spb = HIPK_VG_SLICE;
    slices = ((int64_t)batch + spb - 1) / spb;
    if (slices > 65535) slices = 65535;   // the kernel strides over the slices beyond the grid
    const dim3 grid((unsigned)tiles, (unsigned)slices, 1);
    hipk_csr_vgrad_kernel<T><<<grid, HIPK_THREADS, 0, stream>>>(n, crow, col, batch, spb, (const T *)lam, ldl, (const T *)x, ldx, (T *)g, ldg);
    HIPK_CHECK_HIP(hipGetLastError());
    hipk_vg_launches = 1;
    return HIPK_OK;
}

extern "C" int hipk_batch_grad_values(int64_t n, int64_t nnz, const int32_t *crow, const int32_t *col, int batch, const void *lam, int64_t ldl,
                                      const void *x, int64_t ldx, void *g, int64_t ldg, int dtype, hipk_stream_t stream) {
    hipk_vg_launches = 0;
    HIPK_REQUIRE(n >= 0 && nnz >= 0 && batch >= 0, HIPK_ERR_ARG, "negative size");
    HIPK_REQUIRE(n <= INT32_MAX && nnz <= INT32_MAX, HIPK_ERR_ARG, "n, nnz < 2^31 is required");
    HIPK_REQUIRE(dtype == HIPK_F64 || dtype == HIPK_F32, HIPK_ERR_UNSUPPORTED, "dtype must be HIPK_F32 or HIPK_F64");
    if (nnz == 0 || batch == 0) return HIPK_OK;
    HIPK_REQUIRE(n >= 1, HIPK_ERR_ARG, "nnz > 0 needs n >= 1");
    HIPK_REQUIRE(crow && col && lam && x && g, HIPK_ERR_ARG, "null argument");
    HIPK_REQUIRE(ldl >= n && ldx >= n && ldg >= nnz, HIPK_ERR_ARG, "a leading dimension is shorter than its row (ldl, ldx >= n, ldg >= nnz)");
    HIPK_REQUIRE(g != lam && g != x, HIPK_ERR_ARG, "g must be distinct from lam and x");
    HIPK_REQUIRE(hipk_aligned16(crow) && hipk_aligned16(col) && hipk_aligned16(lam) && hipk_aligned16(x) && hipk_aligned16(g), HIPK_ERR_ALIGN,
                 "crow, col, lam, x and g must be 16-byte aligned");
    const int64_t es = dtype == HIPK_F64 ? 8 : 4;
    HIPK_REQUIRE(batch == 1 || ((ldl * es) % 16 == 0 && (ldx * es) % 16 == 0 && (ldg * es) % 16 == 0), HIPK_ERR_ALIGN,
                 "with batch > 1 every ld * sizeof(T) must be a multiple of 16");
    if (dtype == HIPK_F64) return hipk_vgrad_launch<double>(n, crow, col, batch, lam, ldl, x, ldx, g, ldg, (hipStream_t)stream);
    return hipk_vgrad_launch<float>(n, crow, col, batch, lam, ldl, x, ldx, g, ldg, (hipStream_t)stream);
}

extern "C" int hipk_csr_grad_values(hipk_csr_t h, const void *lam, const void *x, void *gvals, hipk_stream_t stream) {
    hipk_vg_launches = 0;
    HIPK_REQUIRE(h, HIPK_ERR_ARG, "null handle");
    HIPK_REQUIRE(h->dtype == HIPK_F64 || h->dtype == HIPK_F32, HIPK_ERR_UNSUPPORTED, "dtype must be HIPK_F32 or HIPK_F64");
    if (h->nnz == 0) return HIPK_OK;
    HIPK_REQUIRE(lam && x && gvals, HIPK_ERR_ARG, "null argument");
    HIPK_REQUIRE(gvals != lam && gvals != x, HIPK_ERR_ARG, "gvals must be distinct from lam and x");
    HIPK_REQUIRE(hipk_aligned16(lam) && hipk_aligned16(x) && hipk_aligned16(gvals), HIPK_ERR_ALIGN, "lam, x and gvals must be 16-byte aligned");
    if (h->dtype == HIPK_F64)
        return hipk_vgrad_launch<double>(h->n_rows, h->crow, h->col, 1, lam, h->n_rows, x, h->n_cols, gvals, h->nnz, (hipStream_t)stream);
    return hipk_vgrad_launch<float>(h->n_rows, h->crow, h->col, 1, lam, h->n_rows, x, h->n_cols, gvals, h->nnz, (hipStream_t)stream);
}
