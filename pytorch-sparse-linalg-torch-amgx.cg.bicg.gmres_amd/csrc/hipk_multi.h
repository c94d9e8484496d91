// hipk_multi.h -- state and device helpers of the multi-right-hand-side solves (hipk_multi.hip).
//
// Block layout: the k <= 16 columns of one block are stored row-major, (n, KP) with KP in {2, 4, 8, 16} the padded width, so
// the KP values of a row are contiguous and a gather of x[col] fetches a whole row of the block.  Padding columns (k <= c < KP)
// are never read, written or counted.  Every column runs the single-vector launch sequence's arithmetic in the oracle's order;
// the column mask `act` (bit c: column c still iterates) is read once per workgroup and broadcast, so the workgroups of a launch
// agree on it, and a frozen column's vectors are neither read nor written again.
#pragma once

#include "hipk_common.h"

#define HIPK_MULTI_MAXK 16

// one column's scalars (written by thread 0 of workgroup 0 of the deciding kernel only, read by later launches)
struct hipk_mcol {
    double gamma[2];   // CG: <r,r> (PCG: <r,z>) ping-pong by iteration parity
    double rs;         // CG / PCG: <r,r> of the last stop test; BiCGStab: rs of the last direction step (recurrence_rs)
    double atol2, bs;  // max(tol^2 <b,b>, atol^2), <b,b>
    double alpha;      // CG: gamma / <p,Ap> of this iteration (update -> direction)
    double rho, omega, rho_new, alpha_new;  // BiCGStab
    double res2, xx;   // epilogue: ||b - A x||^2 (PCG / Jacobi BiCGStab: of M (b - A x)), <x,x>
    int64_t stop_it;   // iterations >= stop_it are no-ops for this column
    int64_t iters;     // BiCGStab: completed iterations
    int32_t code;      // BiCGStab breakdown: 0 / -10 / -11
    int32_t extra_mv;  // BiCGStab: SpMVs of the iteration that broke down
};
static_assert(sizeof(hipk_mcol) <= 128, "a column's state is 128 bytes");

// the block's words
struct hipk_mblk {
    int64_t all_stop;   // iterations >= all_stop are no-ops for the whole block (hipk_pacer follows it)
    int64_t spmvs;      // block-SpMV launches that did work (some column active)
    int64_t *host_sig;  // pinned host word the deciding kernel reports to (hipk_pacer), or null
};

#ifdef __HIPCC__
template <typename T, int KP>
struct hipk_mvec {
    static constexpr int PV = (int)(16 / sizeof(T)) < KP ? (int)(16 / sizeof(T)) : KP;  // elements per 16-byte (or narrower) piece
    typedef T type __attribute__((ext_vector_type(PV)));
    static constexpr unsigned PM = (1u << PV) - 1u;
};

// v[c] = p[c] for the active columns of one row of a block (p: the row's start, aligned to KP * sizeof(T) bytes)
template <typename T, int KP>
__device__ __forceinline__ void hipk_mld(const T *__restrict__ p, unsigned act, T (&v)[KP]) {
    typedef hipk_mvec<T, KP> M;
#pragma unroll
    for (int q = 0; q < KP / M::PV; ++q) {
        const unsigned m = (act >> (q * M::PV)) & M::PM;
        if (m == M::PM) {
            const typename M::type t = *(const typename M::type *)(p + q * M::PV);
#pragma unroll
            for (int e = 0; e < M::PV; ++e) v[q * M::PV + e] = t[e];
        } else if (m) {
#pragma unroll
            for (int e = 0; e < M::PV; ++e)
                if ((m >> e) & 1u) v[q * M::PV + e] = p[q * M::PV + e];
        }
    }
}
template <typename T, int KP>
__device__ __forceinline__ void hipk_mst(T *__restrict__ p, unsigned act, const T (&v)[KP]) {
    typedef hipk_mvec<T, KP> M;
#pragma unroll
    for (int q = 0; q < KP / M::PV; ++q) {
        const unsigned m = (act >> (q * M::PV)) & M::PM;
        if (m == M::PM) {
            typename M::type t;
#pragma unroll
            for (int e = 0; e < M::PV; ++e) t[e] = v[q * M::PV + e];
            *(typename M::type *)(p + q * M::PV) = t;
        } else if (m) {
#pragma unroll
            for (int e = 0; e < M::PV; ++e)
                if ((m >> e) & 1u) p[q * M::PV + e] = v[q * M::PV + e];
        }
    }
}

// hipk_block_sum for the active columns at once (v[t] += v[t+128], v[t] += v[t+64], the wavefront tree): the same pairs, the same
// bits per column.  Result in every thread (0.0 for inactive columns).  lds: 128 * KP doubles.
template <int KP>
__device__ __forceinline__ void hipk_msum(double (&v)[KP], unsigned act, double *lds) {
    const int t = threadIdx.x;
    if (t >= 128) {
#pragma unroll
        for (int c = 0; c < KP; ++c)
            if ((act >> c) & 1u) lds[c * 128 + t - 128] = v[c];
    }
    __syncthreads();
    if (t < 128) {
#pragma unroll
        for (int c = 0; c < KP; ++c)
            if ((act >> c) & 1u) v[c] = v[c] + lds[c * 128 + t];
    }
    __syncthreads();
    if (t >= 64 && t < 128) {
#pragma unroll
        for (int c = 0; c < KP; ++c)
            if ((act >> c) & 1u) lds[c * 128 + t - 64] = v[c];
    }
    __syncthreads();
    if (t < 64) {
#pragma unroll
        for (int c = 0; c < KP; ++c)
            if ((act >> c) & 1u) {
                const double a = hipk_wave_sum(v[c] + lds[c * 128 + t]);
                if (t == 0) lds[c * 128] = a;
            }
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < KP; ++c) v[c] = ((act >> c) & 1u) ? lds[c * 128] : 0.0;
    __syncthreads();
}

// hipk_reduce_parts per active column over cnt partials laid out [i * KP + c] (thread t takes t, t + 256, .. in ascending order)
template <int KP>
__device__ __forceinline__ void hipk_mfold(const double *__restrict__ part, int cnt, unsigned act, double *lds, double (&out)[KP]) {
#pragma unroll
    for (int c = 0; c < KP; ++c) out[c] = 0.0;
    for (int i = threadIdx.x; i < cnt; i += HIPK_THREADS) {
#pragma unroll
        for (int c = 0; c < KP; ++c)
            if ((act >> c) & 1u) out[c] = out[c] + part[(size_t)i * KP + c];
    }
    hipk_msum<KP>(out, act, lds);
}
#endif  // __HIPCC__
