// hipk_mg_gwalk.h -- the down and up walks of the one-workgroup tail over index-array levels, shared by hipk_mg_gtail_kernel
// (hipk_mg_graph.hip, last level z = dinv r) and hipk_mg_gtail_dense_kernel (hipk_mg_dense.hip, last level z = cinv r), and the
// host check of the sparse levels' envelope.  The steps, the slab and the rules are those of hipk_mg_tail.h: the restriction
// gathers the staged t through amem, the prolongation the staged e through agg, both complete in LDS behind a barrier; thread t
// owns aggregates t, t + 256, ... of the coarse level as it owns its rows, so rc[I] is written by the thread that reads it next.
// Both walks leave and expect the last level's r and z in its slab (the caller's vectors when nlev == 1), every element
// written and read by the thread that owns its row.
#pragma once
#include "hipk_mg_tail.h"

#define HIPK_MG_GTAIL_MAX_LEVELS 32

#ifdef __HIPCC__
// down: steps 1 - 3 on levels 0 .. nlev - 2
template <typename T>
__device__ __forceinline__ void hipk_mg_gwalk_down(const hipk_mg_glevel *lv, int nlev, int m, const T *rin, T *zout, T *slab, T *xs) {
    const int t = threadIdx.x;
    for (int j = 0; j + 1 < nlev; ++j) {
        const hipk_mg_glevel &L = lv[j];
        const hipk_mg_vecs<T> v = hipk_mg_level_vecs<T>(lv, j, rin, zout, slab);
        T *rc = hipk_mg_level_vecs<T>(lv, j + 1, rin, zout, slab).r;
        hipk_mg_smooth<T>(L, m, v.r, v.z, v.w, xs);
        hipk_mg_residual<T>(L, v.z, v.r, v.t, xs);
        hipk_mg_stage(L.n, v.t, xs);
        const int nc = lv[j + 1].n;
        for (int I = t; I < nc; I += HIPK_THREADS) {
            const int lo = L.aptr[I], hi = L.aptr[I + 1];
            T s = xs[L.amem[lo]];
            for (int k = lo + 1; k < hi; ++k) s = s + xs[L.amem[k]];
            rc[I] = s;
        }
        __syncthreads();
    }
}

// up: steps 5 - 6 on levels nlev - 2 .. 0
template <typename T>
__device__ __forceinline__ void hipk_mg_gwalk_up(const hipk_mg_glevel *lv, int nlev, int m, T omega, T scale, const T *rin, T *zout,
                                                 T *slab, T *xs) {
    const int t = threadIdx.x;
    for (int j = nlev - 2; j >= 0; --j) {
        const hipk_mg_glevel &L = lv[j];
        const hipk_mg_vecs<T> v = hipk_mg_level_vecs<T>(lv, j, rin, zout, slab);
        const T *e = hipk_mg_level_vecs<T>(lv, j + 1, rin, zout, slab).z;
        hipk_mg_stage(lv[j + 1].n, e, xs);
        for (int row = t; row < L.n; row += HIPK_THREADS) v.z[row] = v.z[row] + (omega * xs[L.agg[row]]);
        __syncthreads();
        hipk_mg_residual<T>(L, v.z, v.r, v.t, xs);
        hipk_mg_smooth<T>(L, m, v.t, v.d, v.w, xs);
        for (int row = t; row < L.n; row += HIPK_THREADS) {
            const T zz = v.z[row] + v.d[row];
            v.z[row] = (j == 0) ? scale * zz : zz;
        }
    }
}
#endif

// levels [0, nsparse) of a run of nlev: the envelope and the pointers of levels that are smoothed or end in z = dinv r
static inline int hipk_mg_gtail_check_levels(const hipk_mg_glevel *lv, int nsparse, int nlev, const char *envelope) {
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
