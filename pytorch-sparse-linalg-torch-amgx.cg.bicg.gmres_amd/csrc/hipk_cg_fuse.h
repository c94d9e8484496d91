// hipk_cg_fuse.h -- the CG loop's stencil SpMV and its update step in ONE launch: Ap never leaves the chip.
//
// The three-launch iteration writes Ap (8 n bytes) in the SpMV and reads it back in the update kernel, and nobody else reads it.
// Both kernels run one workgroup per reduction chunk and the same rows belong to the same chunk in both; only the scalar
// alpha = gamma / <p,Ap> stands between them, and that needs every chunk's partial.  Here a workgroup
//   1. walks its chunk's tiles as hipk_spmv_sell_wide_kernel does (hipk_sell_wide_walk, FUSE: the same code), Ap staying in LDS
//      (16 KB, indexed by the row's place in the chunk) and the chunk's <p,Ap> partial folded as there (hipk_wave_fold): same bits;
//   2. requests its chunk of r in hipk_cg_update_kernel's per-thread layout (16-byte accesses, thread t, steps of 512 elements);
//   3. publishes the partial as a flagged 16-byte word {value, seq} (hipk_ll_put, hipk_mid.h) -- nobody waits before this;
//   4. the workgroup dispatched first (blockIdx.x == 0) polls the g words (hipk_mid_poll, thread t the words t, t + 256, ...: the
//      order of hipk_reduce_parts), folds them with hipk_block_sum -- the bits every workgroup of hipk_cg_update_kernel derives --
//      and hands <p,Ap> to the others as eight flagged words 128 bytes apart; workgroup b polls replica b & 7 (one lane, relaxed:
//      hipk_fx.h records what an acquire per poll and what every workgroup polling every partial cost);
//   5. alpha = (T)(gamma / <p,Ap>), r -= alpha Ap with Ap from LDS, <r,r> in the update kernel's element order, hipk_block_sum,
//      part_rr[c]: the bits hipk_cg_update_kernel stores.  One thread leaves alpha in the scalar block for the deferred x update.
// Every flagged word validates itself ({lo, seq, hi, seq}), so the value needs no flag of its own and no drain in between.
// seq = iterations since the sequence began + 1: different in every launch of a solve; the host clears the words when the
// sequence begins, so a workspace of any content gives the same solve.
// The g workgroups must be resident together (the host checks g against the occupancy of this kernel; <= 80 SGPRs, <= 64 VGPRs
// and <= 20 KB of LDS by construction: eight workgroups per CU).  Every wait is bounded.  When the collector's poll runs out (a
// workgroup of the launch is not running) it hands out the give-up mark instead of the value, sets stop_it = it and ctl.redo = -1:
// no workgroup has stored r, part_rr or alpha for that iteration, the state is that of iteration `it`, and the host goes on from
// there with the separate kernels (hipk_cg_steps::fuse_end).  give_up (HIPK_TEST_CG_FUSE_GIVE_UP): the collector behaves as
// if its poll had run out, without waiting.
#pragma once
#include "hipk_coded.h"
#include "hipk_mid.h"

static constexpr unsigned kFuseGaveUp = 0x80000000u;   // in a replica's seq: the collector gave up (seq itself stays below 2^31)
static constexpr unsigned kFuseReplicaSlots = 8;       // replicas 8 slots of 16 bytes = 128 bytes apart
static constexpr size_t kFuseCtlBytes = 8 * 128;
static constexpr size_t kFuseWordsBytes = (size_t)HIPK_MAX_PARTS * 16;
static constexpr unsigned kFuseWaitBound = 1u << 24;   // polls of a replica (well beyond the collector's own bound, 8 x kMidSpinBound)

struct hipk_cg_fuse_args {
    hipk_cg_scal *scal;
    double *r;
    double *part_rr;
    double *part_pap;   // the plain <p,Ap> partials as the SpMV leaves them: hipk_cg_direction_kernel folds them (HIPK_CG_DEFER_X=0)
    void *words;     // g flagged words: {<p,Ap> partial of chunk c, seq} at slot c
    void *ctl;       // the collector's eight replicas {<p,Ap>, seq or seq | kFuseGaveUp}
    unsigned seq;
    int give_up;
};

template <int UNITS>
__global__ __launch_bounds__(HIPK_THREADS) HIPK_SGPR80 void hipk_cg_fuse_update_kernel(hipk_spmv_args a, hipk_cg_fuse_args f) {
    typedef double T;
    constexpr int VEC = hipk_vec<T>::VEC, N0 = HIPK_BASE_CHUNK / (VEC * HIPK_THREADS);
    constexpr unsigned STEP = VEC * HIPK_THREADS;
    static_assert(HIPK_MAX_PARTS / HIPK_THREADS == 8, "the collector's poll: eight words per thread");
    __shared__ double s_pap;
    __shared__ int s_fail;
    hipk_wide_chunk wc;
    if (!hipk_sell_wide_walk<UNITS, HIPK_SPMV_DOT_W, 0, true>(a, &wc)) return;   // padding workgroup, or the stop word has fired
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int c = wc.chunk;
    const int64_t base = (int64_t)c * HIPK_BASE_CHUNK;
    const int lim = (int)((base + HIPK_BASE_CHUNK < a.n) ? HIPK_BASE_CHUNK : a.n - base);   // rows of this chunk (>= 1)
    T *const rb = f.r + base;
    const unsigned o0 = VEC * t;
    const double gamma = f.scal->gamma[a.it & 1];
    if (t == 0) s_fail = 0;
    __syncthreads();   // the tile sums and the staged Ap are complete

    // 2. r, requested before the wait.  (The collector requests it behind its poll, in front of the fold's barriers: the polled
    // words and r together do not fit the 64 vector registers of eight workgroups per CU.)
    T rv[N0][VEC];
    auto request_r = [&]() {
#pragma unroll
        for (int k = 0; k < N0; ++k) {
            const int o = (int)(o0 + k * STEP);
            const int nv = (lim - o < VEC) ? lim - o : VEC;
            if (nv > 0) hipk_ld<T>((const T *)rb, o, nv, rv[k]);
        }
    };
    if (blockIdx.x != 0) request_r();
    // 3. publish
    const hipk_ll_rsrc ws = hipk_ll_make(f.words, (size_t)a.g * 16), cs = hipk_ll_make(f.ctl, kFuseCtlBytes);
    if (wave == 0) {
        const double part = hipk_wave_fold(wc.wsum0, wc.cnt, lane);
        if (lane == 0) {
            hipk_ll_put(ws, (unsigned)c, part, f.seq);
            f.part_pap[c] = part;
        }
    }
    // 4. the collector folds; everybody else waits for one of its replicas
    if (blockIdx.x == 0) {
        double acc = 0.0;
        if (f.give_up) {
            if (t == 0) s_fail = 1;
        } else {
            // (two calls of four words per thread, one ascending sum: eight words in flight per thread took 32 vector registers)
            constexpr int NK = HIPK_MAX_PARTS / HIPK_THREADS / 2;
            acc = hipk_mid_poll<NK>(ws, a.g, f.seq, &s_fail, 1);
            acc = hipk_mid_poll<NK>(ws, a.g - NK * HIPK_THREADS, f.seq, &s_fail, 1, NK * HIPK_THREADS * 16, acc);
        }
        request_r();
        const double pap = hipk_block_sum(acc, wc.free256);   // hipk_reduce_parts' tree; its barriers also publish s_fail
        const int failed = s_fail;
        if (t < 8) hipk_ll_put(cs, (unsigned)t * kFuseReplicaSlots, pap, failed ? (f.seq | kFuseGaveUp) : f.seq);
        if (failed) {
            if (t == 0) {
                f.scal->stop_it = a.it;
                f.scal->ctl.redo = -1;
                hipk_signal(f.scal->host_sig, HIPK_SIG_STOP | a.it);
            }
            return;
        }
        if (t == 0) s_pap = pap;
    } else if (t == 0) {
        const unsigned slot = (blockIdx.x & 7) * kFuseReplicaSlots;
        hipk_v4u w = hipk_ll_load(cs, slot);
        unsigned spins = 0;
        int bad = 0;
        while (!(w.y == w.w && (w.y & ~kFuseGaveUp) == f.seq)) {
            __builtin_amdgcn_s_sleep(1);
            if (++spins > kFuseWaitBound) {   // the collector itself is not running: the launch is void (an error on the host)
                f.scal->ctl.redo = -3;
                f.scal->stop_it = a.it;
                hipk_signal(f.scal->host_sig, HIPK_SIG_STOP | a.it);
                bad = 1;
                break;
            }
            w = hipk_ll_load(cs, slot);
        }
        if (bad || (w.y & kFuseGaveUp)) s_fail = 1;
        s_pap = hipk_ll_val(w);
    }
    __syncthreads();
    if (s_fail) return;   // nothing of this iteration has been stored
    // 5. the update step of hipk_cg_update_kernel on the staged Ap
    const T alpha = (T)(gamma / s_pap);   // TSL:846
    if (c == 0 && t == 0) f.scal->alpha[a.it & 1] = (double)alpha;
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < N0; ++k) {
        const int o = (int)(o0 + k * STEP);
        const int nv = (lim - o < VEC) ? lim - o : VEC;
        if (nv > 0) {
            const double2 ap = *(const double2 *)(wc.stage + o);
            const T av[VEC] = {ap.x, ap.y};
            T out[VEC];
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const T m1 = alpha * av[e];
                out[e] = rv[k][e] - m1;   // TSL:848
                if (e < nv) acc = fma((double)out[e], (double)out[e], acc);   // TSL:850
            }
            hipk_st<T>(rb, o, nv, out);
        }
    }
    acc = hipk_block_sum(acc, wc.free256);
    if (t == 0) f.part_rr[c] = acc;
}
