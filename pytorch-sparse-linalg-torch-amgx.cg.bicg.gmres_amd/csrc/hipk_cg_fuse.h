// hipk_cg_fuse.h -- the CG loop's stencil SpMV, its update step and (x update deferred) its direction step in ONE launch: Ap
// never leaves the chip and r is read once.
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
// With the x update deferred the launch goes on with the DIRECTION step (p_next set; hipk_cg_path_fuse): one launch per iteration.
// Only <r,r> stands between the r update and p = r + beta p, and r_{k+1} is in this thread's registers already:
//   6. every workgroup publishes its <r,r> partial (the value it stores to part_rr[c]) as a flagged word of a SECOND words region
//      (g x 16 bytes and eight replicas of its own, behind the first region's replicas at the head of Ap);
//   7. takes its elements of p_k (the walk's operand) in hipk_cg_dir_chunk's layout: with keep_p the steps whose tile was uniform
//      are in this thread's registers since the walk (hipk_sell_wide_walk's `keep`: the diagonal entry's load) and only the steps
//      of tiles with a grid-line end are requested, before the wait; without it, and in workgroup 0, all of them are.  On an x
//      iteration (every second one: x set) the x part comes here too, x = (x + alpha_{k-1} p_{k-1}) + alpha_k p_k with hipk_cg_dir_chunk's
//      operations and roundings, p_{k-1} read from the buffer that will receive p_{k+1}, one step's x and p_{k-1} at a time (the
//      four operands of four steps do not fit 64 registers); its stores leave before the wait;
//   8. workgroup 0 polls the g words (two per thread in flight, four times: hipk_parts_pre::fold's order, then hipk_block_sum --
//      the bits hipk_cg_pdir_kernel folds; r_{k+1} waits in the staged Ap's LDS meanwhile), hands <r,r> out through its replicas,
//      does hipk_cg_dir_done (the next pass's gamma, the stop test, the host's signal word) and only then its own step 7;
//      everybody else polls replica b & 7 as at the first hand-off;
//   9. beta = (T)(<r,r> / gamma), p_{k+1} = r_{k+1} + beta p_k into the other p buffer.
// Per iteration the tail moves 16 n bytes (p in, p out; 8 n plus the non-uniform tiles' rows with keep_p) where hipk_cg_pdir_kernel
// moves 24 n, and 40 n where hipk_cg_xdir_kernel moves 48 n: r is not read again, and there is no second launch.  When the collector of the second hand-off gives up
// (HIPK_TEST_CG_FUSE_DIR_GIVE_UP) it hands out the give-up mark, sets stop_it = it and ctl.redo = kFuseDirGaveUp: no workgroup
// stores p_{k+1} and hipk_cg_dir_done is not run -- the state is iteration `it` after its update (x included on an x iteration),
// and hipk_cg_steps::fuse_end finishes the iteration with hipk_cg_pdir_kernel.
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
static constexpr int kFuseDirGaveUp = -4;               // ctl.redo: the collector of the SECOND hand-off (the direction tail) gave up
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
    // the direction tail (steps 6-9).  p_next null: none -- the launch ends with step 5 and a direction kernel follows
    double *p_next;     // receives p_{k+1} = r_{k+1} + beta p_k; p_k is the walk's operand (a.x).  On an x iteration it holds p_{k-1}
    double *x;          // not null: an x iteration, x = (x + alpha_{k-1} p_{k-1}) + alpha_k p_k before the second wait
    int64_t maxiter;    // hipk_cg_dir_done's
    int keep_p;         // the tail takes p_k of uniform tiles from the walk's registers (HIPK_CG_FUSE_KEEP_P=0: loads all of it)
    int dir_give_up;    // HIPK_TEST_CG_FUSE_DIR_GIVE_UP: the collector of the SECOND hand-off behaves as if its poll had run out
};

template <int UNITS>
__global__ __launch_bounds__(HIPK_THREADS) HIPK_SGPR80 void hipk_cg_fuse_update_kernel(hipk_spmv_args a, hipk_cg_fuse_args f) {
    typedef double T;
    constexpr int VEC = hipk_vec<T>::VEC, N0 = HIPK_BASE_CHUNK / (VEC * HIPK_THREADS);
    constexpr unsigned STEP = VEC * HIPK_THREADS;
    static_assert(HIPK_MAX_PARTS / HIPK_THREADS == 8, "the collector's poll: eight words per thread");
    static_assert(N0 == HIPK_FUSE_TPC / 2 && VEC == 2, "step k of the tail is the walk's tile 2 k + (wave >> 1), two rows per lane");
    __shared__ double s_pap;
    __shared__ int s_fail;
    hipk_wide_chunk wc;
    T pv[N0][VEC];   // p_k of this thread's elements: the walk leaves the steps of uniform tiles here (wc.kept), step 7 loads the others
    if (!hipk_sell_wide_walk<UNITS, HIPK_SPMV_DOT_W, 0, true>(a, &wc, pv)) return;   // padding workgroup, or the stop word has fired
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
        // (the collector loads all of its p in step 7: the walk's values die here, or they would sit beside the polled words)
#pragma unroll
        for (int k = 0; k < N0; ++k) pv[k][0] = pv[k][1] = (T)0;
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
            T out[VEC];   // (a row of its own: a partial store indexes it by a run-time count, which rv must not be)
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const T m1 = alpha * av[e];
                out[e] = rv[k][e] - m1;   // TSL:848
                if (e < nv) acc = fma((double)out[e], (double)out[e], acc);   // TSL:850
                rv[k][e] = out[e];        // r_{k+1}, which the direction tail finds here
            }
            hipk_st<T>(rb, o, nv, out);
        }
    }
    acc = hipk_block_sum(acc, wc.free256);
    if (t == 0) f.part_rr[c] = acc;
    if (f.p_next == nullptr) return;   // no tail: hipk_cg_pdir_kernel, hipk_cg_xdir_kernel or hipk_cg_direction_kernel folds part_rr

    // ---- the direction tail: the second hand-off carries <r,r>, r_{k+1} stays in rv
    // 6. publish (every thread holds the block's sum); the second region follows the first one's replicas
    char *const region2 = (char *)f.ctl + kFuseCtlBytes;
    const hipk_ll_rsrc ws2 = hipk_ll_make(region2, (size_t)a.g * 16), cs2 = hipk_ll_make(region2 + kFuseWordsBytes, kFuseCtlBytes);
    if (t == 0) hipk_ll_put(ws2, (unsigned)c, acc, f.seq);
    // 7. p_k, requested before the wait; on an x iteration the x part, step by step (x and p_{k-1} of ONE step beside r_{k+1} and
    // p_k: all four operands of four steps would take 64 vector registers), in hipk_cg_dir_chunk<T, true, *>'s operations and order.
    // (The collector does this behind its hand-out: on an x iteration the step ends with stores, and the fold's barriers wait for them.)
    const T *const pb = (const T *)a.x + base;
    T *const qb = f.p_next + base;
    const unsigned kept = (f.keep_p && blockIdx.x != 0) ? wc.kept : 0u;   // (a kept step is a whole tile: nv = VEC)
    auto request_p = [&]() {
#pragma unroll
        for (int k = 0; k < N0; ++k) {
            const int o = (int)(o0 + k * STEP);
            const int nv = (lim - o < VEC) ? lim - o : VEC;
            if (nv > 0 && !((kept >> k) & 1u)) hipk_ld<T>(pb, o, nv, pv[k]);
        }
        if (f.x != nullptr) {
            T *const xb = f.x + base;
            const T alpha_prev = (T)f.scal->alpha[(a.it - 1) & 1];
#pragma unroll
            for (int k = 0; k < N0; ++k) {
                const int o = (int)(o0 + k * STEP);
                const int nv = (lim - o < VEC) ? lim - o : VEC;
                if (nv > 0) {
                    T xv[VEC], qv[VEC];
                    hipk_ld<T>((const T *)xb, o, nv, xv);
                    hipk_ld<T>((const T *)qb, o, nv, qv);
#pragma unroll
                    for (int e = 0; e < VEC; ++e) {
                        const T m0 = alpha_prev * qv[e];
                        const T x1 = xv[e] + m0;   // TSL:847 of iteration it - 1
                        const T m1 = alpha * pv[k][e];
                        xv[e] = x1 + m1;           // TSL:847 of iteration it
                    }
                    hipk_st<T>(xb, o, nv, xv);
                }
            }
        }
    };
    // 8. the collector folds <r,r> (hipk_parts_pre::fold's bits) and does the bookkeeping of a direction kernel
    if (blockIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < N0; ++k) pv[k][0] = pv[k][1] = (T)0;   // (as at the first hand-off: nothing of p lives across the poll)
        // (the polled words beside r_{k+1} do not fit the 64 vector registers: r_{k+1} waits in the staged Ap's place, which step
        // 5 has read -- every thread its own elements, so no barrier)
#pragma unroll
        for (int k = 0; k < N0; ++k) *(double2 *)(wc.stage + o0 + k * STEP) = make_double2(rv[k][0], rv[k][1]);
        asm volatile("" ::: "memory");   // (a compiler barrier: the reload below must come from LDS, not from values kept in registers)
        double s = 0.0;
        if (f.dir_give_up) {
            if (t == 0) s_fail = 1;
        } else {
            // (four calls of two words per thread, one ascending sum: the registers of the first hand-off's four are not free here)
            constexpr int NK = HIPK_MAX_PARTS / HIPK_THREADS / 4;
#pragma unroll
            for (int q = 0; q < 4; ++q) s = hipk_mid_poll<NK>(ws2, a.g - q * NK * HIPK_THREADS, f.seq, &s_fail, 1, q * NK * HIPK_THREADS * 16, s);
        }
        const double rr = hipk_block_sum(s, wc.free256);
        const int failed = s_fail;
        if (t < 8) hipk_ll_put(cs2, (unsigned)t * kFuseReplicaSlots, rr, failed ? (f.seq | kFuseGaveUp) : f.seq);
        if (t == 0) {
            if (failed) {   // iteration `it` after its update (x included, on an x iteration): no workgroup stores p_{k+1}
                f.scal->stop_it = a.it;
                // (a workgroup whose wait at the FIRST hand-off ran out has not updated its r and published nothing here: its -3 stays)
                if (__hip_atomic_load(&f.scal->ctl.redo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != -3) f.scal->ctl.redo = kFuseDirGaveUp;
                hipk_signal(f.scal->host_sig, HIPK_SIG_STOP | a.it);
            } else {
                s_pap = rr;
                hipk_cg_dir_done(f.scal, a.it, f.maxiter, rr);
            }
        }
        // its own chunk last (the x part also when it has given up): the whole grid waits for the replicas, nobody for this
        request_p();
#pragma unroll
        for (int k = 0; k < N0; ++k) {
            const double2 rk = *(const double2 *)(wc.stage + o0 + k * STEP);
            rv[k][0] = rk.x;
            rv[k][1] = rk.y;
        }
    } else {
        request_p();
        if (t == 0) {
            const unsigned slot = (blockIdx.x & 7) * kFuseReplicaSlots;
            hipk_v4u w = hipk_ll_load(cs2, slot);
            unsigned spins = 0;
            int bad = 0;
            while (!(w.y == w.w && (w.y & ~kFuseGaveUp) == f.seq)) {
                __builtin_amdgcn_s_sleep(1);
                if (++spins > kFuseWaitBound) {
                    f.scal->ctl.redo = -3;
                    f.scal->stop_it = a.it;
                    hipk_signal(f.scal->host_sig, HIPK_SIG_STOP | a.it);
                    bad = 1;
                    break;
                }
                w = hipk_ll_load(cs2, slot);
            }
            if (bad || (w.y & kFuseGaveUp)) s_fail = 1;
            s_pap = hipk_ll_val(w);
        }
    }
    __syncthreads();
    if (s_fail) return;
    // 9. p_{k+1} = r_{k+1} + beta p_k into the other buffer
    const T beta = (T)(s_pap / gamma);   // TSL:851
#pragma unroll
    for (int k = 0; k < N0; ++k) {
        const int o = (int)(o0 + k * STEP);
        const int nv = (lim - o < VEC) ? lim - o : VEC;
        if (nv > 0) {
            T pn[VEC];
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const T m = beta * pv[k][e];
                pn[e] = rv[k][e] + m;   // TSL:852
            }
            hipk_st<T>(qb, o, nv, pn);
        }
    }
}
