// hipk_cg_fuse.h -- the CG loop's stencil SpMV, its update step and (x update deferred) its direction step in ONE launch: Ap
// never leaves the chip and r is read once.
//
// The three-launch iteration writes Ap (8 n bytes) in the SpMV and reads it back in the update kernel, and nobody else reads it.
// Both kernels run one workgroup per reduction chunk and the same rows belong to the same chunk in both; only the scalar
// alpha = gamma / <p,Ap> stands between them, and that needs every chunk's partial.  Here a workgroup
//   1. walks its chunk's tiles as hipk_spmv_sell_wide_kernel does (hipk_sell_wide_walk, FUSE: the same code), Ap staying in LDS
//      (16 KB, indexed by the row's place in the chunk) and the chunk's <p,Ap> partial folded as there (hipk_wave_fold): same bits;
//   2. requests its chunk of r in hipk_cg_update_kernel's per-thread layout (16-byte accesses, thread t, steps of 512 elements);
//   3. publishes the partial as a flagged 16-byte word {value, seq} (hipk_ll_put, hipk_mid.h) -- nobody waits before this.  Chunk c's
//      word lies at slot (c mod 8) * 256 + c / 8 (hipk_fuse_word_slot): the words of a residue class are contiguous;
//   4. the eight workgroups dispatched first (blockIdx.x < 8, one per XCD; ordinary workgroups otherwise, with chunks of their own)
//      are the COLLECTORS.  The spec's fold (hipk_reduce_parts, hipk_block_sum: thread t of 256 sums words t, t + 256, ... ascending,
//      then the tree with strides 128 ... 1) splits eight ways without changing a bit: the strides >= 8 stay inside t mod 8, so
//      collector s polls class s, ONE word per thread and one round trip (hipk_fuse_class_sum: thread 32 i + j the word of chunk
//      s + 8 j + 256 i), and after one barrier 32 lanes run the chains and the halving tree over j.  It hands {class sum, seq} out
//      in slot s of eight 128-byte lines.  Every workgroup b, the collectors included, waits on line b & 7: eight lanes load its
//      eight slots with one instruction until all carry seq, and the strides 4, 2, 1 follow as lane reads (hipk_fuse_wait):
//      ((c0 + c4) + (c2 + c6)) + ((c1 + c5) + (c3 + c7)) -- the bits every workgroup of hipk_cg_update_kernel derives.  (Relaxed
//      loads: hipk_fx.h records what an acquire per poll and what every workgroup polling every partial cost.  With ONE collector
//      polling eight words per thread the poll was two to four serial round trips and the fold hipk_block_sum's four barriers, on
//      the path the whole chip waits on; with the words in chunk order, every lane of a collector's poll read a 128-byte line of
//      its own and the form was slower than the one collector at N = 4 M: profiles/cg_fuse_collectors_ab.md);
//   5. alpha = (T)(gamma / <p,Ap>), r -= alpha Ap with Ap from LDS, <r,r> in the update kernel's element order, hipk_block_sum,
//      part_rr[c]: the bits hipk_cg_update_kernel stores.  One thread leaves alpha in the scalar block for the deferred x update.
// With the x update deferred the launch goes on with the DIRECTION step (p_next set; hipk_cg_path_fuse): one launch per iteration.
// Only <r,r> stands between the r update and p = r + beta p, and r_{k+1} is in this thread's registers already:
//   6. every workgroup publishes its <r,r> partial (the value it stores to part_rr[c]) as a flagged word of a SECOND words region
//      (laid out as the first, with eight lines of its own, behind the first region's lines at the head of Ap);
//   7. takes its elements of p_k (the walk's operand) in hipk_cg_dir_chunk's layout: with keep_p the steps whose tile was uniform
//      are in this thread's registers since the walk (hipk_sell_wide_walk's `keep`: the diagonal entry's load) and only the steps
//      of tiles with a grid-line end are requested, before the wait; without it all of them are.  On an x iteration (every second
//      one: x set) the x part comes here too, x = (x + alpha_{k-1} p_{k-1}) + alpha_k p_k with hipk_cg_dir_chunk's
//      operations and roundings, p_{k-1} read from the buffer that will receive p_{k+1}, one step's x and p_{k-1} at a time (the
//      four operands of four steps do not fit 64 registers); its stores leave before the wait;
//   8. the collectors fold the second region's words as in step 4 (hipk_parts_pre::fold's order, then hipk_block_sum's tree: the
//      bits hipk_cg_pdir_kernel folds) and hand the class sums out through the region's eight lines -- in front of their own step
//      7: loads return in order and stores are counted with them, so whatever a collector requests in front of its poll stands
//      between the last word's arrival and the whole chip.  Every workgroup waits on line b & 7 as at the first hand-off; thread 0
//      of workgroup 0 does hipk_cg_dir_done (the next pass's gamma, the stop test, the host's signal word) with the <r,r> it has
//      received;
//   9. beta = (T)(<r,r> / gamma), p_{k+1} = r_{k+1} + beta p_k into the other p buffer.
// Per iteration the tail moves 16 n bytes (p in, p out; 8 n plus the non-uniform tiles' rows with keep_p) where hipk_cg_pdir_kernel
// moves 24 n, and 40 n where hipk_cg_xdir_kernel moves 48 n: r is not read again, and there is no second launch.
// Every flagged word validates itself ({lo, seq, hi, seq}), so the value needs no flag of its own and no drain in between.
// seq = iterations since the sequence began + 1: different in every launch of a solve; the host clears the words when the
// sequence begins, so a workspace of any content gives the same solve.
// The g workgroups must be resident together (the host checks g against the occupancy of this kernel; <= 80 SGPRs, <= 64 VGPRs
// and <= 20 KB of LDS by construction: eight workgroups per CU; g > 512, so all eight collectors have a chunk).  Every wait is
// bounded.  GIVING UP: a collector whose poll runs out (a workgroup of the launch is not running) writes the give-up mark instead
// of seq into its slot of all eight lines and sets stop_it = it, ctl.redo and the host's signal word (the same words from every
// collector that does).  A workgroup that finds the mark in ANY slot of its line stores nothing of that hand-off's step:
//   first hand-off (ctl.redo = -1): no workgroup has stored r, part_rr or alpha, the state is that of iteration `it`;
//   second hand-off (ctl.redo = kFuseDirGaveUp): no workgroup stores p_{k+1} and hipk_cg_dir_done is not run -- the state is
//   iteration `it` after its update (x included on an x iteration), and hipk_cg_steps::fuse_end finishes it with hipk_cg_pdir_kernel.
// The host goes on from there with the separate kernels (hipk_cg_steps::fuse_end).  give_up (HIPK_TEST_CG_FUSE_GIVE_UP,
// HIPK_TEST_CG_FUSE_DIR_GIVE_UP; HIPK_TEST_CG_FUSE_GIVE_UP_WHO = s: collector s alone): the collectors named behave as if their
// poll had run out, without waiting.
#pragma once
#include "hipk_coded.h"
#include "hipk_mid.h"

static constexpr unsigned kFuseGaveUp = 0x80000000u;   // in a hand-out slot's seq: its collector gave up (seq itself stays below 2^31)
static constexpr unsigned kFuseCollectors = 8;         // workgroups 0 .. 7, one per XCD: collector s folds residue class s of a hand-off's words
static constexpr unsigned kFuseReplicaSlots = 8;       // a hand-out line: 8 slots of 16 bytes = 128 bytes, slot s collector s's; eight lines
static constexpr size_t kFuseCtlBytes = 8 * 128;
static constexpr size_t kFuseWordsBytes = (size_t)HIPK_MAX_PARTS * 16;
static constexpr int kFuseDirGaveUp = -4;               // ctl.redo: a collector of the SECOND hand-off (the direction tail) gave up
// where chunk c publishes its flagged word: class c mod 8 is contiguous (256 slots each), so that a collector's wavefront polls
// eight 128-byte lines, not sixty-four (with the words in chunk order every lane of it read a line of its own)
__host__ __device__ constexpr unsigned hipk_fuse_word_slot(unsigned c) { return (c % kFuseCollectors) * HIPK_THREADS + c / kFuseCollectors; }
static constexpr unsigned kFuseWaitBound = 1u << 24;   // polls of a line (well beyond a collector's own bound, kMidSpinBound)

struct hipk_cg_fuse_args {
    hipk_cg_scal *scal;
    double *r;
    double *part_rr;
    double *part_pap;   // the plain <p,Ap> partials as the SpMV leaves them: hipk_cg_direction_kernel folds them (HIPK_CG_DEFER_X=0)
    void *words;     // g flagged words: {<p,Ap> partial of chunk c, seq} at slot hipk_fuse_word_slot(c); kFuseWordsBytes on, the collectors' eight lines:
                     // slot s of each {class sum s of <p,Ap>, seq or seq | kFuseGaveUp}
    unsigned seq;
    int give_up;     // bit s: collector s behaves as if its poll had run out (HIPK_TEST_CG_FUSE_GIVE_UP); bit 8 + s: the same at the
                     // SECOND hand-off (HIPK_TEST_CG_FUSE_DIR_GIVE_UP).  (One word: the scalar registers are counted, hipk_common.h)
    // the direction tail (steps 6-9).  p_next null: none -- the launch ends with step 5 and a direction kernel follows
    double *p_next;     // receives p_{k+1} = r_{k+1} + beta p_k; p_k is the walk's operand (a.x).  On an x iteration it holds p_{k-1}
    double *x;          // not null: an x iteration, x = (x + alpha_{k-1} p_{k-1}) + alpha_k p_k before the second wait
    int64_t maxiter;    // hipk_cg_dir_done's
    int keep_p;         // the tail takes p_k of uniform tiles from the walk's registers (HIPK_CG_FUSE_KEEP_P=0: loads all of it)
};

// Collector s of a hand-off: the sum of residue class s of the spec's fold (hipk_reduce_parts, then hipk_block_sum).  The fold's
// virtual thread t sums words t, t + 256, ... ascending and the tree pairs t with t + 128, 64, ... 8 -- strides that stay inside
// t mod 8 -- so class s is the threads t = s + 8 j, j = 0 .. 31, and its part of the tree the halving tree over j (hipk_half_sum).
// Thread u = 32 i + j polls the ONE word of chunk s + 8 j + 256 i -- slot u of the class's 256 (hipk_fuse_word_slot) -- and after
// one barrier lanes j of wavefront 0 run thread t's chain over i.
// Valid in lane 0 of wavefront 0, where *fail is current too.  skip: behave as if the poll had run out, without waiting.
__device__ __forceinline__ double hipk_fuse_class_sum(hipk_ll_rsrc ws, int g, unsigned seq, int s, int skip, int *fail, double *sb) {
    const int u = threadIdx.x, j = u & 31;
    const int mine = s + 8 * j + (u >> 5) * 256;
    if (skip) {
        if (u == 0) *fail = 1;
    } else if (mine < g) {
        double v = 0.0;
        const unsigned slot = hipk_fuse_word_slot((unsigned)mine);
        if (!hipk_ll_wait(ws, slot, seq, hipk_ll_load(ws, slot), v)) *fail = 1;
        sb[u] = v;
    }
    __syncthreads();
    double acc = 0.0;
    if (u < 64) {
        if (!skip) {
#pragma unroll
            for (int i = 0; i < HIPK_MAX_PARTS / HIPK_THREADS; ++i)
                if (s + 8 * j + i * 256 < g) acc = acc + sb[32 * i + j];
        }
        acc = hipk_half_sum(acc);
    }
    return acc;
}
// ... and its hand-out: {class sum, seq} -- or the give-up mark -- into slot s of all eight lines (wavefront 0 calls)
__device__ __forceinline__ void hipk_fuse_hand_out(hipk_ll_rsrc cs, int s, double sum, unsigned seq, int failed, int lane) {
    const double v = __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(sum)), __builtin_amdgcn_readfirstlane(__double2loint(sum)));
    if (lane < (int)kFuseCollectors) hipk_ll_put(cs, (unsigned)lane * kFuseReplicaSlots + (unsigned)s, v, failed ? (seq | kFuseGaveUp) : seq);
}
// Every workgroup's wait (wavefront 0 calls, all lanes): lanes 0 .. 7 load the eight slots of line `line` -- one instruction on one
// 128-byte line -- until all eight carry seq or one carries the give-up mark; the strides 4, 2, 1 of the spec's tree follow as lane
// reads: ((c0 + c4) + (c2 + c6)) + ((c1 + c5) + (c3 + c7)) in lane 0.  *fail set (by lane 0) when a collector gave up or never
// arrived; the latter voids the launch (ctl.redo = -3, an error on the host).
__device__ __forceinline__ double hipk_fuse_wait(hipk_ll_rsrc cs, unsigned line, unsigned seq, hipk_cg_scal *scal, int64_t it, int lane, int *fail) {
    const unsigned slot = line * kFuseReplicaSlots + (unsigned)(lane & 7);
    hipk_v4u w = {0u, 0u, 0u, 0u};
    unsigned spins = 0;
    int bad = 0;
    for (;;) {
        if (lane < (int)kFuseCollectors) w = hipk_ll_load(cs, slot);
        const bool whole = lane < (int)kFuseCollectors && w.y == w.w && (w.y & ~kFuseGaveUp) == seq;
        if (__ballot(whole && (w.y & kFuseGaveUp)) != 0ull) {
            bad = 1;
            break;
        }
        if ((__ballot(whole) & 0xFFull) == 0xFFull) break;
        __builtin_amdgcn_s_sleep(1);
        if (++spins > kFuseWaitBound) {   // a collector is not running: the launch is void
            if (lane == 0) {
                scal->ctl.redo = -3;
                scal->stop_it = it;
                hipk_signal(scal->host_sig, HIPK_SIG_STOP | it);
            }
            bad = 1;
            break;
        }
    }
    if (bad && lane == 0) *fail = 1;
    double v = hipk_ll_val(w);
    v = v + hipk_row_shl<4>(v);
    v = v + hipk_row_shl<2>(v);
    v = v + hipk_row_shl<1>(v);
    return v;
}

template <int UNITS>
__global__ __launch_bounds__(HIPK_THREADS) HIPK_SGPR80 void hipk_cg_fuse_update_kernel(hipk_spmv_args a, hipk_cg_fuse_args f) {
    typedef double T;
    constexpr int VEC = hipk_vec<T>::VEC, N0 = HIPK_BASE_CHUNK / (VEC * HIPK_THREADS);
    constexpr unsigned STEP = VEC * HIPK_THREADS;
    static_assert(HIPK_MAX_PARTS == kFuseCollectors * HIPK_THREADS, "a collector's poll: one word per thread");
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

    // 2. r, requested before the wait
    const bool collector = blockIdx.x < kFuseCollectors;
    const unsigned line = blockIdx.x & 7;
    T rv[N0][VEC];
#pragma unroll
    for (int k = 0; k < N0; ++k) {
        const int o = (int)(o0 + k * STEP);
        const int nv = (lim - o < VEC) ? lim - o : VEC;
        if (nv > 0) hipk_ld<T>((const T *)rb, o, nv, rv[k]);
    }
    // 3. publish
    const hipk_ll_rsrc ws = hipk_ll_make(f.words, kFuseWordsBytes), cs = hipk_ll_make((char *)f.words + kFuseWordsBytes, kFuseCtlBytes);
    if (wave == 0) {
        const double part = hipk_wave_fold(wc.wsum0, wc.cnt, lane);
        if (lane == 0) {
            hipk_ll_put(ws, hipk_fuse_word_slot((unsigned)c), part, f.seq);
            f.part_pap[c] = part;
        }
    }
    // 4. the collectors fold a class each and hand it out; everybody waits for the eight class sums of one line
    if (collector) {   // (in wavefront 0 the thread index is the lane)
        const int cls = (int)blockIdx.x;
        const double sum = hipk_fuse_class_sum(ws, a.g, f.seq, cls, (f.give_up >> cls) & 1, &s_fail, wc.free256);
        if (wave == 0) {
            const int failed = s_fail;
            hipk_fuse_hand_out(cs, cls, sum, f.seq, failed, t);
            if (failed && t == 0) {   // (the same words from every collector that gives up)
                f.scal->stop_it = a.it;
                f.scal->ctl.redo = -1;
                hipk_signal(f.scal->host_sig, HIPK_SIG_STOP | a.it);
            }
        }
    }
    if (wave == 0) {
        const double pap = hipk_fuse_wait(cs, line, f.seq, f.scal, a.it, t, &s_fail);
        if (t == 0) s_pap = pap;
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
    char *const region2 = (char *)f.words + kFuseWordsBytes + kFuseCtlBytes;
    const hipk_ll_rsrc ws2 = hipk_ll_make(region2, kFuseWordsBytes), cs2 = hipk_ll_make(region2 + kFuseWordsBytes, kFuseCtlBytes);
    if (t == 0) hipk_ll_put(ws2, hipk_fuse_word_slot((unsigned)c), acc, f.seq);
    // 8. the collectors fold a class of the <r,r> words each (hipk_parts_pre::fold's bits) and hand it out -- in front of their step
    // 7 and of the x part: the whole grid waits for this poll, which returns behind every request in front of it
    if (collector) {
        const int cls = (int)blockIdx.x;
        const double sum = hipk_fuse_class_sum(ws2, a.g, f.seq, cls, (f.give_up >> (8 + cls)) & 1, &s_fail, wc.free256);
        if (wave == 0) {
            const int failed = s_fail;
            hipk_fuse_hand_out(cs2, cls, sum, f.seq, failed, t);
            if (failed && t == 0) {   // iteration `it` after its update (x included, on an x iteration): no workgroup stores p_{k+1}
                f.scal->stop_it = a.it;
                // (a workgroup whose wait at the FIRST hand-off ran out has not updated its r and published nothing here: its -3 stays)
                if (__hip_atomic_load(&f.scal->ctl.redo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != -3) f.scal->ctl.redo = kFuseDirGaveUp;
                hipk_signal(f.scal->host_sig, HIPK_SIG_STOP | a.it);
            }
        }
    }
    // 7. p_k of the steps the walk did not keep, requested before the wait (a kept step is a whole tile: nv = VEC)
    const T *const pb = (const T *)a.x + base;
    T *const qb = f.p_next + base;
    const unsigned kept = f.keep_p ? wc.kept : 0u;
#pragma unroll
    for (int k = 0; k < N0; ++k) {
        const int o = (int)(o0 + k * STEP);
        const int nv = (lim - o < VEC) ? lim - o : VEC;
        if (nv > 0 && !((kept >> k) & 1u)) hipk_ld<T>(pb, o, nv, pv[k]);
    }
    // on an x iteration the x part (also when a collector has given up), step by step (x and p_{k-1} of ONE step beside r_{k+1} and
    // p_k: all four operands of four steps would take 64 vector registers), in hipk_cg_dir_chunk<T, true, *>'s operations and order
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
    // everybody waits for the eight class sums; workgroup 0 does the bookkeeping of a direction kernel with what it has received
    if (wave == 0) {
        const double rr = hipk_fuse_wait(cs2, line, f.seq, f.scal, a.it, t, &s_fail);
        if (t == 0) {
            s_pap = rr;
            if (blockIdx.x == 0 && !s_fail) hipk_cg_dir_done(f.scal, a.it, f.maxiter, rr);
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
