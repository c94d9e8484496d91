// hipk_dist.hip -- row-partitioned CG, the per-iteration loop driven from C (one rank of it).
//
// New against the reference, which is single-process / single-device; the algorithm is `cg`
// (TSL:806-856 via `_isolve`, TSL:968-1016) on the SAME fused kernels as the single-GPU solve (include/hipk.h, step API).
// Between launches the ranks exchange, on the solver's stream, only
//   (1) the chunk partial sums of <p,Ap>                        : all-gather, <= 2048 doubles in total
//   (2) the chunk partial sums of <r,r> AND the halo entries of r: ONE group (all-gather + the halo, either neighbour
//       send/recv pairs or a second all-gather of padded slabs); every rank then forms the halo entries of
//       p = r + beta p and x += alpha p itself (same operands, same bits as the owner)
// so an iteration has two collective launches, the minimum for CG's two reductions.  Every rank folds the gathered
// partials in the same fixed order: the iterates are bitwise those of the single-GPU solve for any rank count.
//
// The loop used to be Python (pytorch_sparse_solver/distributed.py: 7 ctypes calls of ~4 us each per iteration -- host
// bound at 4 M rows per rank).  Here the host enqueues fixed BATCHES of iterations and learns the stop from a
// stream-ordered read of the device stop word one batch late (two reads in flight): all ranks derive the same stop word
// from the same gathered partials, so they take the same decision at the same batch boundary without talking to each
// other, and the number of collectives issued is identical on every rank (iterations past the stop are no-ops on the
// device; their collectives still pair up).  The RCCL entry points come in as function pointers resolved from the
// librccl that created the communicator (no link-time dependency; tests plug host-staged stand-ins in).
//
// The exchanges and the batch loop are shared with the other five row-partitioned loops (csrc/hipk_dist_xchg.h), the workspace
// carver with every solve (csrc/hipk_solve.h); their argument checks, hipk_dist_check, are defined here.
#include <stdlib.h>

#include "hipk_dist_xchg.h"
#include "hipk_fx.h"

struct hipk_dist_layout {
    size_t scal, part_loc, spare, g_pAp, g_rr, g_bb, out4, fx_loc, send_buf, slab_loc, slab_all, p, r, Ap, total;
};

static hipk_dist_layout hipk_dist_make_layout(const hipk_dist_plan *pl) {
    hipk_dist_layout L;
    hipk_carve take;
    const size_t per = (size_t)pl->per, W = (size_t)pl->world;
    const size_t next = (size_t)(pl->n_ext > 0 ? pl->n_ext : 1), nloc = (size_t)(pl->n_local > 0 ? pl->n_local : 1);
    L.scal = take(256);
    L.part_loc = take(per * 8);
    L.spare = take(per * 8);
    L.g_pAp = take(W * per * 8);
    L.g_rr = take(W * per * 8);
    L.g_bb = take(W * per * 8);
    L.out4 = take(4 * 8);
    L.fx_loc = take(256 + 2 * 8 * 128);   // fused exchanges: the collector's scalars [2][2] + sequence flags [2][8 replicas x 128 B]
    L.send_buf = take((size_t)(pl->n_send > 0 ? pl->n_send : 1) * 8);
    L.slab_loc = take((size_t)(pl->slab > 0 ? pl->slab : 1) * 8);
    L.slab_all = take((size_t)(pl->slab > 0 ? pl->slab : 1) * W * 8);
    L.p = take(next * 8);
    L.r = take(next * 8);
    L.Ap = take(nloc * 8);
    L.total = take.o;
    return L;
}

extern "C" size_t hipk_dist_cg_work_bytes(const hipk_dist_plan *plan) {
    if (!plan || plan->world < 1 || plan->per < 1) return 0;
    return hipk_dist_make_layout(plan).total;
}

int hipk_dist_check(const hipk_csr_s *A, const hipk_dist_plan *pl, const hipk_rccl *cc, bool pre, const void *dinv,
                    const void *b_local, const void *x_ext, const void *work, const hipk_params *prm, const hipk_stats *st,
                    const char *geometry) {
    HIPK_REQUIRE(A && pl && cc && (dinv || !pre) && b_local && x_ext && work && prm && st, HIPK_ERR_ARG, "null argument");
    HIPK_REQUIRE(A->dtype == HIPK_F64, HIPK_ERR_UNSUPPORTED, "the row-partitioned solver is fp64");
    HIPK_REQUIRE(pl->world >= 1 && pl->rank >= 0 && pl->rank < pl->world, HIPK_ERR_ARG, "rank / world");
    HIPK_REQUIRE(pl->n_local > 0 && pl->n_local == A->n_rows && pl->n_ext >= pl->n_local, HIPK_ERR_ARG,
                 "every rank must own rows (n_local > 0) and n_ext >= n_local");
    HIPK_REQUIRE(pl->per >= 1 && (int64_t)pl->per * pl->world >= pl->g_red && pl->g_red >= 1 && pl->g_red <= HIPK_MAX_PARTS,
                 HIPK_ERR_ARG, geometry ? geometry : "partial-sum geometry");
    HIPK_REQUIRE((pl->n_local + pl->chunk_rows - 1) / pl->chunk_rows <= pl->per, HIPK_ERR_ARG, "more local chunks than `per`");
    HIPK_REQUIRE(cc->all_gather && cc->group_start && cc->group_end && (pl->world == 1 || pl->halo_mode == 0 || (cc->send && cc->recv)),
                 HIPK_ERR_ARG, "missing collective entry points");
    HIPK_REQUIRE((((uintptr_t)work) & 255u) == 0 && hipk_aligned16(x_ext) && hipk_aligned16(b_local) && (!pre || hipk_aligned16(dinv)),
                 HIPK_ERR_ALIGN, pre ? "work must be 256-byte, x / b / dinv 16-byte aligned" : "work must be 256-byte, x / b 16-byte aligned");
    return HIPK_OK;
}

extern "C" int hipk_dist_cg_solve(hipk_csr_t A, const hipk_dist_plan *pl, const hipk_rccl *cc, const void *b_local,
                                  void *x_ext, void *work, size_t work_bytes, const hipk_params *prm, hipk_stats *st,
                                  hipk_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    HIPK_TRY(hipk_dist_check(A, pl, cc, false, nullptr, b_local, x_ext, work, prm, st));
    const hipk_dist_layout L = hipk_dist_make_layout(pl);
    HIPK_REQUIRE(work_bytes >= L.total, HIPK_ERR_WORKSPACE, "work too small");
    memset(st, 0, sizeof(*st));

    char *wk = (char *)work;
    void *scal = wk + L.scal;
    double *part_loc = (double *)(wk + L.part_loc), *spare = (double *)(wk + L.spare);
    double *g_pAp = (double *)(wk + L.g_pAp), *g_rr = (double *)(wk + L.g_rr), *g_bb = (double *)(wk + L.g_bb);
    double *out4 = (double *)(wk + L.out4);
    double *p = (double *)(wk + L.p), *r = (double *)(wk + L.r), *Ap = (double *)(wk + L.Ap);
    double *x = (double *)x_ext;
    const double *b = (const double *)b_local;
    const int64_t n = pl->n_local, n_ext = pl->n_ext;
    const int ch = pl->chunk_rows, G = pl->g_red, per = pl->per, W = pl->world;
    const int64_t *stop_dev = (const int64_t *)((char *)scal + 48);   // hipk_cg_scal::stop_it
    const int64_t maxiter = hipk_default_maxiter(prm, pl->n_global);
    const hipk_dist_xchg xc(pl, cc, stream, (double *)(wk + L.send_buf), (double *)(wk + L.slab_loc), (double *)(wk + L.slab_all),
                            "hipk_dist_cg_solve");

    hipk_event_pair whole;
    HIPK_CHECK_HIP(whole.create());
    HIPK_CHECK_HIP(hipEventRecord(whole.a, stream));
    HIPK_CHECK_HIP(hipMemsetAsync(wk, 0, L.p, stream));                                   // scalars, partial slots, pack buffers
    HIPK_CHECK_HIP(hipMemsetAsync(p, 0, (size_t)n_ext * 8, stream));
    HIPK_CHECK_HIP(hipMemsetAsync(r, 0, (size_t)n_ext * 8, stream));
    if (n_ext > n) HIPK_CHECK_HIP(hipMemsetAsync(x + n, 0, (size_t)(n_ext - n) * 8, stream));

    // ---- r0 = b - A x0, <r0,r0>; <b,b> (TSL:815-826); halos of x and r0 explicitly once
    HIPK_TRY(xc.run(x));
    HIPK_TRY(hipk_spmv_ex(A, x, r, HIPK_SPMV_RESID | HIPK_SPMV_DOT_YY, nullptr, b, spare, part_loc, nullptr, 0, stream));
    HIPK_TRY(xc.parts(part_loc, g_rr));
    HIPK_TRY(hipk_dot_parts(n, ch, b, b, HIPK_F64, part_loc, stream));
    HIPK_TRY(xc.parts(part_loc, g_bb));
    HIPK_TRY(xc.run(r));
    HIPK_TRY(hipk_cg_start(n, ch, G, scal, g_rr, g_bb, r, p, HIPK_F64, prm->tol, prm->atol, maxiter, stream));
    if (n_ext > n)   // p0 = r0 on the halo as well
        HIPK_CHECK_HIP(hipMemcpyAsync(p + n, r + n, (size_t)(n_ext - n) * 8, hipMemcpyDeviceToDevice, stream));

    // ---- the loop: fixed batches, the stop word read one batch late (hipk_dist_batches)
    int64_t it = 0, stop = INT64_MAX;
    // HIPK_DIST_OVERLAP=1 (opt-in): x += alpha p leaves the direction kernel and runs on a SIDE STREAM while the second collective
    // of the iteration (the <r,r> partials + the halo of r) is in flight -- it needs alpha (first collective) and the old p only;
    // the direction kernel then streams 24 n instead of 40 n bytes behind the collective.  Same operands, same bits.  Not the
    // default: the two cross-stream event dependencies per iteration cost more than the 9 us they can hide (world-1 rehearsal
    // at 4 M rows: 98 us per iteration against 66 fused).
    const bool overlap = hipk_sw_int("HIPK_DIST_OVERLAP", 0) != 0;
    hipStream_t side = nullptr;
    hipEvent_t ev_upd = nullptr, ev_x = nullptr;
    if (overlap) {
        HIPK_CHECK_HIP(hipStreamCreateWithFlags(&side, hipStreamNonBlocking));
        HIPK_CHECK_HIP(hipEventCreateWithFlags(&ev_upd, hipEventDisableTiming));
        HIPK_CHECK_HIP(hipEventCreateWithFlags(&ev_x, hipEventDisableTiming));
    }
    struct side_guard {   // every exit path releases the side stream and its events
        hipStream_t &s;
        hipEvent_t &a, &b;
        ~side_guard() {
            if (s) {
                (void)hipStreamSynchronize(s);
                (void)hipStreamDestroy(s);
            }
            if (a) (void)hipEventDestroy(a);
            if (b) (void)hipEventDestroy(b);
        }
    } side_release{side, ev_upd, ev_x};
    // FUSED exchanges (hipk_fx.h): with a mailbox communicator that carries a fused area (hipk_rccl.fused) the two exchanges of an
    // iteration are made by the update / direction kernels themselves -- three launches per iteration, as on one device.
    // HIPK_DIST_FUSED=0 keeps the collective entry points.
    hipk_fx fx;
    unsigned long long fx_seq0 = 0;
    bool fused = cc->fused != nullptr && hipk_sw_enabled("HIPK_DIST_FUSED") && !overlap && (W == 1 || (pl->send_off_dev && pl->dest_off_dev)) &&
                 hipk_p2p_fx_begin((hipk_p2p_s *)cc->fused, per, pl->n_ghost, &fx, &fx_seq0) != 0;
    if (fused) {
        fx.send_idx = pl->send_idx_dev;
        fx.send_off = pl->send_off_dev;
        fx.dest_off = (const long long *)pl->dest_off_dev;
        fx.n_ghost = pl->n_ghost;
        fx.loc_val = (double *)(wk + L.fx_loc);
        fx.loc_flag = (unsigned long long *)(wk + L.fx_loc + 256);
        // (zeroed with the rest of the workspace header above: below every sequence number, which start at 1 and only grow)
    }
    struct fx_guard {   // every exit path tells the communicator how many exchanges were issued
        const hipk_rccl *cc;
        const bool &on;
        const int64_t &it;
        ~fx_guard() {
            if (on) hipk_p2p_fx_end((hipk_p2p_s *)cc->fused, (unsigned long long)it);
        }
    } fx_release{cc, fused, it};
    HIPK_TRY(hipk_dist_batches(prm, A->host_poll, stop_dev, maxiter, stream, it, stop, [&](int64_t it) -> int {
        HIPK_TRY(hipk_spmv_ex(A, p, Ap, HIPK_SPMV_DOT_W, p, nullptr, part_loc, spare, stop_dev, it, stream));
        if (fused) {
            fx.seq = fx_seq0 + (unsigned long long)it;
            fx.ch = (int)(it & 1);
            fx.kind = 0;
            fx.parts = part_loc;     // <p,Ap> partials of this rank's chunks (the SpMV's)
            fx.vec = nullptr;
            HIPK_TRY(hipk_cg_update_fx(n, ch, G, scal, it, Ap, r, spare, &fx, stream));
            fx.kind = 1;
            fx.parts = spare;        // <r,r> partials (the update kernel's)
            fx.vec = r;
            return hipk_cg_direction_fx(n_ext, n, ch, G, scal, it, maxiter, r, p, x, &fx, stream);
        }
        HIPK_TRY(xc.parts(part_loc, g_pAp));
        HIPK_TRY(hipk_cg_update(n, ch, G, scal, it, g_pAp, Ap, r, part_loc, HIPK_F64, stream));
        if (overlap) {
            HIPK_CHECK_HIP(hipEventRecord(ev_upd, stream));
            HIPK_CHECK_HIP(hipStreamWaitEvent(side, ev_upd, 0));
            HIPK_TRY(hipk_cg_xupdate(n_ext, ch, G, scal, it, g_pAp, p, x, HIPK_F64, side));
            HIPK_CHECK_HIP(hipEventRecord(ev_x, side));
        }
        HIPK_TRY(xc.grouped(r, part_loc, g_rr));   // the <r,r> partials and the halo of r in ONE group
        if (overlap) HIPK_CHECK_HIP(hipStreamWaitEvent(stream, ev_x, 0));   // p is about to be replaced
        return hipk_cg_direction(n_ext, ch, G, scal, it, maxiter, g_pAp, g_rr, r, p, overlap ? nullptr : x, HIPK_F64, stream);
    }));
    const int64_t iterations = stop < it ? stop : it;

    // ---- TSL:1007-1014: true residual and ||x|| decide info
    HIPK_TRY(xc.run(x));
    HIPK_TRY(hipk_spmv_ex(A, x, Ap, HIPK_SPMV_RESID | HIPK_SPMV_DOT_YY, nullptr, b, spare, part_loc, nullptr, 0, stream));
    HIPK_TRY(xc.parts(part_loc, g_rr));
    HIPK_TRY(hipk_reduce_parts(g_rr, G, out4 + 0, stream));
    HIPK_TRY(hipk_dot_parts(n, ch, x, x, HIPK_F64, part_loc, stream));
    HIPK_TRY(xc.parts(part_loc, g_pAp));
    HIPK_TRY(hipk_reduce_parts(g_pAp, G, out4 + 1, stream));
    HIPK_TRY(hipk_reduce_parts(g_bb, G, out4 + 2, stream));
    double h4[4] = {0, 0, 0, 0};
    HIPK_CHECK_HIP(hipEventRecord(whole.b, stream));
    HIPK_CHECK_HIP(hipMemcpyAsync(h4, out4, sizeof(h4), hipMemcpyDeviceToHost, stream));
    HIPK_CHECK_HIP(hipStreamSynchronize(stream));
    hipk_finish_isolve_stats(st, prm, h4[2], h4[0], h4[1], iterations, iterations + 2);
    float ms = 0.f;
    HIPK_CHECK_HIP(hipEventElapsedTime(&ms, whole.a, whole.b));
    st->solve_ms = ms;
    return HIPK_OK;
}
