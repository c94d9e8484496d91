// hipk_dist_xchg.h -- host side shared by the six row-partitioned loops (hipk_dist_{,p}cg_solve, hipk_dist_{,p}bicgstab_solve,
// hipk_dist_{,p}gmres_solve): every collective call of one rank through the hipk_rccl entry points, the argument checks, the
// batch driver and the SpMV with a row scaling.
//
// The conventions are those of hipk_dist_cg_solve (csrc/hipk_dist.hip): partials are all-gathered in rank (= global chunk)
// order, the halo of a vector lands in its tail v[n_local .. n_ext) (neighbour send/recv pairs, or an all-gather of padded
// slabs), and a collective that rides with another one goes into the same group.  A failed collective sets
// "<entry point>: <call> failed (ncclResult <r>)" and returns HIPK_ERR_HIP.
#pragma once
#include "hipk_common.h"
#include "hipk_solve.h"
#include "hipk_spmv.h"

struct hipk_dist_xchg {
    const hipk_dist_plan *pl;
    const hipk_rccl *cc;
    hipStream_t stream;
    double *send_buf, *slab_loc, *slab_all;   // workspace: n_send, slab and world * slab doubles
    const char *who;                          // the entry point, for the error text
    bool need_pack = false;                   // some peer's send list is scattered: the pack kernel runs before the sends

    hipk_dist_xchg(const hipk_dist_plan *pl_, const hipk_rccl *cc_, hipStream_t s, double *send_buf_, double *slab_loc_,
                   double *slab_all_, const char *who_)
        : pl(pl_), cc(cc_), stream(s), send_buf(send_buf_), slab_loc(slab_loc_), slab_all(slab_all_), who(who_) {
        // contiguous send ranges go out straight from the vector
        for (int peer = 0; peer < pl->world; ++peer)
            if (pl->send_counts[peer] > 0 && !(pl->send_first && pl->send_first[peer] >= 0)) need_pack = true;
    }
    int nccl(int r, const char *what) const {
        if (r == 0) return HIPK_OK;
        hipk_set_error("%s: %s failed (ncclResult %d)", who, what, r);
        return HIPK_ERR_HIP;
    }
    int group_start() const { return nccl(cc->group_start(), "group_start"); }
    int group_end() const { return nccl(cc->group_end(), "group_end"); }
    // all-gather of `per` partials, src -> dst in rank order
    int parts(const double *src, double *dst) const {
        return nccl(cc->all_gather(src, dst, (size_t)pl->per, NCCL_F64, cc->comm, stream), "all_gather(partials)");
    }
    // in place: this rank's partials are already at arr + rank * per
    int parts(double *arr) const { return parts(arr + (size_t)pl->rank * pl->per, arr); }
    // in place, one call of `count` doubles per rank: this rank's block is at arr + rank * count (the wide GMRES multi-dot)
    int block(double *arr, size_t count) const {
        return nccl(cc->all_gather(arr + (size_t)pl->rank * count, arr, count, NCCL_F64, cc->comm, stream), "all_gather(partials)");
    }
    // ONE step of exchanges: the all-gathers of up to two partial arrays (src -> dst) and the halo of v (v may be null).  run():
    // two or more collective calls go into one group; grouped(): a group at world > 1 whatever the calls.  v = x alone is the
    // stand-alone halo exchange (a group around the send/recv pairs; the slab all-gather on its own).
    int run(double *v, const double *ps0 = nullptr, double *pd0 = nullptr, const double *ps1 = nullptr, double *pd1 = nullptr) const {
        return step(false, v, ps0, pd0, ps1, pd1);
    }
    int grouped(double *v, const double *ps0, double *pd0, const double *ps1 = nullptr, double *pd1 = nullptr) const {
        return step(true, v, ps0, pd0, ps1, pd1);
    }

  private:
    static constexpr int NCCL_F64 = 8;
    int step(bool always, double *v, const double *ps0, double *pd0, const double *ps1, double *pd1) const {
        const int W = pl->world;
        const int64_t n = pl->n_local;
        const bool halo = W > 1 && v != nullptr && !(pl->n_send == 0 && pl->n_ghost == 0 && pl->halo_mode == 1);
        const bool p2p = halo && pl->halo_mode == 1, slabs = halo && pl->halo_mode == 0;
        const int calls = (ps0 ? 1 : 0) + (ps1 ? 1 : 0) + (p2p ? 2 : slabs ? 1 : 0);
        const bool group = W > 1 && (always || calls >= 2);
        if (p2p && pl->n_send && need_pack) HIPK_TRY(hipk_gather(pl->n_send, pl->send_idx_dev, v, send_buf, HIPK_F64, stream));
        if (slabs && pl->n_send) HIPK_TRY(hipk_gather(pl->n_send, pl->send_idx_dev, v, slab_loc, HIPK_F64, stream));
        if (group) HIPK_TRY(group_start());
        if (ps0) HIPK_TRY(parts(ps0, pd0));
        if (ps1) HIPK_TRY(parts(ps1, pd1));
        if (p2p) {
            size_t so = 0, ro = 0;
            for (int peer = 0; peer < W; ++peer) {
                const size_t ns = (size_t)pl->send_counts[peer], nr = (size_t)pl->recv_counts[peer];
                const bool direct = pl->send_first && pl->send_first[peer] >= 0;
                if (ns) HIPK_TRY(nccl(cc->send(direct ? v + pl->send_first[peer] : send_buf + so, ns, NCCL_F64, peer, cc->comm, stream), "send(halo)"));
                if (nr) HIPK_TRY(nccl(cc->recv(v + n + ro, nr, NCCL_F64, peer, cc->comm, stream), "recv(halo)"));
                so += ns;
                ro += nr;
            }
        }
        if (slabs) HIPK_TRY(nccl(cc->all_gather(slab_loc, slab_all, (size_t)pl->slab, NCCL_F64, cc->comm, stream), "all_gather(halo slabs)"));
        if (group) HIPK_TRY(group_end());
        if (slabs && pl->n_ghost) HIPK_TRY(hipk_gather(pl->n_ghost, pl->ghost_src_dev, slab_all, v + n, HIPK_F64, stream));
        return HIPK_OK;
    }
};

// The loop of the row-partitioned CG and BiCGStab: fixed batches of body(it), the stop word read one batch late (two reads in
// flight).  Every rank posts and harvests at the same points and derives the same stop word from the same gathered partials, so
// all ranks leave at the same batch boundary having issued the same collectives (iterations past the stop are no-ops on the
// device; their collectives still pair up).  it = the iterations issued, stop = the harvested stop word; both are the caller's,
// so that its guards see how far the loop got on every exit.
template <class Body>
static int hipk_dist_batches(const hipk_params *prm, int64_t *host_poll, const int64_t *stop_dev, int64_t maxiter,
                             hipStream_t stream, int64_t &it, int64_t &stop, Body &&body) {
    const int64_t batch = prm->check_every > 0 ? prm->check_every : 16;
    hipk_poller poll(host_poll);
    HIPK_CHECK_HIP(poll.create());
    it = 0;
    stop = INT64_MAX;
    while (it < maxiter) {
        const int64_t end = (it + batch < maxiter) ? it + batch : maxiter;
        for (; it < end; ++it) HIPK_TRY(body(it));
        HIPK_CHECK_HIP(hipGetLastError());
        HIPK_CHECK_HIP(poll.post(stop_dev, it, stream));
        if (poll.count == 2) {
            HIPK_CHECK_HIP(hipEventSynchronize(poll.ev[poll.head]));
            poll.harvest(&stop);
        }
        if (stop <= it - batch) break;   // the batch BEFORE the one just enqueued had already reached the stop
    }
    HIPK_CHECK_HIP(poll.drain(&stop));
    return HIPK_OK;
}

// hipk_spmv_ex with one more operand: dscale != null adds HIPK_SPMV_SCALE (y = dscale .* y after the residual form and before the
// fused dots, so ||y||^2 is that of the scaled vector -- the epilogue of the single-device Jacobi solves).  dscale has the
// handle's n_rows entries (this rank's rows).  With dscale = null it launches what hipk_spmv_ex does, without its checks.
static inline int hipk_dist_spmv(const hipk_csr_s *h, const void *x, void *y, int mode, const void *w, const void *bsub,
                                 const void *dscale, double *part0, double *part1, const int64_t *stop_dev, int64_t it,
                                 hipStream_t stream) {
    hipk_spmv_args a = hipk_spmv_base(h);
    a.x = x;
    a.y = y;
    a.mode = mode | (dscale ? HIPK_SPMV_SCALE : 0);
    a.w = w;
    a.bsub = bsub;
    a.dscale = dscale;
    a.part0 = part0;
    a.part1 = part1;
    a.stop_it = stop_dev;
    a.it = it;
    return hipk_launch_spmv(h, a, stream);
}

// the argument checks of the six row-partitioned loops (csrc/hipk_dist.hip); pre: a Jacobi loop, dinv must be given and 16-byte
// aligned.  `geometry` overrides the text of the partial-sum geometry check.
int hipk_dist_check(const hipk_csr_s *A, const hipk_dist_plan *pl, const hipk_rccl *cc, bool pre, const void *dinv,
                    const void *b_local, const void *x_ext, const void *work, const hipk_params *prm, const hipk_stats *st,
                    const char *geometry = nullptr);
