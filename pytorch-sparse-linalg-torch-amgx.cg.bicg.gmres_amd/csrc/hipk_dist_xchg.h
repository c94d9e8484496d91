// hipk_dist_xchg.h -- host side of the row-partitioned Jacobi loops (hipk_dist_pcg_solve, hipk_dist_pbicgstab_solve,
// hipk_dist_pgmres_solve): the exchanges of one rank through the hipk_rccl entry points, and the SpMV with a row scaling.
//
// The conventions are those of hipk_dist_cg_solve (csrc/hipk_dist.hip): partials are all-gathered in rank (= global chunk)
// order, the halo of a vector lands in its tail v[n_local .. n_ext) (neighbour send/recv pairs, or an all-gather of padded
// slabs), and a collective that rides with another one goes into the same group.
#pragma once
#include "hipk_common.h"
#include "hipk_spmv.h"

struct hipk_dist_xchg {
    const hipk_dist_plan *pl;
    const hipk_rccl *cc;
    hipStream_t stream;
    double *send_buf, *slab_loc, *slab_all;   // workspace: n_send, slab and world * slab doubles
    const char *who;                          // the entry point, for the error text
    bool need_pack;                           // some peer's send list is scattered (hipk_dist_cg_solve: pack kernel)

    void init() {
        need_pack = false;
        for (int peer = 0; peer < pl->world; ++peer)
            if (pl->send_counts[peer] > 0 && !(pl->send_first && pl->send_first[peer] >= 0)) need_pack = true;
    }
    int fail(const char *what, int r) const {
        hipk_set_error("%s: %s failed (ncclResult %d)", who, what, r);
        return HIPK_ERR_HIP;
    }
    // ONE step of exchanges: the all-gathers of up to two partial arrays (`per` doubles each, src -> dst) and the halo of v
    // (v may be null).  Two or more collective calls go into one group; a lone all-gather is issued as it is.
    int run(double *v, const double *ps0, double *pd0, const double *ps1 = nullptr, double *pd1 = nullptr) const {
        const int NCCL_F64 = 8, W = pl->world;
        const int64_t n = pl->n_local;
        const size_t per = (size_t)pl->per;
        const bool halo = W > 1 && v != nullptr && !(pl->n_send == 0 && pl->n_ghost == 0 && pl->halo_mode == 1);
        const int calls = (ps0 ? 1 : 0) + (ps1 ? 1 : 0) + (halo ? (pl->halo_mode == 1 ? 2 : 1) : 0);
        const bool grouped = W > 1 && calls >= 2;
        int rc;
        if (halo && pl->halo_mode == 1 && pl->n_send && need_pack &&
            (rc = hipk_gather(pl->n_send, pl->send_idx_dev, v, send_buf, HIPK_F64, stream)) != HIPK_OK)
            return rc;
        if (halo && pl->halo_mode == 0 && pl->n_send &&
            (rc = hipk_gather(pl->n_send, pl->send_idx_dev, v, slab_loc, HIPK_F64, stream)) != HIPK_OK)
            return rc;
        if (grouped && (rc = cc->group_start()) != 0) return fail("group_start", rc);
        if (ps0 && (rc = cc->all_gather(ps0, pd0, per, NCCL_F64, cc->comm, stream)) != 0) return fail("all_gather(partials)", rc);
        if (ps1 && (rc = cc->all_gather(ps1, pd1, per, NCCL_F64, cc->comm, stream)) != 0) return fail("all_gather(partials)", rc);
        if (halo && pl->halo_mode == 1) {
            size_t so = 0, ro = 0;
            for (int peer = 0; peer < W; ++peer) {
                const size_t ns = (size_t)pl->send_counts[peer], nr = (size_t)pl->recv_counts[peer];
                const bool direct = pl->send_first && pl->send_first[peer] >= 0;
                if (ns && (rc = cc->send(direct ? v + pl->send_first[peer] : send_buf + so, ns, NCCL_F64, peer, cc->comm, stream)) != 0)
                    return fail("send(halo)", rc);
                if (nr && (rc = cc->recv(v + n + ro, nr, NCCL_F64, peer, cc->comm, stream)) != 0) return fail("recv(halo)", rc);
                so += ns;
                ro += nr;
            }
        }
        if (halo && pl->halo_mode == 0 &&
            (rc = cc->all_gather(slab_loc, slab_all, (size_t)pl->slab, NCCL_F64, cc->comm, stream)) != 0)
            return fail("all_gather(halo slabs)", rc);
        if (grouped && (rc = cc->group_end()) != 0) return fail("group_end", rc);
        if (halo && pl->halo_mode == 0 && pl->n_ghost &&
            (rc = hipk_gather(pl->n_ghost, pl->ghost_src_dev, slab_all, v + n, HIPK_F64, stream)) != HIPK_OK)
            return rc;
        return HIPK_OK;
    }
};

// hipk_spmv_ex with one more operand: dscale != null adds HIPK_SPMV_SCALE (y = dscale .* y after the residual form and before the
// fused dots, so ||y||^2 is that of the scaled vector -- the epilogue of the single-device Jacobi solves).  dscale has the
// handle's n_rows entries (this rank's rows).
static inline int hipk_dist_spmv(const hipk_csr_s *h, const void *x, void *y, int mode, const void *w, const void *bsub,
                                 const void *dscale, double *part0, double *part1, const int64_t *stop_dev, int64_t it,
                                 hipStream_t stream) {
    hipk_spmv_args a;
    memset(&a, 0, sizeof(a));
    a.crow = h->crow;
    a.col = h->col;
    a.val = h->val;
    a.x = x;
    a.y = y;
    a.n = h->n_rows;
    a.ch = h->geom.ch;
    a.g = h->geom.g;
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

// the argument checks of the three row-partitioned Jacobi loops: those of hipk_dist_cg_solve, plus dinv (csrc/hipk_cg.hip)
int hipk_dist_check(hipk_csr_s *A, const hipk_dist_plan *pl, const hipk_rccl *cc, const void *dinv, const void *b_local,
                    void *x_ext, void *work, const hipk_params *prm, hipk_stats *st);
