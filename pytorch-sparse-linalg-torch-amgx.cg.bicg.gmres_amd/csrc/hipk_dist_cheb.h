// hipk_dist_cheb.h -- the Chebyshev polynomial preconditioner on a row block, and the row-partitioned CG that runs it (included
// by hipk_cg.hip after the step API: it uses hipk_cg_scal, hipk_cgm_start and hipk_cgm_direction).
//
// z = p_m(D^-1 A) D^-1 r of the GLOBAL system, every rank holding its rows: the recurrence and the rounding spec of
// hipk_cheb_apply (include/hipk.h) on the rectangular block handle -- n_local rows, columns in [0, n_ext).  Step k gathers
// z_{k-1} over own and ghost columns and writes z_k for the rank's own rows; the ghost tail of z_k comes from its owners in a halo
// exchange before step k + 1.  No dot product anywhere: an apply costs halo exchanges only.  Where the block handle's SpMV has the
// Chebyshev epilogue a step is ONE launch and z ping-pongs between two n_ext-long buffers (a row must not gather a z another
// workgroup has already replaced), the parity chosen so that z_m lands in the caller's buffer; elsewhere, and with
// HIPK_CHEB_FUSED=0, it is the SpMV's residual form with the row scaling into the other buffer followed by hipk_cheb_step_kernel
// on the rank's rows, z staying in place.  The same operations in the same order per row as on one device: the same bits.
//
// hipk_dist_chebcg_solve is the iteration `_hipk.solve_cg_stepwise` runs on one device with such an M (gamma = <r,z> steers
// alpha and beta, the stop test uses <r,r>, TSL:835-841), with the conventions of hipk_dist_pcg_solve.  Per iteration:
//   SpMV p -> Ap, <p,Ap> | all-gather <p,Ap> | update + Chebyshev step 0 on own rows (ONE kernel) | ONE group: all-gather <r,r> +
//   the halo of r | step 0 on the ghost rows (the owner's operands: the exchanged r and the dinv tail) | steps 1 .. m, a
//   stand-alone halo of z_k before step k + 1 | <r,z> partials | ONE group: all-gather <r,z> + the halo of z_m | direction over
//   n_ext (x += alpha p, p = z + beta p on own and ghost rows)
// = m + 2 collective launches, the minimum: m + 1 products need m + 1 halos (that of p is never exchanged: every rank forms its
// ghost entries from the halo of z_m), CG has two reduction points, and a halo rides with an all-gather wherever one is due.
#pragma once
#include "hipk_dist_xchg.h"

// r -= alpha Ap with the <r,r> chunk partials (hipk_cg_update_kernel) AND Chebyshev step 0, d = c0 * (dinv * r), z_0 = d
// (hipk_cheb_init_kernel), in one pass over the rank's rows: r never comes back from memory for step 0 -- reads Ap, r, dinv,
// writes r, d, z_0: 48 n bytes against 24 n + 32 n of the two kernels, and one launch less.  Every operation its own rounding:
// the bits of the two kernels.  Gated on the stop word like every vector kernel of the loop: past the stop the steps behind it
// work on the d and z of the last iteration -- nothing reads their output, and the final apply starts from step 0 again.
template <typename T>
__global__ __launch_bounds__(HIPK_THREADS) void hipk_cheb_update_kernel(
    int64_t n, int ch, int g, const hipk_cg_scal *__restrict__ scal, int64_t it, const double *__restrict__ part_pAp,
    const T *__restrict__ Ap, const T *__restrict__ dinv, T c0, T *__restrict__ r, T *__restrict__ d, T *__restrict__ z0,
    double *__restrict__ part_rr) {
    constexpr int VEC = hipk_vec<T>::VEC;
    const int c = blockIdx.x;
    hipk_pre<T, 2> pre;
    pre.issue(n, ch, c, {Ap, (const T *)r});
    if (it >= scal->stop_it) return;
    __shared__ double sbuf[HIPK_THREADS];
    const double pAp = hipk_reduce_parts(part_pAp, g, sbuf);
    const double gamma = scal->gamma[it & 1];
    const T alpha = (T)(gamma / pAp);  // TSL:846
    double acc = 0.0;
    pre.run([&](int64_t i, int nv, T(&v)[2][VEC]) {
        T rv[VEC], dv[VEC], o[VEC];
        hipk_ld<T>(dinv, i, nv, dv);
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const T m1 = alpha * v[0][k];
            rv[k] = v[1][k] - m1;  // TSL:848
            if (k < nv) acc = fma((double)rv[k], (double)rv[k], acc);  // TSL:850
            o[k] = c0 * (dv[k] * rv[k]);  // step 0
        }
        hipk_st<T>(r, i, nv, rv);
        hipk_st<T>(d, i, nv, o);
        hipk_st<T>(z0, i, nv, o);
    });
    acc = hipk_block_sum(acc, sbuf);
    if (threadIdx.x == 0) part_rr[c] = acc;
}

// step 0 on the ghost rows, z_0 = c0 * (dinv * r) from the exchanged r and the caller's dinv tail: the owner's operands, the
// owner's bits (d lives on own rows only).  The tails start at n_local, any alignment: one element per lane.
template <typename T>
__global__ __launch_bounds__(HIPK_THREADS) void hipk_cheb_ghost0_kernel(int64_t n_ghost, T c0, const T *__restrict__ dinv_g,
                                                                        const T *__restrict__ r_g, T *__restrict__ z_g) {
    const int64_t i = (int64_t)blockIdx.x * HIPK_THREADS + threadIdx.x;
    if (i < n_ghost) z_g[i] = c0 * (dinv_g[i] * r_g[i]);
}

// one apply on a row block: the operands, the two z buffers and which form a step takes
struct hipk_dcheb {
    const hipk_csr_s *A;
    const hipk_dist_plan *pl;
    const hipk_dist_xchg *xc;
    hipStream_t stream;
    int m;
    const double *dinv;   // n_ext: own rows, then the owners' entries at the halo positions
    const double *coef;   // host: c0, c1[1..m], c2[1..m], scale
    double *d;            // n_local
    double *z_out;        // n_ext: z_m lands in its first n_local entries
    double *z_alt;        // n_ext: the other z buffer (one launch per step) or res (two)
    bool fused;

    // does the kernel the block handle's SpMV resolves to have the epilogue?  (y = null: nothing is launched)
    int begin() {
        fused = hipk_sw_enabled("HIPK_CHEB_FUSED");
        if (fused) {
            hipk_spmv_args a = args(nullptr);
            a.mode = HIPK_SPMV_CHEB_MODE;
            const int rc = hipk_launch_spmv(A, a, stream);
            if (rc != HIPK_OK && rc != HIPK_SPMV_NO_CHEB) return rc;
            fused = rc == HIPK_OK;
        }
        return HIPK_OK;
    }
    // where z_0 goes: z_k lives in z_out when m - k is even (one launch per step), always (two)
    double *z_start() const { return (fused && (m & 1)) ? z_alt : z_out; }
    hipk_spmv_args args(const double *r) const {
        hipk_spmv_args a = hipk_spmv_base(A);
        a.bsub = r;
        a.dscale = dinv;
        a.cheb_d = d;
        return a;
    }
    // step 0 on the ghost rows of z_start(), after the halo of r
    int ghost0(const double *r) const {
        const int64_t n = pl->n_local, ng = pl->n_ghost;
        if (ng <= 0) return HIPK_OK;
        hipk_cheb_ghost0_kernel<double><<<(int)((ng + HIPK_THREADS - 1) / HIPK_THREADS), HIPK_THREADS, 0, stream>>>(
            ng, coef[0], dinv + n, r + n, z_start() + n);
        HIPK_CHECK_HIP(hipGetLastError());
        return HIPK_OK;
    }
    // steps 1 .. m on z_0 = z_start() (own AND ghost rows filled); a stand-alone halo of z_k before step k + 1.  z_m: the first
    // n_local entries of z_out.
    int steps(const double *r) const {
        const int64_t n = pl->n_local;
        const double *c1 = coef, *c2 = coef + m, scale = coef[2 * m + 1];   // c1[k], c2[k], k = 1 .. m
        hipk_spmv_args a = args(r);
        double *zk = z_start();
        for (int k = 1; k <= m; ++k) {
            const double sk = (k == m) ? scale : 1.0;
            if (k > 1) HIPK_TRY(xc->run(zk));
            if (fused) {
                double *zn = (zk == z_out) ? z_alt : z_out;
                a.mode = HIPK_SPMV_CHEB_MODE;
                a.x = zk;
                a.y = zn;
                a.cheb_c1 = c1[k];
                a.cheb_c2 = c2[k];
                a.cheb_scale = sk;
                HIPK_TRY(hipk_launch_spmv(A, a, stream));
                zk = zn;
            } else {
                a.mode = HIPK_SPMV_RESID | HIPK_SPMV_SCALE;
                a.x = z_out;
                a.y = z_alt;
                HIPK_TRY(hipk_launch_spmv(A, a, stream));
                HIPK_TRY(hipk_launch_cheb_step(n, pl->chunk_rows, c1[k], c2[k], sk, z_alt, d, z_out, stream));
            }
        }
        if (!fused) hipk_note_cheb_step();
        return HIPK_OK;
    }
    // the whole apply on r (n_ext; its ghost tail is filled here, by a stand-alone halo exchange)
    int apply(double *r) const {
        HIPK_TRY(xc->run(r));
        HIPK_TRY(hipk_launch_cheb_init(pl->n_local, pl->chunk_rows, coef[0], dinv, r, d, z_start(), stream));
        HIPK_TRY(ghost0(r));
        return steps(r);
    }
};

static int hipk_dcheb_check(const hipk_csr_s *A, const hipk_dist_plan *pl, int degree, const double *coef_host) {
    HIPK_REQUIRE(coef_host, HIPK_ERR_ARG, "null argument");
    HIPK_REQUIRE(degree >= 1 && degree <= 32, HIPK_ERR_ARG, "degree must be in [1, 32]");
    HIPK_REQUIRE(A->op_cb == nullptr, HIPK_ERR_UNSUPPORTED, "the row block must be a CSR handle, not a matrix-free operator");
    HIPK_REQUIRE(A->n_cols >= pl->n_ext && A->geom.ch == pl->chunk_rows, HIPK_ERR_ARG,
                 "the block handle must have n_ext columns and the plan's chunk size");
    return HIPK_OK;
}

// ---- the apply on its own: header (pack buffers) | d | the second z buffer
struct hipk_dcheb_layout {
    size_t send_buf, slab_loc, slab_all, d, z_alt, total;
};
static hipk_dcheb_layout hipk_dcheb_make_layout(const hipk_dist_plan *pl) {
    hipk_dcheb_layout L;
    hipk_carve take;
    const size_t W = (size_t)pl->world;
    const size_t next = (size_t)(pl->n_ext > 0 ? pl->n_ext : 1), nloc = (size_t)(pl->n_local > 0 ? pl->n_local : 1);
    L.send_buf = take((size_t)(pl->n_send > 0 ? pl->n_send : 1) * 8);
    L.slab_loc = take((size_t)(pl->slab > 0 ? pl->slab : 1) * 8);
    L.slab_all = take((size_t)(pl->slab > 0 ? pl->slab : 1) * W * 8);
    L.d = take(nloc * 8);
    L.z_alt = take(next * 8);
    L.total = take.o;
    return L;
}

extern "C" size_t hipk_dist_cheb_work_bytes(const hipk_dist_plan *plan) {
    if (!plan || plan->world < 1 || plan->per < 1) return 0;
    return hipk_dcheb_make_layout(plan).total;
}

extern "C" int hipk_dist_cheb_apply(hipk_csr_t A, const hipk_dist_plan *pl, const hipk_rccl *cc, int degree, const void *dinv_ext,
                                    const double *coef_host, void *r_ext, void *z_ext, void *work, size_t work_bytes,
                                    hipk_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    static const hipk_params no_params = {};   // hipk_dist_check looks at the pointers only
    static const hipk_stats no_stats = {};
    HIPK_TRY(hipk_dist_check(A, pl, cc, true, dinv_ext, r_ext, z_ext, work, &no_params, &no_stats));
    HIPK_TRY(hipk_dcheb_check(A, pl, degree, coef_host));
    HIPK_REQUIRE(r_ext != z_ext && dinv_ext != z_ext, HIPK_ERR_ARG, "r, z and dinv must be distinct");
    const hipk_dcheb_layout L = hipk_dcheb_make_layout(pl);
    HIPK_REQUIRE(work_bytes >= L.total, HIPK_ERR_WORKSPACE, "work too small");
    char *wk = (char *)work;
    const hipk_dist_xchg xc(pl, cc, stream, (double *)(wk + L.send_buf), (double *)(wk + L.slab_loc), (double *)(wk + L.slab_all),
                            "hipk_dist_cheb_apply");
    hipk_dcheb ap = {A, pl, &xc, stream, degree, (const double *)dinv_ext, coef_host, (double *)(wk + L.d), (double *)z_ext,
                     (double *)(wk + L.z_alt), false};
    HIPK_TRY(ap.begin());
    HIPK_TRY(ap.apply((double *)r_ext));
    HIPK_CHECK_HIP(hipGetLastError());
    return HIPK_OK;
}

// ---- the loop
struct hipk_dchebcg_layout {
    size_t scal, part_loc, part_rz, spare, g_pAp, g_rr, g_bb, g_rz, g_xx, out4, send_buf, slab_loc, slab_all, p, r, Ap, d, z0, z1, total;
};
static hipk_dchebcg_layout hipk_dchebcg_make_layout(const hipk_dist_plan *pl) {
    hipk_dchebcg_layout L;
    hipk_carve take;
    const size_t per = (size_t)pl->per, W = (size_t)pl->world;
    const size_t next = (size_t)(pl->n_ext > 0 ? pl->n_ext : 1), nloc = (size_t)(pl->n_local > 0 ? pl->n_local : 1);
    L.scal = take(256);
    L.part_loc = take(per * 8);
    L.part_rz = take(per * 8);
    L.spare = take(per * 8);
    L.g_pAp = take(W * per * 8);
    L.g_rr = take(W * per * 8);
    L.g_bb = take(W * per * 8);
    L.g_rz = take(W * per * 8);
    L.g_xx = take(W * per * 8);
    L.out4 = take(4 * 8);
    L.send_buf = take((size_t)(pl->n_send > 0 ? pl->n_send : 1) * 8);
    L.slab_loc = take((size_t)(pl->slab > 0 ? pl->slab : 1) * 8);
    L.slab_all = take((size_t)(pl->slab > 0 ? pl->slab : 1) * W * 8);
    L.p = take(next * 8);
    L.r = take(next * 8);
    L.Ap = take(nloc * 8);
    L.d = take(nloc * 8);
    L.z0 = take(next * 8);
    L.z1 = take(next * 8);
    L.total = take.o;
    return L;
}

extern "C" size_t hipk_dist_chebcg_work_bytes(const hipk_dist_plan *plan) {
    if (!plan || plan->world < 1 || plan->per < 1) return 0;
    return hipk_dchebcg_make_layout(plan).total;
}

extern "C" int hipk_dist_chebcg_solve(hipk_csr_t A, const hipk_dist_plan *pl, const hipk_rccl *cc, int degree, const void *dinv_ext,
                                      const double *coef_host, const void *b_local, void *x_ext, void *work, size_t work_bytes,
                                      const hipk_params *prm, hipk_stats *st, hipk_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    HIPK_TRY(hipk_dist_check(A, pl, cc, true, dinv_ext, b_local, x_ext, work, prm, st));
    HIPK_TRY(hipk_dcheb_check(A, pl, degree, coef_host));
    const hipk_dchebcg_layout L = hipk_dchebcg_make_layout(pl);
    HIPK_REQUIRE(work_bytes >= L.total, HIPK_ERR_WORKSPACE, "work too small");
    memset(st, 0, sizeof(*st));
    char *wk = (char *)work;
    hipk_cg_scal *scal = (hipk_cg_scal *)(wk + L.scal);
    double *part_loc = (double *)(wk + L.part_loc), *part_rz = (double *)(wk + L.part_rz), *spare = (double *)(wk + L.spare);
    double *g_pAp = (double *)(wk + L.g_pAp), *g_rr = (double *)(wk + L.g_rr), *g_bb = (double *)(wk + L.g_bb);
    double *g_rz = (double *)(wk + L.g_rz), *g_xx = (double *)(wk + L.g_xx), *out4 = (double *)(wk + L.out4);
    double *p = (double *)(wk + L.p), *r = (double *)(wk + L.r), *Ap = (double *)(wk + L.Ap);
    double *x = (double *)x_ext;
    const double *b = (const double *)b_local, *dinv = (const double *)dinv_ext;
    const int64_t n = pl->n_local, n_ext = pl->n_ext;
    const int ch = pl->chunk_rows, G = pl->g_red;
    const int grid = (int)((n + ch - 1) / ch);
    const int64_t maxiter = hipk_default_maxiter(prm, pl->n_global);
    const int64_t *stop_dev = &scal->stop_it;
    const hipk_dist_xchg xc(pl, cc, stream, (double *)(wk + L.send_buf), (double *)(wk + L.slab_loc), (double *)(wk + L.slab_all),
                            "hipk_dist_chebcg_solve");
    hipk_dcheb M = {A, pl, &xc, stream, degree, dinv, coef_host, (double *)(wk + L.d), (double *)(wk + L.z0), (double *)(wk + L.z1),
                    false};
    double *z = M.z_out;
    hipk_set_solve_path(nullptr, "hipk_dist_chebcg launch sequence");

    hipk_event_pair whole;
    HIPK_CHECK_HIP(whole.create());
    HIPK_CHECK_HIP(hipEventRecord(whole.a, stream));
    HIPK_CHECK_HIP(hipMemsetAsync(wk, 0, L.total, stream));
    if (n_ext > n) HIPK_CHECK_HIP(hipMemsetAsync(x + n, 0, (size_t)(n_ext - n) * 8, stream));
    HIPK_TRY(M.begin());

    // ---- r0 = b - A x0, <r0,r0>; <b,b>; z0 = M r0, gamma0 = <r0,z0>; p0 = z0 on own and ghost rows (TSL:815-826)
    HIPK_TRY(xc.run(x));
    HIPK_TRY(hipk_dist_spmv(A, x, r, HIPK_SPMV_RESID | HIPK_SPMV_DOT_YY, nullptr, b, nullptr, spare, part_loc, nullptr, 0, stream));
    HIPK_TRY(xc.parts(part_loc, g_rr));
    HIPK_TRY(hipk_dot_parts(n, ch, b, b, HIPK_F64, part_loc, stream));
    HIPK_TRY(xc.parts(part_loc, g_bb));
    HIPK_TRY(M.apply(r));
    HIPK_TRY(hipk_dot_parts(n, ch, r, z, HIPK_F64, part_rz, stream));
    HIPK_TRY(xc.run(z, part_rz, g_rz));
    HIPK_TRY(hipk_cgm_start(n_ext, ch, G, scal, g_rz, g_rr, g_bb, z, p, HIPK_F64, prm->tol, prm->atol, maxiter, stream));

    // ---- the loop: fixed batches, the stop word read one batch late (hipk_dist_batches)
    int64_t it = 0, stop = INT64_MAX;
    HIPK_TRY(hipk_dist_batches(prm, A->host_poll, stop_dev, maxiter, stream, it, stop, [&](int64_t it) -> int {
        HIPK_TRY(hipk_dist_spmv(A, p, Ap, HIPK_SPMV_DOT_W, p, nullptr, nullptr, part_loc, spare, stop_dev, it, stream));
        HIPK_TRY(xc.parts(part_loc, g_pAp));
        hipk_cheb_update_kernel<double><<<grid, HIPK_THREADS, 0, stream>>>(n, ch, G, scal, it, g_pAp, Ap, dinv, coef_host[0], r, M.d,
                                                                            M.z_start(), part_loc);
        HIPK_TRY(xc.grouped(r, part_loc, g_rr));       // the <r,r> partials and the halo of r in ONE group
        HIPK_TRY(M.ghost0(r));
        HIPK_TRY(M.steps(r));
        HIPK_TRY(hipk_dot_parts(n, ch, r, z, HIPK_F64, part_rz, stream));
        HIPK_TRY(xc.grouped(z, part_rz, g_rz));        // the <r,z> partials and the halo of z_m in ONE group
        return hipk_cgm_direction(n_ext, ch, G, scal, it, maxiter, g_pAp, g_rz, g_rr, z, p, x, HIPK_F64, stream);
    }));
    const int64_t iterations = stop < it ? stop : it;

    // ---- TSL:1007-1014 with M: ||M (b - A x)||, ||x||  (the residual takes r's place: its ghost tail is needed once more)
    HIPK_TRY(xc.run(x));
    HIPK_TRY(hipk_dist_spmv(A, x, r, HIPK_SPMV_RESID, nullptr, b, nullptr, spare, spare, nullptr, 0, stream));
    HIPK_TRY(M.apply(r));
    HIPK_TRY(hipk_dot_parts(n, ch, z, z, HIPK_F64, part_loc, stream));
    HIPK_TRY(xc.parts(part_loc, g_rr));
    HIPK_TRY(hipk_reduce_parts(g_rr, G, out4 + 0, stream));
    HIPK_TRY(hipk_dot_parts(n, ch, x, x, HIPK_F64, part_loc, stream));
    HIPK_TRY(xc.parts(part_loc, g_xx));
    HIPK_TRY(hipk_reduce_parts(g_xx, G, out4 + 1, stream));
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
