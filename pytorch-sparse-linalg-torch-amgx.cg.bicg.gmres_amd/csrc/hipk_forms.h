// The forms a solve of libhipk can finish in (hipk_last_solve_form): the ONE table of their names.  hipk_last_solve_path says which
// KIND of loop finished a solve ("launch sequence", "hipk_cg_solve_lds_kernel", a mid kernel); the form says which of that kind's
// variants, at the resolution of the dispatch structs (hipk_cg_path, hipk_bi_path, hipk_gm_path).  A dispatch site names its form
// with HIPK_FORM("..."): a string that is not a row does not compile.  DESIGN.md 8b lists the same rows; tests/_form_cases.py
// pins each of them to the oracle (tests/test_form_cases.py keeps table and cases in step).
#pragma once
#include "hipk_switch.h"

struct hipk_form_row {
    const char *name, *meaning;
};

// the instantiations of the one-launch loops, fp64 and fp32
#define HIPK_FORM_T2(head, tail, meaning) {head "double," tail, meaning}, {head "float," tail, meaning}
#define HIPK_FORM_CG_LDS(LOCAL, PRE, meaning) HIPK_FORM_T2("hipk_cg_solve_lds_kernel<", #LOCAL "," #PRE ">", meaning)
#define HIPK_FORM_BI_LDS(LOCAL, PRE, meaning) HIPK_FORM_T2("hipk_bi_solve_lds_kernel<", #LOCAL "," #PRE ">", meaning)
#define HIPK_FORM_GM_LDS(LOCAL, meaning) HIPK_FORM_T2("hipk_gm_solve_lds_kernel<", #LOCAL ">", meaning)
#define HIPK_FORM_CG_MID(W, NCH, PRE) HIPK_FORM_T2("hipk_cg_mid_kernel<", #W "," #NCH "," #PRE ">", "CG / Jacobi PCG mid loop (hipk_cg_mid.h)")
#define HIPK_FORM_BI_MID(W, PRE) HIPK_FORM_T2("hipk_bi_mid_kernel<", #W "," #PRE ">", "BiCGStab mid loop (hipk_bi_mid.h)")
#define HIPK_FORM_GM_MID(W, PRE) HIPK_FORM_T2("hipk_gm_mid_kernel<", #W "," #PRE ">", "GMRES mid cycle (hipk_gm_mid.h)")
// a launch sequence of GMRES or BiCGStab, and the same with the caller's M through a callback
#define HIPK_FORM_CB(name, meaning) {name, meaning}, {name ", callback M", meaning}

// one row per form
static constexpr hipk_form_row hipk_solve_forms[] = {
    // ---- CG and Jacobi PCG (hipk_cg.hip): <T, LOCAL, PRE>
    HIPK_FORM_CG_LDS(true, false, "CG, whole loop in one launch on ONE XCD, hand-offs through its L2"),
    HIPK_FORM_CG_LDS(false, false, "CG, whole loop in one launch, agent-scope hand-offs (spread over the chip, HIPK_CG_LOOP_AGENT, or after a -2)"),
    HIPK_FORM_CG_LDS(true, true, "Jacobi PCG, whole loop in one launch on ONE XCD"),
    HIPK_FORM_CG_LDS(false, true, "Jacobi PCG, whole loop in one launch, agent-scope hand-offs"),
    HIPK_FORM_CG_MID(5, 1, false), HIPK_FORM_CG_MID(7, 1, false), HIPK_FORM_CG_MID(9, 1, false), HIPK_FORM_CG_MID(12, 1, false),
    HIPK_FORM_CG_MID(5, 2, false), HIPK_FORM_CG_MID(7, 2, false),
    HIPK_FORM_CG_MID(5, 1, true), HIPK_FORM_CG_MID(7, 1, true), HIPK_FORM_CG_MID(9, 1, true), HIPK_FORM_CG_MID(12, 1, true),
    {"cg two-launch: hipk_cg2_spmv_kernel<double,1280> + hipk_cg2_update_kernel", "33 .. 150 chunks, fp64: tiles of up to 1280 entries"},
    {"cg two-launch: hipk_cg2_spmv_kernel<float,2048> + hipk_cg2_update_kernel", "33 .. 150 chunks, fp32: tiles of up to 2048 entries"},
    {"cg three-launch, small", "<= 8 chunks: SpMV without its combine launch, update and direction fold the tile sums"},
    {"cg three-launch", "SpMV, update, direction with the default cache policy"},
    {"cg three-launch, streams", "x, r, p, Ap beyond 384 MiB: the vector kernels treat every operand as a stream"},
    {"cg three-launch, streams + flat direction", "... and the direction step as a scalars launch + a flat grid (a vector beyond 256 MiB)"},
    {"pcg three-launch, Jacobi", "Jacobi PCG: SpMV, hipk_pcg_update_kernel, hipk_pcg_direction_kernel"},
    // ---- BiCGStab (hipk_bicgstab.hip): <T, LOCAL, PRE>
    HIPK_FORM_BI_LDS(true, false, "BiCGStab, whole loop in one launch on ONE XCD"),
    HIPK_FORM_BI_LDS(false, false, "BiCGStab, whole loop in one launch, agent-scope hand-offs"),
    HIPK_FORM_BI_LDS(true, true, "Jacobi BiCGStab, whole loop in one launch on ONE XCD"),
    HIPK_FORM_BI_LDS(false, true, "Jacobi BiCGStab, whole loop in one launch, agent-scope hand-offs"),
    HIPK_FORM_BI_MID(5, false), HIPK_FORM_BI_MID(7, false), HIPK_FORM_BI_MID(9, false), HIPK_FORM_BI_MID(12, false),
    HIPK_FORM_BI_MID(5, true), HIPK_FORM_BI_MID(7, true), HIPK_FORM_BI_MID(9, true), HIPK_FORM_BI_MID(12, true),
    HIPK_FORM_CB("bicgstab five-launch, small", "<= 8 chunks: both SpMVs without their combine launch"),
    HIPK_FORM_CB("bicgstab five-launch", "direction, SpMV, s update, SpMV, x update"),
    {"bicgstab five-launch, small, Jacobi", "<= 8 chunks, M = diag(dinv) applied in the kernels"},
    {"bicgstab five-launch, Jacobi", "M = diag(dinv) applied in the kernels"},
    // ---- GMRES (hipk_gmres.hip): <T, LOCAL>; Jacobi is a run-time argument of every GMRES kernel
    HIPK_FORM_GM_LDS(true, "GMRES, whole solve in one launch on ONE XCD"),
    HIPK_FORM_GM_LDS(false, "GMRES, whole solve in one launch, agent-scope hand-offs (spread over the chip, HIPK_GM_CYCLE_AGENT, or after a -2)"),
    {"hipk_gm_cycle_small_kernel<double>", "<= 8 chunks: one launch per restart cycle, one workgroup per tile"},
    {"hipk_gm_cycle_small_kernel<float>", "<= 8 chunks: one launch per restart cycle, one workgroup per tile"},
    HIPK_FORM_GM_MID(5, false), HIPK_FORM_GM_MID(7, false), HIPK_FORM_GM_MID(9, false), HIPK_FORM_GM_MID(12, false),
    HIPK_FORM_GM_MID(5, true), HIPK_FORM_GM_MID(7, true), HIPK_FORM_GM_MID(9, true), HIPK_FORM_GM_MID(12, true),
    HIPK_FORM_CB("gmres small + wide", "<= 8 chunks, restart <= 31: hipk_gm_multidot_wide_kernel / hipk_gm_update_wide_kernel"),
    HIPK_FORM_CB("gmres small + 256-thread", "<= 8 chunks, restart <= 31: hipk_gm_multidot_kernel<T,true> / hipk_gm_update_kernel<T,true>"),
    HIPK_FORM_CB("gmres large, first kernels", "restart <= 31, HIPK_GMRES_NO_STREAM: hipk_gm_multidot_kernel<T,false> / hipk_gm_update_kernel<T,false>"),
    HIPK_FORM_CB("gmres large, first kernels + split norm", "... normalise step as hipk_gm_hcol_kernel + hipk_gm_scale_kernel"),
    HIPK_FORM_CB("gmres large, streaming", "restart <= 31: hipk_gm_multidot_stream_kernel / hipk_gm_update_stream_kernel"),
    HIPK_FORM_CB("gmres large, streaming + split norm", "... normalise step as hipk_gm_hcol_kernel + hipk_gm_scale_kernel"),
    HIPK_FORM_CB("gmres restart > 31", "the streaming kernels with H, R and the Givens pairs in the workspace"),
    HIPK_FORM_CB("gmres restart > 31 + split norm", "... normalise step as hipk_gm_hcol_kernel + hipk_gm_scale_kernel"),
};
#undef HIPK_FORM_T2
#undef HIPK_FORM_CG_LDS
#undef HIPK_FORM_BI_LDS
#undef HIPK_FORM_GM_LDS
#undef HIPK_FORM_CG_MID
#undef HIPK_FORM_BI_MID
#undef HIPK_FORM_GM_MID
#undef HIPK_FORM_CB

constexpr bool hipk_form_is_row(const char *name) {
    for (const hipk_form_row &r : hipk_solve_forms)
        if (hipk_sw_streq(r.name, name)) return true;
    return false;
}
template <bool in_table>
struct hipk_form_checked {
    static_assert(in_table, "not a row of hipk_solve_forms");
    static constexpr const char *get(const char *name) { return name; }
};
// `name` (a string literal) as a form; a string that is not a row does not compile
#define HIPK_FORM(name) (hipk_form_checked<hipk_form_is_row(name)>::get(name))
// ... of a kernel template over T: head "double," tail or head "float," tail
#define HIPK_FORM_OF_T(T, head, tail) (sizeof(T) == 8 ? HIPK_FORM(head "double," tail) : HIPK_FORM(head "float," tail))

// the form of this thread's last solve (hipk_last_solve_form); hipk_set_solve_path resets it to the path it records
void hipk_set_solve_form(const char *form);
