// Environment switches of libhipk: the ONE table of them and the only calls of getenv in csrc/.
// Defaults are the product's behaviour; the switches exist for tests and for A/B measurements ("Environment switches",
// lists the same rows; tests/test_switch_table.py keeps table, call sites and document in step).
#pragma once
#include <cstdint>
#include <cstdlib>
#include <cstring>

// how a switch's value is parsed
enum hipk_sw_kind {
    HIPK_SW_PRESENT,    // set at all means on -- also when set to 0 or to the empty string
    HIPK_SW_OFF_IF_0,   // on unless the value starts with '0'
    HIPK_SW_FORCE01,    // unset: the automatic choice; set: on exactly when the value starts with '1'
    HIPK_SW_INT,        // a decimal integer (atoll; not a number: 0), with the clamp its row states
    HIPK_SW_WORD,       // compared with the word its row states
};
struct hipk_sw_row {
    const char *name;
    hipk_sw_kind kind;
    const char *dflt, *read, *meaning, *used_by;   // read: when the value is looked at; used_by: test, tools A/B, user
};

// one row per switch, one line per row
static constexpr hipk_sw_row hipk_switches[] = {
    // ---- handle creation and the SpMV dispatch (hipk_api.hip)
    {"HIPK_SPMV_CODED", HIPK_SW_OFF_IF_0, "on", "handle creation", "0: build neither coded form, plain CSR kernels only", "test, tools A/B"},
    {"HIPK_SPMV_OFFSET_CODED", HIPK_SW_OFF_IF_0, "on", "handle creation", "0: skip the offset-coded form (variable coefficients stay on the CSR kernels)", "test"},
    {"HIPK_SPMV_CODED_LAYOUT", HIPK_SW_WORD, "sliced-ELL planes", "handle creation", "csr: pair codes in CSR order + row lengths; any other word is the default", "test, tools A/B"},
    {"HIPK_SPMV_UNIFORM", HIPK_SW_OFF_IF_0, "on", "handle creation", "0: no uniform-tile words, the coded SpMV reads every tile's code planes", "test"},
    {"HIPK_SPMV_MASKED", HIPK_SW_FORCE01, "off", "handle creation", "1: build the masked-tile analysis (fp64 pair codes); measured slower", "test"},
    {"HIPK_SPMV_SELL_CHUNKED", HIPK_SW_INT, "2", "handle creation; whether set: first coded SpMV of the process", "k: chunk-per-workgroup form when k x chunks >= resident workgroups; < 0 reads as 0 (never), 1 reads as 2 (quirk, kept); set at all also turns off the factor 4 of the two-rows-per-lane kernel", "test, tools A/B"},
    {"HIPK_SPMV_SELL_LOOP", HIPK_SW_INT, "1", "handle creation", "k: persistent grid = k x the resident workgroups, clamped to 1 .. 4", "test, tools A/B"},
    {"HIPK_SPMV_NO_PLAN_CACHE", HIPK_SW_PRESENT, "off", "first coded SpMV of the process", "resolve the coded SpMV's dispatch per launch instead of once per (handle, mode, geometry)", "test, tools A/B"},
    {"HIPK_SPMV_SELL_NO_MODE", HIPK_SW_PRESENT, "off", "first coded SpMV of the process", "run-time instead of compiled-in mode bits in the pair / two-rows-per-lane kernels", "test, tools A/B"},
    {"HIPK_SPMV_SELL_NO_WIDE", HIPK_SW_PRESENT, "off", "each SpMV dispatch", "the one-row-per-lane coded kernels instead of the two-rows-per-lane kernel", "test, tools A/B"},
    {"HIPK_SPMV_SELL_STRIDED", HIPK_SW_INT, "automatic", "each SpMV dispatch", "0 | nonzero: force the chunk walk | the grouped walk of the coded kernels (unset: by tiles per chunk)", "test, tools A/B"},
    {"HIPK_SPMV_SELL_NO_PAIR", HIPK_SW_PRESENT, "off", "first chunked coded SpMV of the process", "the one-tile-per-trip coded kernel instead of the pair kernel", "test, tools A/B"},
    {"HIPK_CHEB_FUSED", HIPK_SW_OFF_IF_0, "on", "each hipk_cheb_apply", "0: every Chebyshev step as SpMV + hipk_cheb_step_kernel instead of the SpMV's Chebyshev epilogue (same bits)", "test, tools A/B"},
    // ---- every solve loop (hipk_solve.h)
    {"HIPK_HOST_SIGNAL", HIPK_SW_OFF_IF_0, "on", "each solve", "0: follow the loop with stream-ordered reads of the device stop word instead of the pinned-host signal word", "test"},
    {"HIPK_PACE_TIMEOUT_US", HIPK_SW_INT, "200000", "each solve", "t: microseconds the signal word may stand still before the stream-ordered fallback; negative: ignored", "test"},
    {"HIPK_PACE_WINDOW", HIPK_SW_INT, "8", "each solve", "k: iterations the host may run ahead of the GPU; outside 1 .. 4096: ignored", "test, user"},
    {"HIPK_TEST_LDS_NOT_RESIDENT", HIPK_SW_INT, "unset", "each one-launch loop; each hand-back", "k: the k-th launch of a one-launch loop reports its workgroups as not co-resident, k < 2 (0 included) reads as 1; set at all: a hand-back does not set the process-wide latch", "test"},
    {"HIPK_NO_LDS_SPREAD", HIPK_SW_PRESENT, "off", "each solve", "9 .. 32 chunks: the launch sequences instead of the one-launch kernels spread over the chip (cg, bicgstab, gmres)", "test, tools A/B"},
    // ---- CG (hipk_cg.hip)
    {"HIPK_CG_NO_SMALL", HIPK_SW_PRESENT, "off", "each CG solve", "general launch sequence also for <= 8 reduction chunks; also keeps both one-launch loops away", "test"},
    {"HIPK_CG_NO_LDS_LOOP", HIPK_SW_PRESENT, "off", "each CG solve", "launch sequences instead of either one-launch loop (mid and LDS)", "test, tools A/B"},
    {"HIPK_CG_MID", HIPK_SW_OFF_IF_0, "on", "each CG solve", "0: no hipk_cg_mid_kernel; the LDS loop up to 32 chunks, else the launch sequences", "test, tools A/B"},
    {"HIPK_CG_MID_STRIDE", HIPK_SW_INT, "by chunk count", "each launch of the mid loop, plain CG only", "k: chunk-partial slots k x 16 B apart; outside 1 .. 16 reads as 16", "tools A/B"},
    {"HIPK_CG_MID_XCD", HIPK_SW_OFF_IF_0, "on", "each launch of the mid loop, plain CG only", "0: workgroup b takes row range b (no XCD-aware placement)", "tools A/B"},
    {"HIPK_CG_LAUNCH_ITS", HIPK_SW_INT, "16384", "each one-launch loop", "k: iterations one launch of a one-launch CG loop may run, at least 1", "test"},
    {"HIPK_CG_LOOP_AGENT", HIPK_SW_PRESENT, "off", "each LDS loop", "agent-scope hand-offs in hipk_cg_solve_lds_kernel also on one XCD", "test"},
    {"HIPK_CG_TWO_LAUNCH", HIPK_SW_OFF_IF_0, "on", "each plain CG solve", "0: the three-launch iteration instead of hipk_cg2_spmv_kernel + hipk_cg2_update_kernel", "test, tools A/B"},
    {"HIPK_CG_DEFER_X", HIPK_SW_OFF_IF_0, "on", "each plain CG solve", "0: every direction launch updates x (hipk_cg_direction_kernel)", "test, tools A/B"},
    {"HIPK_CG_FUSE_UPDATE", HIPK_SW_FORCE01, "automatic", "each plain CG solve", "0 | 1: the SpMV and the update step as two launches | as hipk_cg_fuse_update_kernel where the form applies (unset: fused where it applies)", "test, tools A/B"},
    {"HIPK_CG_FUSE_DIRECTION", HIPK_SW_FORCE01, "automatic", "each plain CG solve", "0 | 1: the direction step of the fused deferred-x sequence as hipk_cg_pdir_kernel / hipk_cg_xdir_kernel launches | as the tail of hipk_cg_fuse_update_kernel where the form applies (unset: the tail where it applies)", "test, tools A/B"},
    {"HIPK_CG_FUSE_KEEP_P", HIPK_SW_OFF_IF_0, "on", "each plain CG solve", "0: the direction tail of hipk_cg_fuse_update_kernel loads all of p_k again instead of keeping the uniform tiles' rows in the walk's registers (same bits)", "test, tools A/B"},
    {"HIPK_TEST_CG_FUSE_DIR_GIVE_UP", HIPK_SW_INT, "unset", "each fused CG sequence", "k: the collectors of the direction tail's hand-off at iteration k behave as if their poll had run out (the solve goes on with the separate kernels)", "test"},
    {"HIPK_TEST_CG_FUSE_GIVE_UP", HIPK_SW_INT, "unset", "each fused CG sequence", "k: the collectors of hipk_cg_fuse_update_kernel at iteration k behave as if their poll had run out (the solve goes on with the separate kernels)", "test"},
    {"HIPK_TEST_CG_FUSE_GIVE_UP_WHO", HIPK_SW_INT, "unset", "each fused CG sequence", "s: only collector s (0 .. 7) obeys HIPK_TEST_CG_FUSE_GIVE_UP / HIPK_TEST_CG_FUSE_DIR_GIVE_UP; outside 0 .. 7: ignored (all eight do)", "test"},
    {"HIPK_CG_STREAMS", HIPK_SW_FORCE01, "automatic", "each plain CG solve", "0 | 1: force the vector kernels' cache policy (unset: streams when x, r, p, Ap exceed 384 MiB)", "test"},
    {"HIPK_CG_FLAT_DIRECTION", HIPK_SW_FORCE01, "automatic", "each plain CG solve", "0 | 1: with the streaming policy, the direction step per chunk | as scalars launch + flat grid (unset: flat when a vector exceeds 256 MiB)", "test, tools A/B"},
    // ---- BiCGStab (hipk_bicgstab.hip)
    {"HIPK_BICGSTAB_NO_SMALL", HIPK_SW_PRESENT, "off", "each BiCGStab solve", "general launch sequence also for <= 8 reduction chunks; also keeps both one-launch loops away", "test"},
    {"HIPK_BICGSTAB_NO_LDS_LOOP", HIPK_SW_PRESENT, "off", "each BiCGStab solve", "five launches per iteration instead of either one-launch loop (mid and LDS)", "test, tools A/B"},
    {"HIPK_BICGSTAB_MID", HIPK_SW_OFF_IF_0, "on", "each BiCGStab solve", "0: no hipk_bi_mid_kernel; the LDS loop up to 32 chunks, else the launch sequence", "test, tools A/B"},
    {"HIPK_BICGSTAB_LAUNCH_ITS", HIPK_SW_INT, "8192", "each one-launch loop", "k: iterations one launch of a one-launch BiCGStab loop may run, at least 1", "test"},
    {"HIPK_BICGSTAB_LOOP_AGENT", HIPK_SW_PRESENT, "off", "each LDS loop", "agent-scope hand-offs in hipk_bi_solve_lds_kernel also on one XCD", "test"},
    // ---- GMRES (hipk_gmres.hip)
    {"HIPK_GMRES_NO_SMALL", HIPK_SW_PRESENT, "off", "each GMRES solve", "general launch sequence also for <= 8 reduction chunks; also keeps the spread whole-solve kernel away", "test"},
    {"HIPK_GMRES_NO_WIDE", HIPK_SW_PRESENT, "off", "each GMRES solve", "small systems: the 256-thread multi-dot / update kernels instead of the wide ones (and no one-launch cycle)", "test"},
    {"HIPK_GMRES_NO_CYCLE", HIPK_SW_PRESENT, "off", "each GMRES solve", "one launch per kernel instead of any one-launch cycle (small, LDS, mid)", "test, tools A/B"},
    {"HIPK_GMRES_NO_LDS_CYCLE", HIPK_SW_PRESENT, "off", "each GMRES solve", "hipk_gm_cycle_small_kernel (one launch per restart cycle) instead of hipk_gm_solve_lds_kernel", "test, tools A/B"},
    {"HIPK_GM_CYCLE_AGENT", HIPK_SW_PRESENT, "off", "each GMRES solve", "agent-scope hand-offs in hipk_gm_solve_lds_kernel also on one XCD", "test"},
    {"HIPK_GM_LAUNCH_CYCLES", HIPK_SW_INT, "64", "each launch of a one-launch cycle", "k: restart cycles one launch of hipk_gm_solve_lds_kernel may run (no clamp)", "test"},
    {"HIPK_GMRES_NO_STREAM", HIPK_SW_PRESENT, "off", "each GMRES solve", "large systems, restart <= 31: the first multi-dot / update kernels instead of the streaming ones", "test, tools A/B"},
    {"HIPK_GMRES_MID", HIPK_SW_OFF_IF_0, "on", "each GMRES solve", "0: the launch sequence per Arnoldi step instead of hipk_gm_mid_kernel", "test, tools A/B"},
    {"HIPK_GMRES_MID_MIN", HIPK_SW_INT, "32", "each GMRES solve", "k: hipk_gm_mid_kernel from k + 1 chunks, floor 8 (A/B against the whole-solve kernel of 9 .. 32 chunks)", "tools A/B"},
    {"HIPK_GM_MD_WIDE", HIPK_SW_INT, "0", "each GMRES solve", "nonzero: multi-dot with up to 32 columns per workgroup; measured slower", "tools A/B"},
    {"HIPK_GM_SPLIT_NORM", HIPK_SW_INT, "by chunk count", "each GMRES solve", "0 | nonzero: the one-kernel normalise step | scalars launch + flat scale kernel (large systems)", "test, tools A/B"},
    {"HIPK_GM_NRES", HIPK_SW_INT, "5", "each GMRES solve", "k: basis columns read with the default cache policy, the rest non-temporal (no clamp)", "test, tools A/B"},
    {"HIPK_GM_SPEC", HIPK_SW_INT, "1", "each GMRES solve", "second CGS pass launched at every step (0), where predicted (1), or learned from scratch (2)", "test, tools A/B"},
    {"HIPK_GM_STAMPS", HIPK_SW_PRESENT, "off", "each launch and the end of a small-system GMRES solve", "stamps build only: print the per-phase shader clocks of the cycle kernels", "tools A/B"},
    // ---- many small systems (hipk_batch.hip)
    {"HIPK_BATCH_LAUNCH_ITS", HIPK_SW_INT, "16384", "each batch solve", "k: iterations per system one launch of a batch kernel may run, at least 1", "test"},
    // ---- row-partitioned CG (hipk_dist.hip)
    {"HIPK_DIST_OVERLAP", HIPK_SW_INT, "0", "each hipk_dist_cg_solve", "nonzero: x += alpha p on a side stream beside the second collective; measured slower", "test"},
    {"HIPK_DIST_FUSED", HIPK_SW_OFF_IF_0, "on", "each hipk_dist_cg_solve", "0: the collective entry points also on a communicator with a fused area", "user"},
};

constexpr bool hipk_sw_streq(const char *a, const char *b) {
    while (*a && *a == *b) ++a, ++b;
    return *a == *b;
}
// compile time: `name` is a row, and of kind `kind` (any: whether it is set may be asked of every row)
constexpr bool hipk_sw_is_row(const char *name, hipk_sw_kind kind, bool any = false) {
    for (const hipk_sw_row &r : hipk_switches)
        if (hipk_sw_streq(r.name, name)) return any || r.kind == kind;
    return false;
}
template <bool in_table>
struct hipk_sw_checked {
    static_assert(in_table, "not a row of hipk_switches, or a row of another kind");
    static const char *get(const char *name) { return getenv(name); }
};
// the value of the switch `name` (a string literal), or null; a wrong name or kind does not compile
#define HIPK_SW_GET(name, ...) (hipk_sw_checked<hipk_sw_is_row(name, __VA_ARGS__)>::get(name))

// The accessors hide the parsing and nothing else: every call reads the environment, so a site that wants a value once per
// process or per handle keeps it in a static or in the handle, and a site that reads per launch just calls.
#define hipk_sw_present(name) (HIPK_SW_GET(name, HIPK_SW_PRESENT, true) != nullptr)
#define hipk_sw_enabled(name) hipk_sw_parse_enabled(HIPK_SW_GET(name, HIPK_SW_OFF_IF_0))
#define hipk_sw_force(name, automatic) hipk_sw_parse_force(HIPK_SW_GET(name, HIPK_SW_FORCE01), (automatic))
#define hipk_sw_int(name, ...) hipk_sw_parse_int(HIPK_SW_GET(name, HIPK_SW_INT), __VA_ARGS__)   // (name, dflt[, lo, hi])
#define hipk_sw_word_is(name, word) hipk_sw_parse_word(HIPK_SW_GET(name, HIPK_SW_WORD), (word))

static inline bool hipk_sw_parse_enabled(const char *e) { return !(e && e[0] == '0'); }
static inline bool hipk_sw_parse_force(const char *e, bool automatic) { return e ? e[0] == '1' : automatic; }
// unset: dflt; the clamp applies to both
static inline int64_t hipk_sw_parse_int(const char *e, int64_t dflt, int64_t lo = INT64_MIN, int64_t hi = INT64_MAX) {
    const int64_t v = e ? (int64_t)atoll(e) : dflt;
    return v < lo ? lo : v > hi ? hi : v;
}
static inline bool hipk_sw_parse_word(const char *e, const char *word) { return e && strcmp(e, word) == 0; }
