"""One row per case of tests/test_gpu_solver_forms.py: the forms a single-device solve can finish in (hipk_last_solve_form, the
table csrc/hipk_forms.h) outside the mid loops that tests/test_gpu_mid_oracle.py pins -- the whole-solve LDS kernels on one XCD
and spread over the chip, the small and general launch sequences, the two-launch CG iteration on both sides of each of its
guards, and GMRES at restart 32 .. 255.  Expected paths and forms are written literally from reading the dispatch code
(hipk_cg_path_*, hipk_bi_path_*, hipk_gm_path_choose); tests/test_form_cases.py checks, without a GPU, that every form of the
library has a case here (or in the mid table) and that each matrix has the shape its expected form implies.

Not reachable as a bitwise case: hipk_gm_solve_lds_bytes<T>(m) is 79 888 bytes at its largest (fp64, m = 31), below the
80 KB guard of hipk_gm_path_choose, so that guard has one side only."""
import json
import os

import numpy as np
import scipy.sparse as sp

from _oracle_cases import _band, _signed_band

CH = 2048            # rows per reduction chunk below 4 M rows (hipk_chunk_size)
TILE = 256
N46 = 45 * CH + 37
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _n_cu():
    """Compute units of the device; 256 (an MI355X) where there is none (the table checks of test_form_cases.py)."""
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256


def _g1():
    """Most chunks the one-XCD LDS loops take: 8 g workgroups on an eighth of the compute units, two each; never above 8."""
    return max(1, min(8, 2 * (_n_cu() // 8) // 8))


def _with_pair(M, i, j):
    """M plus one symmetric off-diagonal pair (i, j), diagonals raised to keep it diagonally dominant."""
    E = sp.csr_matrix(([-0.25, -0.25, 0.25, 0.25], ([i, j, i, j], [j, i, i, j])), shape=M.shape)
    R = (M + E).tocsr()
    R.sort_indices()
    return R


def _star(n, hub, k):
    """Tridiagonal SPD matrix whose row `hub` has k more entries, 300 columns apart (their partner rows one more each)."""
    M = _band(n, (1,))
    for q in range(k):
        M = _with_pair(M, hub, hub + 300 * (q + 1))
    return M


def _dense(n, sym, seed):
    rng = np.random.default_rng(seed)
    D = rng.uniform(-1.0, -0.1, (n, n))
    if sym:
        D = np.triu(D, 1) + np.triu(D, 1).T
    np.fill_diagonal(D, 0.0)
    np.fill_diagonal(D, np.abs(D).sum(axis=1) + 0.5)
    M = sp.csr_matrix(D)
    M.sort_indices()
    return M


def _breakdown(code):
    d = json.load(open(os.path.join(GOLDEN, "bicgstab_breakdown.json")))[code]
    M = sp.csr_matrix(np.asarray(d["A"], dtype=np.float64))
    M.sort_indices()
    return M


OFF12, OFF13, OFF32, OFF33 = (1, 2, 3, 4, 5), (1, 2, 3, 4, 5, 6), tuple(range(1, 16)), tuple(range(1, 17))
FAR = (4096, 12288, 20480, 28672)   # aligned far bands: own 8 window tiles + 8 x 8 = 72 > kMidPlanSlots

MATRICES = {
    # ---- one XCD (<= 8 chunks): ragged single chunk, a chunk exactly, two chunks, the most chunks, and that with a ragged last one
    "s5_n35": lambda: _band(35, (1, 2)),
    "s5_c1": lambda: _band(CH, (1, 2)),
    "s5_c1r": lambda: _band(CH + 37, (1, 2)),
    "s5_g1": lambda: _band(_g1() * CH, (1, 2)),
    "s5_g1r": lambda: _band((_g1() - 1) * CH + 1, (1, 2)),
    "n5_n35": lambda: _band(35, (1, 2), sym=False, seed=1),
    "n5_c1": lambda: _band(CH, (1, 2), sym=False, seed=1),
    "n5_c1r": lambda: _band(CH + 37, (1, 2), sym=False, seed=1),
    "n5_g1": lambda: _band(_g1() * CH, (1, 2), sym=False, seed=1),
    "n5_g1r": lambda: _band((_g1() - 1) * CH + 1, (1, 2), sym=False, seed=1),
    # rows of 12 (kCgRowRegs, kBiRowRegs), 13, 32 (HIPK_LONG_ROW) and 33 entries; a dense matrix (row-per-wavefront SpMV)
    "s12_c1r": lambda: _band(CH + 37, OFF12, match=300),
    "n12_c1r": lambda: _band(CH + 37, OFF12, match=300, sym=False, seed=1),
    "s13_c1r": lambda: _band(CH + 37, OFF13),
    "n13_c1r": lambda: _band(CH + 37, OFF13, sym=False, seed=1),
    "s32_c1r": lambda: _band(CH + 37, OFF32, match=300),
    "n32_c1r": lambda: _band(CH + 37, OFF32, match=300, sym=False, seed=1),
    "n33_c1r": lambda: _band(CH + 37, OFF33, sym=False, seed=1),
    "dense300s": lambda: _dense(300, True, 3),
    "dense300n": lambda: _dense(300, False, 4),
    "s13_c8": lambda: _band(8 * CH, OFF13),
    "s13_c9": lambda: _band(8 * CH + 1, OFF13),
    "n13_c8": lambda: _band(8 * CH, OFF13, sym=False, seed=1),
    "n13_c9": lambda: _band(8 * CH + 1, OFF13, sym=False, seed=1),
    # ---- spread over the chip (9 .. 32 chunks) and its far side
    "s5_c9": lambda: _band(8 * CH + 1, (1, 2)),
    "s5_c32": lambda: _band(32 * CH, (1, 2)),
    "s5_c33": lambda: _band(32 * CH + 1, (1, 2)),             # 1280 entries in a full tile: the fp64 capacity of two-launch CG
    "n5_c9": lambda: _band(8 * CH + 1, (1, 2), sym=False, seed=1),
    "n5_c32": lambda: _band(32 * CH, (1, 2), sym=False, seed=1),
    "n5_c33": lambda: _band(32 * CH + 1, (1, 2), sym=False, seed=1),
    "sfar_c32": lambda: _band(32 * CH, FAR),                  # 9-entry rows whose window the mid loops refuse (72 tiles)
    "nfar_c32": lambda: _band(32 * CH, FAR, sym=False, seed=1),
    # ---- two-launch CG (33 .. 150 chunks, tiles of <= 1280 / 2048 entries, rows of <= 32)
    "s5_c46": lambda: _band(N46, (1, 2)),
    "s5_c150": lambda: _band(150 * CH, (1, 2)),
    "s5_c151": lambda: _band(150 * CH + 1, (1, 2)),
    "s5x_c33": lambda: _with_pair(_band(32 * CH + 1, (1, 2)), 3 * TILE + 7, 10 * TILE + 9),      # two tiles of 1281
    "s8_c33": lambda: _band(32 * CH + 1, (1, 2, 3), match=300),                                # 2048 in a full tile (fp32 capacity)
    "s8x_c33": lambda: _with_pair(_band(32 * CH + 1, (1, 2, 3), match=300), 5 * TILE + 7, 10 * TILE + 9),   # two tiles of 2049
    "star32_c33": lambda: _star(32 * CH + 1, 20000, 29),
    "star33_c33": lambda: _star(32 * CH + 1, 20000, 30),
    "reach_out": lambda: _band(80 * CH, (1, 64768)),          # a block spans 514 tiles > kMidPlanRange: the mid loop refuses
    # ---- breakdowns
    "bd-10": lambda: _breakdown("-10"),
    "bd-11": lambda: _breakdown("-11"),
    "eye5": lambda: sp.identity(5, format="csr"),
}
FIXED_B = {"bd-10": lambda: np.array(json.load(open(os.path.join(GOLDEN, "bicgstab_breakdown.json")))["-10"]["b"]),
           "bd-11": lambda: np.array(json.load(open(os.path.join(GOLDEN, "bicgstab_breakdown.json")))["-11"]["b"])}

# what each matrix is FOR, checked in numpy by test_form_cases.py (g1: _g1() chunks): chunks g, longest row W, most entries in a
# 256-row tile, most window tiles (distinct 256-column tiles a 2048-row block references), widest tile range of a block
MATRIX_PROPS = {
    "s5_n35": dict(g=1, W=5), "s5_c1": dict(g=1, W=5), "s5_c1r": dict(g=2, W=5), "s5_g1": dict(g="g1", W=5), "s5_g1r": dict(g="g1", W=5),
    "n5_n35": dict(g=1, W=5), "n5_c1": dict(g=1, W=5), "n5_c1r": dict(g=2, W=5), "n5_g1": dict(g="g1", W=5), "n5_g1r": dict(g="g1", W=5),
    "s12_c1r": dict(g=2, W=12), "n12_c1r": dict(g=2, W=12), "s13_c1r": dict(g=2, W=13), "n13_c1r": dict(g=2, W=13),
    "s32_c1r": dict(g=2, W=32), "n32_c1r": dict(g=2, W=32), "n33_c1r": dict(g=2, W=33),
    "dense300s": dict(g=1, W=300), "dense300n": dict(g=1, W=300),
    "s13_c8": dict(g=8, W=13), "s13_c9": dict(g=9, W=13), "n13_c8": dict(g=8, W=13), "n13_c9": dict(g=9, W=13),
    "s5_c9": dict(g=9, W=5), "s5_c32": dict(g=32, W=5), "s5_c33": dict(g=33, W=5, tile=1280),
    "n5_c9": dict(g=9, W=5), "n5_c32": dict(g=32, W=5), "n5_c33": dict(g=33, W=5),
    "sfar_c32": dict(g=32, W=9, slots=72), "nfar_c32": dict(g=32, W=9, slots=72),
    "s5_c46": dict(g=46, W=5, tile=1280), "s5_c150": dict(g=150, W=5, tile=1280), "s5_c151": dict(g=151, W=5, tile=1280),
    "s5x_c33": dict(g=33, W=6, tile=1281), "s8_c33": dict(g=33, W=8, tile=2048), "s8x_c33": dict(g=33, W=9, tile=2049),
    "star32_c33": dict(g=33, W=32, tile=797), "star33_c33": dict(g=33, W=33, tile=798),
    "reach_out": dict(g=80, W=5, tile=1280, range=514),
    "bd-10": dict(g=1, W=3), "bd-11": dict(g=1, W=2), "eye5": dict(g=1, W=1),
}

F64, F32 = "f64", "f32"
LS = "launch sequence"
CG_LDS, BI_LDS, GM_LDS, GM_SMALL = "hipk_cg_solve_lds_kernel", "hipk_bi_solve_lds_kernel", "hipk_gm_solve_lds_kernel", "hipk_gm_cycle_small_kernel"
# forms (csrc/hipk_forms.h)
CG2_64 = "cg two-launch: hipk_cg2_spmv_kernel<double,1280> + hipk_cg2_update_kernel"
CG2_32 = "cg two-launch: hipk_cg2_spmv_kernel<float,2048> + hipk_cg2_update_kernel"
CG3S, CG3, PCG3 = "cg three-launch, small", "cg three-launch", "pcg three-launch, Jacobi"
BI5S, BI5, BI5SJ, BI5J = "bicgstab five-launch, small", "bicgstab five-launch", "bicgstab five-launch, small, Jacobi", "bicgstab five-launch, Jacobi"
GSW, GS256, GLF, GLS, GBIG = "gmres small + wide", "gmres small + 256-thread", "gmres large, first kernels", "gmres large, streaming", "gmres restart > 31"
SPLIT, CB = " + split norm", ", callback M"
MID0, BMID0 = {"HIPK_CG_MID": "0"}, {"HIPK_BICGSTAB_MID": "0"}
NOSPREAD = {"HIPK_NO_LDS_SPREAD": "1"}
NR1, NR2 = {"HIPK_TEST_LDS_NOT_RESIDENT": "1"}, {"HIPK_TEST_LDS_NOT_RESIDENT": "2"}
CITS7, BITS7, GCYC2 = {"HIPK_CG_LAUNCH_ITS": "7"}, {"HIPK_BICGSTAB_LAUNCH_ITS": "7"}, {"HIPK_GM_LAUNCH_CYCLES": "2"}

# solve options: tol / maxiter (CG, BiCGStab: iterations; GMRES: restart cycles), restart, solve_method; callback: M = (v -> dinv * v)
# through hipk_pbicgstab_solve_cb / hipk_pgmres_solve_cb
KW = dict(tol=1e-8, maxiter=400)
KW32 = dict(tol=1e-4, maxiter=200)
KW12 = lambda mi: dict(tol=1e-12, maxiter=mi)   # noqa: E731  (runs into maxiter)
GM = dict(tol=1e-8, restart=20, maxiter=3)
GM32 = dict(tol=1e-4, restart=20, maxiter=3)
INC = {"solve_method": "incremental"}


def GMR(restart, maxiter=2, tol=1e-12, **more):
    return dict(tol=tol, restart=restart, maxiter=maxiter, **more)


# (id, solver, matrix, dtype, solve options, environment, x0: None | "rand" | "exact" (b = A x0) | "fixture", expected
#  hipk_last_solve_path, expected hipk_last_solve_form)
CASES = [
    # ================================================================== the LDS whole-solve kernels on ONE XCD (<= 8 chunks)
    # ---- CG
    ("cg-lds-n35-f64", "cg", "s5_n35", F64, KW, {}, None, CG_LDS, "hipk_cg_solve_lds_kernel<double,true,false>"),
    ("cg-lds-n35-f32", "cg", "s5_n35", F32, KW32, {}, None, CG_LDS, "hipk_cg_solve_lds_kernel<float,true,false>"),
    ("cg-lds-c1-f64", "cg", "s5_c1", F64, KW, {}, None, CG_LDS, "hipk_cg_solve_lds_kernel<double,true,false>"),
    ("cg-lds-c1r-f32", "cg", "s5_c1r", F32, KW32, {}, None, CG_LDS, "hipk_cg_solve_lds_kernel<float,true,false>"),
    ("cg-lds-g1-f64", "cg", "s5_g1", F64, KW, {}, None, CG_LDS, "hipk_cg_solve_lds_kernel<double,true,false>"),
    ("cg-lds-g1-f32", "cg", "s5_g1", F32, KW32, {}, None, CG_LDS, "hipk_cg_solve_lds_kernel<float,true,false>"),
    ("cg-lds-g1r-f64", "cg", "s5_g1r", F64, KW, {}, "rand", CG_LDS, "hipk_cg_solve_lds_kernel<double,true,false>"),
    ("cg-lds-row12-f64", "cg", "s12_c1r", F64, KW, {}, None, CG_LDS, "hipk_cg_solve_lds_kernel<double,true,false>"),
    ("cg-lds-row12-f32", "cg", "s12_c1r", F32, KW32, {}, None, CG_LDS, "hipk_cg_solve_lds_kernel<float,true,false>"),
    ("cg-small-row13-f64", "cg", "s13_c1r", F64, KW, {}, None, LS, CG3S),
    ("cg-small-row13-f32", "cg", "s13_c1r", F32, KW32, {}, None, LS, CG3S),
    ("cg-lds-warm-f32", "cg", "s5_c1r", F32, KW32, {}, "rand", CG_LDS, "hipk_cg_solve_lds_kernel<float,true,false>"),
    ("cg-lds-stop0-f64", "cg", "s5_c1r", F64, dict(tol=0.5, maxiter=400), {}, "exact", CG_LDS, "hipk_cg_solve_lds_kernel<double,true,false>"),
    ("cg-lds-maxiter0-f64", "cg", "s5_c1r", F64, KW12(0), {}, None, LS, CG3S),   # the one-launch loops need maxiter > 0
    ("cg-lds-maxiter1-f64", "cg", "s5_c1r", F64, KW12(1), {}, "rand", CG_LDS, "hipk_cg_solve_lds_kernel<double,true,false>"),
    ("cg-lds-its7-maxiter7-f64", "cg", "s5_c1r", F64, KW12(7), CITS7, None, CG_LDS, "hipk_cg_solve_lds_kernel<double,true,false>"),
    ("cg-lds-its7-maxiter8-f64", "cg", "s5_c1r", F64, KW12(8), CITS7, None, CG_LDS, "hipk_cg_solve_lds_kernel<double,true,false>"),
    ("cg-lds-its7-f32", "cg", "s5_g1r", F32, KW32, CITS7, "rand", CG_LDS, "hipk_cg_solve_lds_kernel<float,true,false>"),
    ("cg-lds-agent-f64", "cg", "s5_g1r", F64, KW, {"HIPK_CG_LOOP_AGENT": "1"}, None, CG_LDS, "hipk_cg_solve_lds_kernel<double,false,false>"),
    ("cg-lds-agent-f32", "cg", "s5_c1r", F32, KW32, {"HIPK_CG_LOOP_AGENT": "1"}, None, CG_LDS, "hipk_cg_solve_lds_kernel<float,false,false>"),
    # ---- Jacobi PCG
    ("pcg-lds-n35-f64", "pcg", "s5_n35", F64, KW, {}, None, CG_LDS, "hipk_cg_solve_lds_kernel<double,true,true>"),
    ("pcg-lds-n35-f32", "pcg", "s5_n35", F32, KW32, {}, "rand", CG_LDS, "hipk_cg_solve_lds_kernel<float,true,true>"),
    ("pcg-lds-c1-f32", "pcg", "s5_c1", F32, KW32, {}, None, CG_LDS, "hipk_cg_solve_lds_kernel<float,true,true>"),
    ("pcg-lds-c1r-f64", "pcg", "s5_c1r", F64, KW, {}, None, CG_LDS, "hipk_cg_solve_lds_kernel<double,true,true>"),
    ("pcg-lds-g1-f64", "pcg", "s5_g1", F64, KW, {}, None, CG_LDS, "hipk_cg_solve_lds_kernel<double,true,true>"),
    ("pcg-lds-g1r-f32", "pcg", "s5_g1r", F32, KW32, {}, None, CG_LDS, "hipk_cg_solve_lds_kernel<float,true,true>"),
    ("pcg-lds-row12-f64", "pcg", "s12_c1r", F64, KW, {}, "rand", CG_LDS, "hipk_cg_solve_lds_kernel<double,true,true>"),
    ("pcg-seq-row13-f64", "pcg", "s13_c1r", F64, KW, {}, None, LS, PCG3),
    ("pcg-lds-stop0-f64", "pcg", "s5_c1r", F64, dict(tol=0.5, maxiter=400), {}, "exact", CG_LDS, "hipk_cg_solve_lds_kernel<double,true,true>"),
    ("pcg-lds-maxiter0-f64", "pcg", "s5_c1r", F64, KW12(0), {}, None, LS, PCG3),
    ("pcg-lds-maxiter1-f32", "pcg", "s5_c1r", F32, KW12(1), {}, None, CG_LDS, "hipk_cg_solve_lds_kernel<float,true,true>"),
    ("pcg-lds-its7-maxiter7-f64", "pcg", "s5_c1r", F64, KW12(7), CITS7, None, CG_LDS, "hipk_cg_solve_lds_kernel<double,true,true>"),
    ("pcg-lds-its7-maxiter8-f64", "pcg", "s5_c1r", F64, KW12(8), CITS7, "rand", CG_LDS, "hipk_cg_solve_lds_kernel<double,true,true>"),
    ("pcg-lds-agent-f64", "pcg", "s5_c1r", F64, KW, {"HIPK_CG_LOOP_AGENT": "1"}, None, CG_LDS, "hipk_cg_solve_lds_kernel<double,false,true>"),
    ("pcg-lds-agent-f32", "pcg", "s5_g1r", F32, KW32, {"HIPK_CG_LOOP_AGENT": "1"}, None, CG_LDS, "hipk_cg_solve_lds_kernel<float,false,true>"),
    # ---- BiCGStab and Jacobi BiCGStab
    ("bicgstab-lds-n35-f64", "bicgstab", "n5_n35", F64, KW, {}, None, BI_LDS, "hipk_bi_solve_lds_kernel<double,true,false>"),
    ("bicgstab-lds-n35-f32", "bicgstab", "n5_n35", F32, KW32, {}, None, BI_LDS, "hipk_bi_solve_lds_kernel<float,true,false>"),
    ("bicgstab-lds-c1-f64", "bicgstab", "n5_c1", F64, KW, {}, None, BI_LDS, "hipk_bi_solve_lds_kernel<double,true,false>"),
    ("bicgstab-lds-c1r-f32", "bicgstab", "n5_c1r", F32, KW32, {}, None, BI_LDS, "hipk_bi_solve_lds_kernel<float,true,false>"),
    ("bicgstab-lds-g1-f64", "bicgstab", "n5_g1", F64, KW, {}, None, BI_LDS, "hipk_bi_solve_lds_kernel<double,true,false>"),
    ("bicgstab-lds-g1r-f32", "bicgstab", "n5_g1r", F32, KW32, {}, "rand", BI_LDS, "hipk_bi_solve_lds_kernel<float,true,false>"),
    ("bicgstab-lds-row12-f64", "bicgstab", "n12_c1r", F64, KW, {}, None, BI_LDS, "hipk_bi_solve_lds_kernel<double,true,false>"),
    ("bicgstab-lds-row12-f32", "bicgstab", "n12_c1r", F32, KW32, {}, None, BI_LDS, "hipk_bi_solve_lds_kernel<float,true,false>"),
    ("bicgstab-small-row13-f64", "bicgstab", "n13_c1r", F64, KW, {}, None, LS, BI5S),
    ("bicgstab-small-row13-f32", "bicgstab", "n13_c1r", F32, KW32, {}, None, LS, BI5S),
    ("bicgstab-lds-stop0-f64", "bicgstab", "n5_c1r", F64, dict(tol=0.5, maxiter=300), {}, "exact", BI_LDS, "hipk_bi_solve_lds_kernel<double,true,false>"),
    ("bicgstab-lds-maxiter0-f64", "bicgstab", "n5_c1r", F64, KW12(0), {}, None, LS, BI5S),
    ("bicgstab-lds-maxiter1-f64", "bicgstab", "n5_c1r", F64, KW12(1), {}, "rand", BI_LDS, "hipk_bi_solve_lds_kernel<double,true,false>"),
    ("bicgstab-lds-its7-maxiter7-f64", "bicgstab", "n5_c1r", F64, KW12(7), BITS7, None, BI_LDS, "hipk_bi_solve_lds_kernel<double,true,false>"),
    ("bicgstab-lds-its7-maxiter8-f64", "bicgstab", "n5_c1r", F64, KW12(8), BITS7, None, BI_LDS, "hipk_bi_solve_lds_kernel<double,true,false>"),
    ("bicgstab-lds-agent-f64", "bicgstab", "n5_g1r", F64, KW, {"HIPK_BICGSTAB_LOOP_AGENT": "1"}, None, BI_LDS, "hipk_bi_solve_lds_kernel<double,false,false>"),
    ("bicgstab-lds-agent-f32", "bicgstab", "n5_c1r", F32, KW32, {"HIPK_BICGSTAB_LOOP_AGENT": "1"}, None, BI_LDS, "hipk_bi_solve_lds_kernel<float,false,false>"),
    ("bicgstab-lds-breakdown-rho-f64", "bicgstab", "bd-10", F64, dict(tol=1e-12, maxiter=200), {}, "fixture", BI_LDS, "hipk_bi_solve_lds_kernel<double,true,false>"),
    ("bicgstab-lds-breakdown-omega-f64", "bicgstab", "bd-11", F64, dict(tol=1e-12, maxiter=200), {}, "fixture", BI_LDS, "hipk_bi_solve_lds_kernel<double,true,false>"),
    ("pbicgstab-lds-n35-f64", "pbicgstab", "n5_n35", F64, KW, {}, "rand", BI_LDS, "hipk_bi_solve_lds_kernel<double,true,true>"),
    ("pbicgstab-lds-c1-f32", "pbicgstab", "n5_c1", F32, KW32, {}, None, BI_LDS, "hipk_bi_solve_lds_kernel<float,true,true>"),
    ("pbicgstab-lds-c1r-f64", "pbicgstab", "n5_c1r", F64, KW, {}, None, BI_LDS, "hipk_bi_solve_lds_kernel<double,true,true>"),
    ("pbicgstab-lds-g1-f32", "pbicgstab", "n5_g1", F32, KW32, {}, None, BI_LDS, "hipk_bi_solve_lds_kernel<float,true,true>"),
    ("pbicgstab-lds-g1r-f64", "pbicgstab", "n5_g1r", F64, KW, {}, None, BI_LDS, "hipk_bi_solve_lds_kernel<double,true,true>"),
    ("pbicgstab-lds-row12-f64", "pbicgstab", "n12_c1r", F64, KW, {}, None, BI_LDS, "hipk_bi_solve_lds_kernel<double,true,true>"),
    ("pbicgstab-small-row13-f64", "pbicgstab", "n13_c1r", F64, KW, {}, None, LS, BI5SJ),
    ("pbicgstab-lds-its7-maxiter8-f32", "pbicgstab", "n5_c1r", F32, KW12(8), BITS7, None, BI_LDS, "hipk_bi_solve_lds_kernel<float,true,true>"),
    ("pbicgstab-lds-agent-f64", "pbicgstab", "n5_c1r", F64, KW, {"HIPK_BICGSTAB_LOOP_AGENT": "1"}, None, BI_LDS, "hipk_bi_solve_lds_kernel<double,false,true>"),
    ("pbicgstab-lds-agent-f32", "pbicgstab", "n5_g1r", F32, KW32, {"HIPK_BICGSTAB_LOOP_AGENT": "1"}, "rand", BI_LDS, "hipk_bi_solve_lds_kernel<float,false,true>"),
    # ---- GMRES and Jacobi GMRES (rows of up to 32 entries stay in the kernel: the rest of a row beyond 12 is read from memory)
    ("gmres-lds-n35-f64", "gmres", "n5_n35", F64, GM, {}, None, GM_LDS, "hipk_gm_solve_lds_kernel<double,true>"),
    ("gmres-lds-n35-f32", "gmres", "n5_n35", F32, GM32, {}, None, GM_LDS, "hipk_gm_solve_lds_kernel<float,true>"),
    ("gmres-lds-c1-f64", "gmres", "n5_c1", F64, GM, {}, None, GM_LDS, "hipk_gm_solve_lds_kernel<double,true>"),
    ("gmres-lds-c1r-f32", "gmres", "n5_c1r", F32, GM32, {}, None, GM_LDS, "hipk_gm_solve_lds_kernel<float,true>"),
    ("gmres-lds-g1-f64", "gmres", "n5_g1", F64, GM, {}, None, GM_LDS, "hipk_gm_solve_lds_kernel<double,true>"),
    ("gmres-lds-g1-f32", "gmres", "n5_g1", F32, GM32, {}, None, GM_LDS, "hipk_gm_solve_lds_kernel<float,true>"),
    ("gmres-lds-g1r-f64", "gmres", "n5_g1r", F64, GM, {}, "rand", GM_LDS, "hipk_gm_solve_lds_kernel<double,true>"),
    ("gmres-lds-row12-f64", "gmres", "n12_c1r", F64, GM, {}, None, GM_LDS, "hipk_gm_solve_lds_kernel<double,true>"),
    ("gmres-lds-row13-f64", "gmres", "n13_c1r", F64, GM, {}, None, GM_LDS, "hipk_gm_solve_lds_kernel<double,true>"),
    ("gmres-lds-row32-f32", "gmres", "n32_c1r", F32, GM32, {}, None, GM_LDS, "hipk_gm_solve_lds_kernel<float,true>"),
    ("gmres-small-row33-f64", "gmres", "n33_c1r", F64, GM, {}, None, LS, GSW),
    ("gmres-lds-restart1-f64", "gmres", "n5_c1r", F64, GMR(1, maxiter=5), {}, None, GM_LDS, "hipk_gm_solve_lds_kernel<double,true>"),
    ("gmres-lds-restart8-f64", "gmres", "n5_c1r", F64, GMR(8, maxiter=3), {}, None, GM_LDS, "hipk_gm_solve_lds_kernel<double,true>"),
    ("gmres-lds-restart9-incremental-f64", "gmres", "n5_c1r", F64, GMR(9, maxiter=3, **INC), {}, None, GM_LDS, "hipk_gm_solve_lds_kernel<double,true>"),
    ("gmres-lds-restart31-f64", "gmres", "n5_c1r", F64, GMR(31), {}, "rand", GM_LDS, "hipk_gm_solve_lds_kernel<double,true>"),
    ("gmres-lds-restart31-incremental-f32", "gmres", "n5_g1r", F32, GMR(31, tol=1e-5, **INC), {}, None, GM_LDS, "hipk_gm_solve_lds_kernel<float,true>"),
    ("gmres-lds-restart1-incremental-f32", "gmres", "n5_c1r", F32, GMR(1, maxiter=5, tol=1e-5, **INC), {}, None, GM_LDS, "hipk_gm_solve_lds_kernel<float,true>"),
    ("gmres-lds-stop0-f64", "gmres", "n5_c1r", F64, GM, {}, "exact", LS, GSW),                          # no cycle ran
    ("gmres-lds-maxiter0-f64", "gmres", "n5_c1r", F64, dict(tol=1e-8, restart=20, maxiter=0), {}, None, LS, GSW),   # no cycle ran
    ("gmres-lds-maxiter1-f64", "gmres", "n5_c1r", F64, GMR(5, maxiter=1), {}, None, GM_LDS, "hipk_gm_solve_lds_kernel<double,true>"),
    ("gmres-lds-cycles2-maxiter2-f64", "gmres", "n5_c1r", F64, GMR(3, maxiter=2), GCYC2, None, GM_LDS, "hipk_gm_solve_lds_kernel<double,true>"),
    ("gmres-lds-cycles2-maxiter3-f64", "gmres", "n5_c1r", F64, GMR(3, maxiter=3), GCYC2, None, GM_LDS, "hipk_gm_solve_lds_kernel<double,true>"),
    ("gmres-lds-inside-cycle-f64", "gmres", "n5_c1r", F64, GMR(30, maxiter=4, tol=1e-3), {}, None, GM_LDS, "hipk_gm_solve_lds_kernel<double,true>"),
    ("gmres-lds-agent-f64", "gmres", "n5_g1r", F64, GM, {"HIPK_GM_CYCLE_AGENT": "1"}, None, GM_LDS, "hipk_gm_solve_lds_kernel<double,false>"),
    ("gmres-lds-agent-f32", "gmres", "n5_c1r", F32, GM32, {"HIPK_GM_CYCLE_AGENT": "1"}, None, GM_LDS, "hipk_gm_solve_lds_kernel<float,false>"),
    ("gmres-lds-happy-eye5-f64", "gmres", "eye5", F64, GM, {}, None, GM_LDS, "hipk_gm_solve_lds_kernel<double,true>"),
    ("pgmres-lds-n35-f64", "pgmres", "n5_n35", F64, GM, {}, None, GM_LDS, "hipk_gm_solve_lds_kernel<double,true>"),
    ("pgmres-lds-c1-f32", "pgmres", "n5_c1", F32, GM32, {}, None, GM_LDS, "hipk_gm_solve_lds_kernel<float,true>"),
    ("pgmres-lds-c1r-f64", "pgmres", "n5_c1r", F64, GM, {}, "rand", GM_LDS, "hipk_gm_solve_lds_kernel<double,true>"),
    ("pgmres-lds-g1-f64", "pgmres", "n5_g1", F64, GM, {}, None, GM_LDS, "hipk_gm_solve_lds_kernel<double,true>"),
    ("pgmres-lds-g1r-f32", "pgmres", "n5_g1r", F32, GM32, {}, None, GM_LDS, "hipk_gm_solve_lds_kernel<float,true>"),
    ("pgmres-lds-row12-incremental-f64", "pgmres", "n12_c1r", F64, {**GM, **INC}, {}, None, GM_LDS, "hipk_gm_solve_lds_kernel<double,true>"),
    ("pgmres-lds-restart31-f64", "pgmres", "n5_c1r", F64, GMR(31), {}, None, GM_LDS, "hipk_gm_solve_lds_kernel<double,true>"),
    ("pgmres-lds-cycles2-maxiter3-f64", "pgmres", "n5_c1r", F64, GMR(3, maxiter=3), GCYC2, None, GM_LDS, "hipk_gm_solve_lds_kernel<double,true>"),
    ("pgmres-lds-agent-f64", "pgmres", "n5_c1r", F64, GM, {"HIPK_GM_CYCLE_AGENT": "1"}, None, GM_LDS, "hipk_gm_solve_lds_kernel<double,false>"),
    # ---- a launch of an LDS kernel reports its workgroups as not co-resident: the launch sequence takes over, at iteration 0 (nothing
    # was modified) and at iteration 7 / after two cycles (PCG rebuilds <r,z>'s chunk partials, BiCGStab its <r,r>, <rhat,r> ones)
    ("cg-lds-not-resident1-f64", "cg", "s5_c1r", F64, KW, NR1, None, CG_LDS + " -> " + LS, CG3S),
    ("cg-lds-not-resident2-f32", "cg", "s5_g1r", F32, KW32, {**CITS7, **NR2}, None, CG_LDS + " -> " + LS, CG3S),
    ("pcg-lds-not-resident1-f32", "pcg", "s5_c1r", F32, KW32, NR1, "rand", CG_LDS + " -> " + LS, PCG3),
    ("pcg-lds-not-resident2-f64", "pcg", "s5_g1r", F64, KW, {**CITS7, **NR2}, None, CG_LDS + " -> " + LS, PCG3),
    ("bicgstab-lds-not-resident1-f64", "bicgstab", "n5_c1r", F64, KW, NR1, None, BI_LDS + " -> " + LS, BI5S),
    ("bicgstab-lds-not-resident2-f64", "bicgstab", "n5_g1r", F64, KW, {**BITS7, **NR2}, None, BI_LDS + " -> " + LS, BI5S),
    ("pbicgstab-lds-not-resident2-f32", "pbicgstab", "n5_c1r", F32, KW32, {**BITS7, **NR2}, None, BI_LDS + " -> " + LS, BI5SJ),
    ("gmres-lds-not-resident1-f64", "gmres", "n5_c1r", F64, GMR(5, maxiter=4), NR1, None, GM_LDS + " -> " + LS, GSW),
    ("pgmres-lds-not-resident2-f64", "pgmres", "n5_g1r", F64, GMR(3, maxiter=5), {**GCYC2, **NR2}, None, GM_LDS + " -> " + LS, GSW),
    # ================================================================== the same kernels spread over the chip (9 .. 32 chunks)
    ("gmres-spread-c9-f64", "gmres", "n5_c9", F64, GM, {}, None, GM_LDS, "hipk_gm_solve_lds_kernel<double,false>"),
    ("gmres-spread-c9-f32", "gmres", "n5_c9", F32, GM32, {}, "rand", GM_LDS, "hipk_gm_solve_lds_kernel<float,false>"),
    ("gmres-spread-c32-f64", "gmres", "n5_c32", F64, GM, {}, None, GM_LDS, "hipk_gm_solve_lds_kernel<double,false>"),
    ("gmres-spread-c32-incremental-f32", "gmres", "n5_c32", F32, {**GM32, **INC}, {}, None, GM_LDS, "hipk_gm_solve_lds_kernel<float,false>"),
    ("pgmres-spread-c9-f64", "pgmres", "n5_c9", F64, GM, {}, None, GM_LDS, "hipk_gm_solve_lds_kernel<double,false>"),
    ("pgmres-spread-c32-f32", "pgmres", "n5_c32", F32, GM32, {}, None, GM_LDS, "hipk_gm_solve_lds_kernel<float,false>"),
    ("gmres-spread-c33-f64", "gmres", "n5_c33", F64, GM, {}, None, "hipk_gm_mid_kernel<double,5,false>", "hipk_gm_mid_kernel<double,5,false>"),
    ("gmres-nospread-c9-f64", "gmres", "n5_c9", F64, GM, NOSPREAD, None, LS, GLS),
    ("cg-spread-mid0-c9-f64", "cg", "s5_c9", F64, KW, MID0, None, CG_LDS, "hipk_cg_solve_lds_kernel<double,false,false>"),
    ("cg-spread-mid0-c32-f32", "cg", "s5_c32", F32, KW32, MID0, "rand", CG_LDS, "hipk_cg_solve_lds_kernel<float,false,false>"),
    ("cg-spread-far-c32-f64", "cg", "sfar_c32", F64, KW, {}, None, CG_LDS, "hipk_cg_solve_lds_kernel<double,false,false>"),
    ("cg-spread-far-c32-f32", "cg", "sfar_c32", F32, KW32, {}, None, CG_LDS, "hipk_cg_solve_lds_kernel<float,false,false>"),
    ("cg-nospread-mid0-c9-f64", "cg", "s5_c9", F64, KW, {**MID0, **NOSPREAD}, None, LS, CG3),
    ("cg-nospread-far-c32-f64", "cg", "sfar_c32", F64, KW, NOSPREAD, None, LS, CG3),
    ("pcg-spread-mid0-c9-f32", "pcg", "s5_c9", F32, KW32, MID0, None, CG_LDS, "hipk_cg_solve_lds_kernel<float,false,true>"),
    ("pcg-spread-mid0-c32-f64", "pcg", "s5_c32", F64, KW, MID0, None, CG_LDS, "hipk_cg_solve_lds_kernel<double,false,true>"),
    ("pcg-spread-far-c32-f64", "pcg", "sfar_c32", F64, KW, {}, "rand", CG_LDS, "hipk_cg_solve_lds_kernel<double,false,true>"),
    ("pcg-seq-mid0-c33-f64", "pcg", "s5_c33", F64, KW, MID0, None, LS, PCG3),
    ("pcg-nospread-mid0-c9-f64", "pcg", "s5_c9", F64, KW, {**MID0, **NOSPREAD}, None, LS, PCG3),
    ("bicgstab-spread-mid0-c9-f64", "bicgstab", "n5_c9", F64, KW, BMID0, None, BI_LDS, "hipk_bi_solve_lds_kernel<double,false,false>"),
    ("bicgstab-spread-mid0-c32-f32", "bicgstab", "n5_c32", F32, KW32, BMID0, "rand", BI_LDS, "hipk_bi_solve_lds_kernel<float,false,false>"),
    ("bicgstab-spread-far-c32-f64", "bicgstab", "nfar_c32", F64, KW, {}, None, BI_LDS, "hipk_bi_solve_lds_kernel<double,false,false>"),
    ("bicgstab-spread-far-c32-f32", "bicgstab", "nfar_c32", F32, KW32, {}, None, BI_LDS, "hipk_bi_solve_lds_kernel<float,false,false>"),
    ("bicgstab-seq-mid0-c33-f64", "bicgstab", "n5_c33", F64, KW, BMID0, None, LS, BI5),
    ("bicgstab-nospread-mid0-c9-f64", "bicgstab", "n5_c9", F64, KW, {**BMID0, **NOSPREAD}, None, LS, BI5),
    ("pbicgstab-spread-mid0-c9-f32", "pbicgstab", "n5_c9", F32, KW32, BMID0, None, BI_LDS, "hipk_bi_solve_lds_kernel<float,false,true>"),
    ("pbicgstab-spread-mid0-c32-f64", "pbicgstab", "n5_c32", F64, KW, BMID0, None, BI_LDS, "hipk_bi_solve_lds_kernel<double,false,true>"),
    ("pbicgstab-spread-far-c32-f64", "pbicgstab", "nfar_c32", F64, KW, {}, None, BI_LDS, "hipk_bi_solve_lds_kernel<double,false,true>"),
    ("pbicgstab-seq-mid0-c33-f64", "pbicgstab", "n5_c33", F64, KW, BMID0, None, LS, BI5J),
    # ================================================================== the small launch sequences (<= 8 chunks) and their far side
    ("cg-small-row32-f64", "cg", "s32_c1r", F64, KW, {}, None, LS, CG3S),
    ("cg-small-dense300-f64", "cg", "dense300s", F64, KW, {}, None, LS, CG3S),
    ("cg-small-dense300-f32", "cg", "dense300s", F32, KW32, {}, "rand", LS, CG3S),
    ("cg-small-no-lds-loop-f64", "cg", "s5_g1r", F64, KW, {"HIPK_CG_NO_LDS_LOOP": "1"}, None, LS, CG3S),
    ("cg-small-no-lds-loop-f32", "cg", "s5_c1r", F32, KW32, {"HIPK_CG_NO_LDS_LOOP": "1"}, None, LS, CG3S),
    ("cg-general-no-small-f64", "cg", "s5_c1r", F64, KW, {"HIPK_CG_NO_SMALL": "1"}, None, LS, CG3),
    ("cg-general-no-small-f32", "cg", "s5_g1r", F32, KW32, {"HIPK_CG_NO_SMALL": "1"}, None, LS, CG3),
    ("cg-small-row13-c8-f64", "cg", "s13_c8", F64, KW, {}, None, LS, CG3S),
    ("cg-general-row13-c9-f64", "cg", "s13_c9", F64, KW, {}, None, LS, CG3),
    ("bicgstab-small-row32-f64", "bicgstab", "n32_c1r", F64, KW, {}, None, LS, BI5S),
    ("bicgstab-small-dense300-f64", "bicgstab", "dense300n", F64, KW, {}, None, LS, BI5S),
    ("bicgstab-small-dense300-f32", "bicgstab", "dense300n", F32, KW32, {}, None, LS, BI5S),
    ("bicgstab-small-no-lds-loop-f64", "bicgstab", "n5_g1r", F64, KW, {"HIPK_BICGSTAB_NO_LDS_LOOP": "1"}, None, LS, BI5S),
    ("pbicgstab-small-no-lds-loop-f32", "pbicgstab", "n5_c1r", F32, KW32, {"HIPK_BICGSTAB_NO_LDS_LOOP": "1"}, None, LS, BI5SJ),
    ("bicgstab-general-no-small-f64", "bicgstab", "n5_c1r", F64, KW, {"HIPK_BICGSTAB_NO_SMALL": "1"}, None, LS, BI5),
    ("pbicgstab-general-no-small-f64", "pbicgstab", "n5_g1r", F64, KW, {"HIPK_BICGSTAB_NO_SMALL": "1"}, "rand", LS, BI5J),
    ("bicgstab-small-row13-c8-f64", "bicgstab", "n13_c8", F64, KW, {}, None, LS, BI5S),
    ("bicgstab-general-row13-c9-f64", "bicgstab", "n13_c9", F64, KW, {}, None, LS, BI5),
    ("pbicgstab-general-row13-c9-f32", "pbicgstab", "n13_c9", F32, KW32, {}, None, LS, BI5J),
    ("pbicgstab-callback-small-f64", "pbicgstab", "n5_c1r", F64, {**KW, "callback": True}, {}, None, LS, BI5S + CB),
    ("pbicgstab-callback-general-f64", "pbicgstab", "n5_c9", F64, {**KW, "callback": True}, {}, None, LS, BI5 + CB),
    ("gmres-cycle-small-f64", "gmres", "n5_g1r", F64, GM, {"HIPK_GMRES_NO_LDS_CYCLE": "1"}, None, GM_SMALL, "hipk_gm_cycle_small_kernel<double>"),
    ("gmres-cycle-small-f32", "gmres", "n5_c1r", F32, GM32, {"HIPK_GMRES_NO_LDS_CYCLE": "1"}, "rand", GM_SMALL, "hipk_gm_cycle_small_kernel<float>"),
    ("pgmres-cycle-small-incremental-f64", "pgmres", "n12_c1r", F64, {**GM, **INC}, {"HIPK_GMRES_NO_LDS_CYCLE": "1"}, None, GM_SMALL, "hipk_gm_cycle_small_kernel<double>"),
    ("gmres-small-wide-f64", "gmres", "n5_g1r", F64, GM, {"HIPK_GMRES_NO_CYCLE": "1"}, None, LS, GSW),
    ("gmres-small-wide-f32", "gmres", "n5_c1r", F32, GM32, {"HIPK_GMRES_NO_CYCLE": "1"}, None, LS, GSW),
    ("gmres-small-256-f64", "gmres", "n5_c1r", F64, GM, {"HIPK_GMRES_NO_WIDE": "1"}, None, LS, GS256),
    ("pgmres-small-256-f32", "pgmres", "n5_g1r", F32, GM32, {"HIPK_GMRES_NO_WIDE": "1"}, None, LS, GS256),
    ("gmres-small-dense300-f64", "gmres", "dense300n", F64, GM, {}, None, LS, GSW),
    ("gmres-small-dense300-incremental-f32", "gmres", "dense300n", F32, {**GM32, **INC}, {}, None, LS, GSW),
    ("gmres-large-no-small-f64", "gmres", "n5_c1r", F64, GM, {"HIPK_GMRES_NO_SMALL": "1"}, None, LS, GLS),
    ("gmres-large-first-f64", "gmres", "n5_c9", F64, GM, {**NOSPREAD, "HIPK_GMRES_NO_STREAM": "1"}, None, LS, GLF),
    ("pgmres-large-first-f32", "pgmres", "n5_c1r", F32, GM32, {"HIPK_GMRES_NO_SMALL": "1", "HIPK_GMRES_NO_STREAM": "1"}, None, LS, GLF),
    ("gmres-large-first-split-f64", "gmres", "n5_c1r", F64, GM, {"HIPK_GMRES_NO_SMALL": "1", "HIPK_GMRES_NO_STREAM": "1", "HIPK_GM_SPLIT_NORM": "1"}, None, LS, GLF + SPLIT),
    ("gmres-large-streaming-split-f64", "gmres", "n5_c9", F64, GM, {**NOSPREAD, "HIPK_GM_SPLIT_NORM": "1"}, None, LS, GLS + SPLIT),
    ("gmres-large-streaming-split-f32", "gmres", "n5_c1r", F32, GM32, {"HIPK_GMRES_NO_SMALL": "1", "HIPK_GM_SPLIT_NORM": "1"}, None, LS, GLS + SPLIT),
    # callback M: ||M(.)||^2 is a chunked dot where the Jacobi form fuses a tiled one, so GMRES agrees with the oracle in its counts
    # and to 1e-9 in x (the comparison of test_gpu_pcg.py's callable-M test), not bit for bit; path and form are exact
    ("pgmres-callback-small-wide-f64", "pgmres", "n5_c1r", F64, {**GM, "callback": True}, {}, None, LS, GSW + CB),
    ("pgmres-callback-small-256-f64", "pgmres", "n5_c1r", F64, {**GM, "callback": True}, {"HIPK_GMRES_NO_WIDE": "1"}, None, LS, GS256 + CB),
    ("pgmres-callback-large-first-f64", "pgmres", "n5_c9", F64, {**GM, "callback": True}, {"HIPK_GMRES_NO_STREAM": "1"}, None, LS, GLF + CB),
    ("pgmres-callback-large-first-split-f64", "pgmres", "n5_c1r", F64, {**GM, "callback": True},
     {"HIPK_GMRES_NO_SMALL": "1", "HIPK_GMRES_NO_STREAM": "1", "HIPK_GM_SPLIT_NORM": "1"}, None, LS, GLF + SPLIT + CB),
    ("pgmres-callback-large-streaming-f64", "pgmres", "n5_c9", F64, {**GM, "callback": True}, {}, None, LS, GLS + CB),
    ("pgmres-callback-large-streaming-split-f64", "pgmres", "n5_c1r", F64, {**GM, "callback": True},
     {"HIPK_GMRES_NO_SMALL": "1", "HIPK_GM_SPLIT_NORM": "1"}, None, LS, GLS + SPLIT + CB),
    ("pgmres-callback-restart32-f64", "pgmres", "n5_c1r", F64, {**GMR(32), "callback": True}, {}, None, LS, GBIG + CB),
    ("pgmres-callback-restart32-split-f64", "pgmres", "n5_c1r", F64, {**GMR(32), "callback": True}, {"HIPK_GM_SPLIT_NORM": "1"}, None, LS, GBIG + SPLIT + CB),
    # ================================================================== two-launch CG: one case on each side of every guard of hipk_cg_path_two
    ("cg2-c33-mid0-f64", "cg", "s5_c33", F64, KW, MID0, None, LS, CG2_64),                       # g > 32; a tile AT the fp64 capacity
    ("cg2-c33-mid0-f32", "cg", "s5_c33", F32, KW32, MID0, None, LS, CG2_32),
    ("cg2-c32-mid0-nospread-f64", "cg", "s5_c32", F64, KW, {**MID0, **NOSPREAD}, None, LS, CG3),
    ("cg2-c150-mid0-f64", "cg", "s5_c150", F64, dict(tol=1e-8, maxiter=200), MID0, None, LS, CG2_64),   # g <= kCg2MaxChunks
    ("cg2-c150-mid0-f32", "cg", "s5_c150", F32, KW32, MID0, "rand", LS, CG2_32),
    ("cg2-c151-mid0-f64", "cg", "s5_c151", F64, dict(tol=1e-8, maxiter=200), MID0, None, LS, CG3),
    ("cg2-tile1281-mid0-f64", "cg", "s5x_c33", F64, KW, MID0, None, LS, CG3),                    # max_tile_nnz <= 1280 (fp64)
    ("cg2-tile1281-mid0-f32", "cg", "s5x_c33", F32, KW32, MID0, None, LS, CG2_32),
    ("cg2-tile2048-mid0-f32", "cg", "s8_c33", F32, KW32, MID0, None, LS, CG2_32),                # ... <= 2048 (fp32)
    ("cg2-tile2048-mid0-f64", "cg", "s8_c33", F64, KW, MID0, None, LS, CG3),
    ("cg2-tile2049-mid0-f32", "cg", "s8x_c33", F32, KW32, MID0, None, LS, CG3),
    ("cg2-row32-f64", "cg", "star32_c33", F64, KW, {}, None, LS, CG2_64),                        # max_row_len <= HIPK_LONG_ROW (the mid loop: <= 12)
    ("cg2-row32-f32", "cg", "star32_c33", F32, KW32, {}, None, LS, CG2_32),
    ("cg2-row33-f64", "cg", "star33_c33", F64, KW, {}, None, LS, CG3),
    ("cg2-switch-off-mid0-f64", "cg", "s5_c33", F64, KW, {**MID0, "HIPK_CG_TWO_LAUNCH": "0"}, None, LS, CG3),
    ("cg2-reach-out-f64", "cg", "reach_out", F64, KW, {}, None, LS, CG2_64),                     # default environment: the mid loop refuses the reach
    ("cg2-reach-out-f32", "cg", "reach_out", F32, KW32, {}, None, LS, CG2_32),
    ("cg2-reach-out-warm-f64", "cg", "reach_out", F64, KW, {}, "rand", LS, CG2_64),
    ("cg2-reach-out-maxiter38-f64", "cg", "reach_out", F64, KW12(38), {}, None, LS, CG2_64),
    ("cg2-reach-out-maxiter37-f64", "cg", "reach_out", F64, KW12(37), {}, "rand", LS, CG2_64),
    ("cg2-reach-out-maxiter1-f32", "cg", "reach_out", F32, KW12(1), {}, None, LS, CG2_32),
    ("cg2-reach-out-stop0-f64", "cg", "reach_out", F64, dict(tol=0.5, maxiter=400), {}, "exact", LS, CG2_64),
    ("cg2-after-mid-hand-back-it0-f64", "cg", "s5_c46", F64, KW, NR1, None, "hipk_cg_mid_kernel<double,5,1,false> -> " + LS, CG2_64),
    # it == 0 fails after the mid loop ran 7 iterations: p_7 is not where the two-launch iteration's first pass reads it
    ("cg2-after-mid-hand-back-it7-f64", "cg", "s5_c46", F64, KW, {**CITS7, "HIPK_TEST_LDS_NOT_RESIDENT": "2"}, None,
     "hipk_cg_mid_kernel<double,5,1,false> -> " + LS, CG3),
    # ================================================================== GMRES above restart 31 (H, R, Givens pairs in the workspace)
    ("gmres-big-r32-n35-f64", "gmres", "n5_n35", F64, GMR(32), {}, None, LS, GBIG),              # restart > n - 3
    ("gmres-big-r33-n35-incremental-f32", "gmres", "n5_n35", F32, GMR(33, tol=1e-5, **INC), {}, None, LS, GBIG),
    ("gmres-big-r64-n35-f64", "gmres", "n5_n35", F64, GMR(64), {}, "rand", LS, GBIG),             # restart > n
    ("gmres-big-r255-n35-incremental-f64", "gmres", "n5_n35", F64, GMR(255, **INC), {}, None, LS, GBIG),
    ("gmres-big-r32-c1r-f64", "gmres", "n5_c1r", F64, GMR(32, maxiter=3), {}, None, LS, GBIG),
    ("gmres-big-r33-c1r-incremental-f64", "gmres", "n5_c1r", F64, GMR(33, maxiter=3, **INC), {}, "rand", LS, GBIG),
    ("gmres-big-r64-c1r-f32", "gmres", "n5_c1r", F32, GMR(64, tol=1e-5), {}, None, LS, GBIG),
    ("gmres-big-r127-c1r-incremental-f64", "gmres", "n12_c1r", F64, GMR(127, **INC), {}, None, LS, GBIG),
    ("gmres-big-r128-c1r-f64", "gmres", "n12_c1r", F64, GMR(128), {}, None, LS, GBIG),
    ("gmres-big-r128-c1r-incremental-f32", "gmres", "n5_c1r", F32, GMR(128, tol=1e-5, **INC), {}, None, LS, GBIG),
    ("gmres-big-r255-c1r-f64", "gmres", "n5_c1r", F64, GMR(255), {}, None, LS, GBIG),
    ("gmres-big-r255-c1r-f32", "gmres", "n5_c1r", F32, GMR(255, tol=1e-5), {}, "rand", LS, GBIG),
    ("gmres-big-r32-c9-f64", "gmres", "n5_c9", F64, GMR(32, maxiter=3), {}, None, LS, GBIG),
    ("gmres-big-r128-c9-incremental-f64", "gmres", "n5_c9", F64, GMR(128, **INC), {}, None, LS, GBIG),
    ("gmres-big-r64-c9-f32", "gmres", "n5_c9", F32, GMR(64, tol=1e-5), {}, None, LS, GBIG),
    ("gmres-big-r255-c9-incremental-f32", "gmres", "n5_c9", F32, GMR(255, tol=1e-5, **INC), {}, None, LS, GBIG),
    ("gmres-big-r32-split-f64", "gmres", "n5_c1r", F64, GMR(32), {"HIPK_GM_SPLIT_NORM": "1"}, None, LS, GBIG + SPLIT),
    ("pgmres-big-r32-c1r-f64", "pgmres", "n5_c1r", F64, GMR(32, maxiter=3), {}, None, LS, GBIG),
    ("pgmres-big-r64-n35-incremental-f64", "pgmres", "n5_n35", F64, GMR(64, **INC), {}, None, LS, GBIG),
    ("pgmres-big-r128-c1r-f32", "pgmres", "n5_c1r", F32, GMR(128, tol=1e-5), {}, None, LS, GBIG),
    ("pgmres-big-r255-c9-incremental-f64", "pgmres", "n5_c9", F64, GMR(255, **INC), {}, "rand", LS, GBIG),
    ("pgmres-big-r255-c1r-split-f32", "pgmres", "n12_c1r", F32, GMR(255, tol=1e-5), {"HIPK_GM_SPLIT_NORM": "1"}, None, LS, GBIG + SPLIT),
]

# forms of the table no case above (or of the mid table) reaches, each with its reason
UNREACHABLE = {
    "cg three-launch, streams": "needs x, r, p, Ap beyond 384 MiB; run at full size by test_cg_multi_step_chunks_both_cache_policies",
    "cg three-launch, streams + flat direction": "needs a vector beyond 256 MiB; run at full size by test_cg_multi_step_chunks_both_cache_policies",
}


def matrix_props(M):
    """(chunks, longest row, most entries in a 256-row tile, most window tiles of a 2048-row block, widest tile range of a block),
    in numpy from the CSR arrays alone."""
    n = M.shape[0]
    g = (n + CH - 1) // CH
    lens = np.diff(M.indptr)
    tile = int(np.add.reduceat(lens, np.arange(0, n, TILE)).max())
    rows = np.repeat(np.arange(n), lens)
    key = (rows // CH).astype(np.int64) * (1 << 32) + (M.indices // TILE)
    uniq = np.unique(key)
    blk, ct = uniq >> 32, uniq & 0xFFFFFFFF
    slots = int(np.bincount(blk).max())
    first = np.full(g, np.iinfo(np.int64).max)
    last = np.zeros(g, dtype=np.int64)
    np.minimum.at(first, blk, ct)
    np.maximum.at(last, blk, ct)
    return dict(g=g, W=int(lens.max()), tile=tile, slots=slots, range=int((last - first + 1).max()))
