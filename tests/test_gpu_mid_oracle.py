"""The one-launch loops of mid-size systems (csrc/hipk_cg_mid.h, hipk_bi_mid.h, hipk_gm_mid.h) against the CPU oracle, case by
case: every instantiation the four dispatch sites can select (hipk_cg.hip CG and Jacobi PCG, hipk_bicgstab.hip, hipk_gmres.hip),
both sides of each dispatch boundary, and the edges inside the loops.  Each case asserts

  * which loop finished the solve (hipk_last_solve_path), written literally below from reading the dispatch code;
  * x, iterations, matvecs, info and breakdown bitwise equal to the oracle's;
  * the returned stats against a long-double recomputation from the stored A, b and the returned x, so that the kernels and
    the oracle cannot share a bug unnoticed.

Every solve runs through tests/_solve_runner.py: the workspace in a guarded arena of exactly *_work_bytes, x, b and dinv in arenas
of exactly n elements, once per workspace state (0x00, 0xFF, 0x5A fill, no refill).  The path, the guards and the read-only
operands are asserted after every run (the form too: form_of below); the 0x00 run feeds the assertions above, the others must
equal it bit for bit.  No solve of this table takes 0.5 s on the GPU (the longest 0.008 s): every case runs all four states.

Sizes that depend on the device (its compute-unit count n_cu) are resolved when a case runs; the paths do not depend on it."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from _arena import FILLS
from _oracle_cases import _band, _check_stats_long_double, _ldc, _signed_band
from _solve_runner import build_case, run_solve_case

DEV = "cuda:0"
CH = 2048            # rows per reduction chunk below 4 M rows (hipk_chunk_size)
N46 = 45 * CH + 37   # 46 chunks, the last one ragged


# ---------------------------------------------------------------------------------------------- matrices (scipy, seeded)
def _lap9(nx):
    """2-D 9-point Laplacian (SPD, 9 entries per interior row, reach nx + 1)."""
    T = sp.diags([1.0, 1.0, 1.0], [-1, 0, 1], shape=(nx, nx))
    M = (sp.diags(np.full(nx * nx, 9.0)) - sp.kron(T, T)).tocsr()   # 8 on the diagonal, -1 at the 8 neighbours
    M.sort_indices()
    return M


def _upwind8(nx):
    """Nonsymmetric 8-entry stencil on an nx-wide grid (lexicographic order): the diagonal, the four edge neighbours and
    three corners (no north-east one), upwind-weighted values."""
    return _signed_band(nx * nx, (-nx - 1, -nx, -nx + 1, -1, 0, 1, nx - 1, nx), seed=2)


def _grid3d(m):
    """7-point Laplacian on an m^3 grid (SPD; reach m^2)."""
    T = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(m, m))
    I = sp.identity(m)
    M = (sp.kron(sp.kron(T, I), I) + sp.kron(sp.kron(I, T), I) + sp.kron(sp.kron(I, I), T)).tocsr()
    M.sort_indices()
    return M


def _n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _odd_chunks_above_ncu():
    c = _n_cu() + 1 if (_n_cu() + 1) % 2 else _n_cu() + 2
    return (c - 1) * CH + 1000   # c chunks (odd, > n_cu), the last one ragged


def _grid3d_above_ncu():
    m = 2
    while m ** 3 <= _n_cu() * CH:
        m += 1
    return _grid3d(m)


MATRICES = {
    # rows of exactly W entries, and of the smallest length that selects W (6, 8, 10): padded lanes
    "sym5": lambda: _band(N46, (1, 2)),
    "sym6": lambda: _band(N46, (1, 2), match=300),
    "sym7": lambda: _band(N46, (1, 2, 3)),
    "sym8": lambda: _band(N46, (1, 2, 3), match=300),
    "sym10": lambda: _band(N46, (1, 2, 3, 4), match=300),
    "sym12": lambda: _band(N46, (1, 2, 3, 4, 5), match=300),
    "sym13": lambda: _band(N46, (1, 2, 3, 4, 5, 6)),
    "non5": lambda: _band(N46, (1, 2), sym=False, seed=1),
    "non6": lambda: _band(N46, (1, 2), match=300, sym=False, seed=1),
    "non7": lambda: _band(N46, (1, 2, 3), sym=False, seed=1),
    "non10": lambda: _band(N46, (1, 2, 3, 4), match=300, sym=False, seed=1),
    "non12": lambda: _band(N46, (1, 2, 3, 4, 5), match=300, sym=False, seed=1),
    "non13": lambda: _band(N46, (1, 2, 3, 4, 5, 6), sym=False, seed=1),
    "lap9": lambda: _lap9(300),            # 44 chunks
    "upwind8": lambda: _upwind8(300),
    "ldc": lambda: _ldc(400),              # 79 chunks
    # dispatch boundaries
    "sym5_c8": lambda: _band(8 * CH, (1, 2)),
    "sym5_c9": lambda: _band(8 * CH + 1, (1, 2)),
    "sym5_c16": lambda: _band(16 * CH, (1, 2)),
    "non5_c8": lambda: _band(8 * CH, (1, 2), sym=False, seed=1),
    "non5_c9": lambda: _band(8 * CH + 1, (1, 2), sym=False, seed=1),
    "non5_c32": lambda: _band(32 * CH, (1, 2), sym=False, seed=1),
    "non5_c33": lambda: _band(32 * CH + 1, (1, 2), sym=False, seed=1),
    "non5_c40": lambda: _band(40 * CH, (1, 2), sym=False, seed=1),
    "sym5_ncu": lambda: _band(_n_cu() * CH, (1, 2)),
    "sym5_ncu1": lambda: _band(_n_cu() * CH + 1, (1, 2)),
    "sym6_ncu1": lambda: _band(_n_cu() * CH + 1, (1, 2), match=300),
    "sym7_ncu1": lambda: _band(_n_cu() * CH + 1, (1, 2, 3)),
    "sym8_ncu1": lambda: _band(_n_cu() * CH + 1, (1, 2, 3), match=300),
    "sym5_odd": lambda: _band(_odd_chunks_above_ncu(), (1, 2)),
    "non5_ncu": lambda: _band(_n_cu() * CH, (1, 2), sym=False, seed=1),
    "non5_ncu1": lambda: _band(_n_cu() * CH + 1, (1, 2), sym=False, seed=1),
    "sym5_c512": lambda: _band(512 * CH, (1, 2)),
    "sym5_c513": lambda: _band(512 * CH + 1, (1, 2)),
    "grid3d_ncu1": _grid3d_above_ncu,
    # plan reach (kMidPlanRange = 512 tiles of 256 columns from a block's first to its last): a block of 2048 rows with
    # columns +-d around it spans 8 + 2 d / 256 tiles -- 512 at d = 64512, 514 at d = 64768 (symmetric: even counts only)
    "reach_in": lambda: _band(80 * CH, (1, 64512)),
    "reach_out": lambda: _band(80 * CH, (1, 64768)),
    # window tiles (kMidPlanSlots = 64): own 8 tiles + 2 for +-1 + three pairs of unaligned bands of 9 tiles = 64; four pairs
    # of aligned bands of 8 = 72 (fp32: the LDS of the CG loop holds 77 tiles, so the slot rule decides)
    "slots64": lambda: _band(50 * CH, (1, 4196, 12388, 20580)),
    "slots72": lambda: _band(80 * CH, (4096, 12288, 20480, 28672)),
    # nonsymmetric (GMRES, fp32: 85 tiles of LDS): own 8 + seven aligned one-sided bands of 8 = 64; one unaligned = 65
    "gslots64": lambda: _signed_band(40 * CH, (-20480, -12288, -4096, 0, 4096, 12288, 20480, 28672)),
    "gslots65": lambda: _signed_band(40 * CH, (-20480, -12288, -4096, 0, 4096, 12288, 20480, 28772)),
}

F64, F32 = "f64", "f32"
LS = "launch sequence"
CG_LDS, BI_LDS, GM_LDS = "hipk_cg_solve_lds_kernel", "hipk_bi_solve_lds_kernel", "hipk_gm_solve_lds_kernel"
NR1 = {"HIPK_TEST_LDS_NOT_RESIDENT": "1"}

# (id, matrix, dtype, solve options, environment, x0: None | "rand" | "exact" (b = A x0), expected hipk_last_solve_path)
# solve options: tol / maxiter (CG, BiCGStab: iterations; GMRES: restart cycles), restart, solve_method
CG_KW = dict(tol=1e-8, maxiter=400)
CG32_KW = dict(tol=1e-4, maxiter=200)
GM_KW = dict(tol=1e-8, restart=20, maxiter=3)
GM32_KW = dict(tol=1e-4, restart=20, maxiter=3)
CASES = [
    # ---- CG, one chunk per workgroup: W in {5, 7, 9, 12}
    ("cg-w5-sym5-f64", "sym5", F64, CG_KW, {}, None, "hipk_cg_mid_kernel<double,5,1,false>"),
    ("cg-w5-sym5-f32", "sym5", F32, CG32_KW, {}, None, "hipk_cg_mid_kernel<float,5,1,false>"),
    ("cg-w5-ldc-f64", "ldc", F64, dict(tol=1e-8, maxiter=300), {}, "consistent", "hipk_cg_mid_kernel<double,5,1,false>"),
    ("cg-w5-ldc-f32", "ldc", F32, dict(tol=1e-4, maxiter=200), {}, "consistent", "hipk_cg_mid_kernel<float,5,1,false>"),
    ("cg-w7-sym7-f64", "sym7", F64, CG_KW, {}, None, "hipk_cg_mid_kernel<double,7,1,false>"),
    ("cg-w7-sym6-f64", "sym6", F64, CG_KW, {}, None, "hipk_cg_mid_kernel<double,7,1,false>"),
    ("cg-w7-sym7-f32", "sym7", F32, CG32_KW, {}, None, "hipk_cg_mid_kernel<float,7,1,false>"),
    ("cg-w7-sym6-f32", "sym6", F32, CG32_KW, {}, None, "hipk_cg_mid_kernel<float,7,1,false>"),
    ("cg-w9-lap9-f64", "lap9", F64, CG_KW, {}, None, "hipk_cg_mid_kernel<double,9,1,false>"),
    ("cg-w9-sym8-f64", "sym8", F64, CG_KW, {}, None, "hipk_cg_mid_kernel<double,9,1,false>"),
    ("cg-w9-lap9-f32", "lap9", F32, CG32_KW, {}, None, "hipk_cg_mid_kernel<float,9,1,false>"),
    ("cg-w9-sym8-f32", "sym8", F32, CG32_KW, {}, None, "hipk_cg_mid_kernel<float,9,1,false>"),
    ("cg-w12-sym12-f64", "sym12", F64, CG_KW, {}, None, "hipk_cg_mid_kernel<double,12,1,false>"),
    ("cg-w12-sym10-f64", "sym10", F64, CG_KW, {}, None, "hipk_cg_mid_kernel<double,12,1,false>"),
    ("cg-w12-sym12-f32", "sym12", F32, CG32_KW, {}, None, "hipk_cg_mid_kernel<float,12,1,false>"),
    ("cg-w12-sym10-f32", "sym10", F32, CG32_KW, {}, None, "hipk_cg_mid_kernel<float,12,1,false>"),
    # ---- CG, two chunks per workgroup (> n_cu chunks): W in {5, 7}
    ("cg-nch2-w5-f64", "sym5_ncu1", F64, CG_KW, {}, None, "hipk_cg_mid_kernel<double,5,2,false>"),
    ("cg-nch2-w5-f32", "sym5_ncu1", F32, CG32_KW, {}, None, "hipk_cg_mid_kernel<float,5,2,false>"),
    ("cg-nch2-w7-sym7-f64", "sym7_ncu1", F64, CG_KW, {}, None, "hipk_cg_mid_kernel<double,7,2,false>"),
    ("cg-nch2-w7-sym6-f64", "sym6_ncu1", F64, CG_KW, {}, None, "hipk_cg_mid_kernel<double,7,2,false>"),
    ("cg-nch2-w7-sym7-f32", "sym7_ncu1", F32, CG32_KW, {}, None, "hipk_cg_mid_kernel<float,7,2,false>"),
    ("cg-nch2-w7-sym6-f32", "sym6_ncu1", F32, CG32_KW, {}, None, "hipk_cg_mid_kernel<float,7,2,false>"),
    ("cg-nch2-w7-grid3d-f32", "grid3d_ncu1", F32, CG32_KW, {}, None, "hipk_cg_mid_kernel<float,7,2,false>"),
    # the 3-D window at two chunks (own rows +- a grid line and the two planes: 52 tiles) exceeds the LDS of the fp64 loop
    ("cg-nch2-w7-grid3d-f64", "grid3d_ncu1", F64, CG_KW, {}, None, LS),
    # four rows per thread hold at most 7 entries each in registers: no <T, 9, 2> / <T, 12, 2>
    ("cg-nch2-w9-sym8-f64", "sym8_ncu1", F64, CG_KW, {}, None, LS),
    # ---- CG dispatch boundaries
    ("cg-chunks8-f64", "sym5_c8", F64, CG_KW, {}, None, CG_LDS),
    ("cg-chunks9-f64", "sym5_c9", F64, CG_KW, {}, None, "hipk_cg_mid_kernel<double,5,1,false>"),
    ("cg-chunks-ncu-f64", "sym5_ncu", F64, CG_KW, {}, None, "hipk_cg_mid_kernel<double,5,1,false>"),
    ("cg-chunks-ncu1-f64", "sym5_ncu1", F64, CG_KW, {}, "rand", "hipk_cg_mid_kernel<double,5,2,false>"),
    ("cg-chunks512-f64", "sym5_c512", F64, dict(tol=1e-8, maxiter=60), {}, None, "hipk_cg_mid_kernel<double,5,2,false>"),
    ("cg-chunks513-f64", "sym5_c513", F64, dict(tol=1e-8, maxiter=60), {}, None, LS),
    ("cg-row12-f64", "sym12", F64, CG_KW, {}, "rand", "hipk_cg_mid_kernel<double,12,1,false>"),
    ("cg-row13-f64", "sym13", F64, CG_KW, {}, None, LS),
    ("cg-row13-f32", "sym13", F32, CG32_KW, {}, None, LS),
    ("cg-reach512-f64", "reach_in", F64, CG_KW, {}, None, "hipk_cg_mid_kernel<double,5,1,false>"),
    ("cg-reach514-f64", "reach_out", F64, CG_KW, {}, None, LS),
    ("cg-slots64-f32", "slots64", F32, CG32_KW, {}, None, "hipk_cg_mid_kernel<float,9,1,false>"),
    ("cg-slots72-f32", "slots72", F32, CG32_KW, {}, None, LS),
    # ---- CG edges
    ("cg-nch2-odd-ragged-f64", "sym5_odd", F64, CG_KW, {}, "rand", "hipk_cg_mid_kernel<double,5,2,false>"),
    ("cg-nch2-odd-ragged-f32", "sym5_odd", F32, CG32_KW, {}, None, "hipk_cg_mid_kernel<float,5,2,false>"),
    ("cg-warm-f64", "sym5", F64, CG_KW, {}, "rand", "hipk_cg_mid_kernel<double,5,1,false>"),
    ("cg-warm-f32", "sym7", F32, CG32_KW, {}, "rand", "hipk_cg_mid_kernel<float,7,1,false>"),
    ("cg-maxiter1-f64", "sym5", F64, dict(tol=1e-12, maxiter=1), {}, "rand", "hipk_cg_mid_kernel<double,5,1,false>"),
    ("cg-maxiter7-f64", "sym5", F64, dict(tol=1e-12, maxiter=7), {}, None, "hipk_cg_mid_kernel<double,5,1,false>"),
    ("cg-maxiter0-f64", "sym5", F64, dict(tol=1e-12, maxiter=0), {}, None, LS),   # the one-launch loop needs maxiter > 0
    ("cg-stop0-f64", "sym5", F64, dict(tol=0.5, maxiter=400), {}, "exact", "hipk_cg_mid_kernel<double,5,1,false>"),
    ("cg-launch-its7-f64", "sym5", F64, CG_KW, {"HIPK_CG_LAUNCH_ITS": "7"}, None, "hipk_cg_mid_kernel<double,5,1,false>"),
    ("cg-launch-its7-f32", "sym5", F32, CG32_KW, {"HIPK_CG_LAUNCH_ITS": "7"}, "rand", "hipk_cg_mid_kernel<float,5,1,false>"),
    ("cg-not-resident1-f64", "sym5", F64, CG_KW, NR1, None, "hipk_cg_mid_kernel<double,5,1,false> -> " + LS),
    ("cg-not-resident2-f64", "sym5", F64, CG_KW, {"HIPK_CG_LAUNCH_ITS": "7", "HIPK_TEST_LDS_NOT_RESIDENT": "2"}, None,
     "hipk_cg_mid_kernel<double,5,1,false> -> " + LS),
    # at 16 chunks the whole-loop kernel takes over from a hand-back, and its first launch hands back too
    ("cg-not-resident1-chunks16-f64", "sym5_c16", F64, CG_KW, NR1, None,
     "hipk_cg_mid_kernel<double,5,1,false> -> " + CG_LDS + " -> " + LS),
    # ---- Jacobi PCG (hipk_cg_mid_kernel<T, W, 1, true>, up to min(256, n_cu) chunks)
    ("pcg-w5-sym5-f64", "sym5", F64, CG_KW, {}, None, "hipk_cg_mid_kernel<double,5,1,true>"),
    ("pcg-w5-sym5-f32", "sym5", F32, CG32_KW, {}, None, "hipk_cg_mid_kernel<float,5,1,true>"),
    ("pcg-w5-ldc-f64", "ldc", F64, dict(tol=1e-8, maxiter=300), {}, "consistent", "hipk_cg_mid_kernel<double,5,1,true>"),
    ("pcg-w5-ldc-f32", "ldc", F32, dict(tol=1e-4, maxiter=200), {}, "consistent", "hipk_cg_mid_kernel<float,5,1,true>"),
    ("pcg-w7-sym7-f64", "sym7", F64, CG_KW, {}, None, "hipk_cg_mid_kernel<double,7,1,true>"),
    ("pcg-w7-sym6-f64", "sym6", F64, CG_KW, {}, None, "hipk_cg_mid_kernel<double,7,1,true>"),
    ("pcg-w7-sym7-f32", "sym7", F32, CG32_KW, {}, None, "hipk_cg_mid_kernel<float,7,1,true>"),
    ("pcg-w7-sym6-f32", "sym6", F32, CG32_KW, {}, None, "hipk_cg_mid_kernel<float,7,1,true>"),
    ("pcg-w9-lap9-f64", "lap9", F64, CG_KW, {}, None, "hipk_cg_mid_kernel<double,9,1,true>"),
    ("pcg-w9-sym8-f64", "sym8", F64, CG_KW, {}, None, "hipk_cg_mid_kernel<double,9,1,true>"),
    ("pcg-w9-lap9-f32", "lap9", F32, CG32_KW, {}, None, "hipk_cg_mid_kernel<float,9,1,true>"),
    ("pcg-w9-sym8-f32", "sym8", F32, CG32_KW, {}, None, "hipk_cg_mid_kernel<float,9,1,true>"),
    ("pcg-w12-sym12-f64", "sym12", F64, CG_KW, {}, None, "hipk_cg_mid_kernel<double,12,1,true>"),
    ("pcg-w12-sym10-f64", "sym10", F64, CG_KW, {}, None, "hipk_cg_mid_kernel<double,12,1,true>"),
    ("pcg-w12-sym12-f32", "sym12", F32, CG32_KW, {}, None, "hipk_cg_mid_kernel<float,12,1,true>"),
    ("pcg-w12-sym10-f32", "sym10", F32, CG32_KW, {}, None, "hipk_cg_mid_kernel<float,12,1,true>"),
    ("pcg-chunks8-f64", "sym5_c8", F64, CG_KW, {}, None, CG_LDS),
    ("pcg-chunks9-f64", "sym5_c9", F64, CG_KW, {}, None, "hipk_cg_mid_kernel<double,5,1,true>"),
    ("pcg-chunks-ncu-f64", "sym5_ncu", F64, CG_KW, {}, None, "hipk_cg_mid_kernel<double,5,1,true>"),
    ("pcg-chunks-ncu1-f64", "sym5_ncu1", F64, CG_KW, {}, None, LS),
    ("pcg-row13-f64", "sym13", F64, CG_KW, {}, None, LS),
    ("pcg-warm-f64", "sym7", F64, CG_KW, {}, "rand", "hipk_cg_mid_kernel<double,7,1,true>"),
    ("pcg-maxiter1-f64", "sym5", F64, dict(tol=1e-12, maxiter=1), {}, None, "hipk_cg_mid_kernel<double,5,1,true>"),
    ("pcg-maxiter7-f64", "sym5", F64, dict(tol=1e-12, maxiter=7), {}, "rand", "hipk_cg_mid_kernel<double,5,1,true>"),
    ("pcg-stop0-f64", "sym5", F64, dict(tol=0.5, maxiter=400), {}, "exact", "hipk_cg_mid_kernel<double,5,1,true>"),
    ("pcg-launch-its7-f64", "sym5", F64, CG_KW, {"HIPK_CG_LAUNCH_ITS": "7"}, None, "hipk_cg_mid_kernel<double,5,1,true>"),
    ("pcg-not-resident1-f64", "sym5", F64, CG_KW, NR1, None, "hipk_cg_mid_kernel<double,5,1,true> -> " + LS),
    ("pcg-not-resident2-f64", "sym5", F64, CG_KW, {"HIPK_CG_LAUNCH_ITS": "7", "HIPK_TEST_LDS_NOT_RESIDENT": "2"}, "rand",
     "hipk_cg_mid_kernel<double,5,1,true> -> " + LS),
    # ---- BiCGStab, M = identity and Jacobi: W in {5, 7, 9, 12} x PRE
    ("bicgstab-w5-non5-f64", "non5", F64, CG_KW, {}, None, "hipk_bi_mid_kernel<double,5,false>"),
    ("bicgstab-w5-non5-f32", "non5", F32, CG32_KW, {}, None, "hipk_bi_mid_kernel<float,5,false>"),
    ("bicgstab-w5-ldc-f64", "ldc", F64, dict(tol=1e-8, maxiter=200), {}, "consistent", "hipk_bi_mid_kernel<double,5,false>"),
    ("bicgstab-w7-non7-f64", "non7", F64, CG_KW, {}, None, "hipk_bi_mid_kernel<double,7,false>"),
    ("bicgstab-w7-non6-f64", "non6", F64, CG_KW, {}, None, "hipk_bi_mid_kernel<double,7,false>"),
    ("bicgstab-w7-non7-f32", "non7", F32, CG32_KW, {}, None, "hipk_bi_mid_kernel<float,7,false>"),
    ("bicgstab-w7-non6-f32", "non6", F32, CG32_KW, {}, None, "hipk_bi_mid_kernel<float,7,false>"),
    ("bicgstab-w9-lap9-f64", "lap9", F64, CG_KW, {}, None, "hipk_bi_mid_kernel<double,9,false>"),
    ("bicgstab-w9-upwind8-f64", "upwind8", F64, CG_KW, {}, None, "hipk_bi_mid_kernel<double,9,false>"),
    ("bicgstab-w9-lap9-f32", "lap9", F32, CG32_KW, {}, None, "hipk_bi_mid_kernel<float,9,false>"),
    ("bicgstab-w9-upwind8-f32", "upwind8", F32, CG32_KW, {}, None, "hipk_bi_mid_kernel<float,9,false>"),
    ("bicgstab-w12-non12-f64", "non12", F64, CG_KW, {}, None, "hipk_bi_mid_kernel<double,12,false>"),
    ("bicgstab-w12-non10-f64", "non10", F64, CG_KW, {}, None, "hipk_bi_mid_kernel<double,12,false>"),
    ("bicgstab-w12-non12-f32", "non12", F32, CG32_KW, {}, None, "hipk_bi_mid_kernel<float,12,false>"),
    ("bicgstab-w12-non10-f32", "non10", F32, CG32_KW, {}, None, "hipk_bi_mid_kernel<float,12,false>"),
    ("pbicgstab-w5-non5-f64", "non5", F64, CG_KW, {}, None, "hipk_bi_mid_kernel<double,5,true>"),
    ("pbicgstab-w5-non5-f32", "non5", F32, CG32_KW, {}, None, "hipk_bi_mid_kernel<float,5,true>"),
    ("pbicgstab-w5-ldc-f32", "ldc", F32, dict(tol=1e-4, maxiter=200), {}, "consistent", "hipk_bi_mid_kernel<float,5,true>"),
    ("pbicgstab-w7-non7-f64", "non7", F64, CG_KW, {}, None, "hipk_bi_mid_kernel<double,7,true>"),
    ("pbicgstab-w7-non6-f64", "non6", F64, CG_KW, {}, None, "hipk_bi_mid_kernel<double,7,true>"),
    ("pbicgstab-w7-non7-f32", "non7", F32, CG32_KW, {}, None, "hipk_bi_mid_kernel<float,7,true>"),
    ("pbicgstab-w7-non6-f32", "non6", F32, CG32_KW, {}, None, "hipk_bi_mid_kernel<float,7,true>"),
    ("pbicgstab-w9-lap9-f64", "lap9", F64, CG_KW, {}, None, "hipk_bi_mid_kernel<double,9,true>"),
    ("pbicgstab-w9-upwind8-f64", "upwind8", F64, CG_KW, {}, None, "hipk_bi_mid_kernel<double,9,true>"),
    ("pbicgstab-w9-lap9-f32", "lap9", F32, CG32_KW, {}, None, "hipk_bi_mid_kernel<float,9,true>"),
    ("pbicgstab-w9-upwind8-f32", "upwind8", F32, CG32_KW, {}, None, "hipk_bi_mid_kernel<float,9,true>"),
    ("pbicgstab-w12-non12-f64", "non12", F64, CG_KW, {}, None, "hipk_bi_mid_kernel<double,12,true>"),
    ("pbicgstab-w12-non10-f64", "non10", F64, CG_KW, {}, None, "hipk_bi_mid_kernel<double,12,true>"),
    ("pbicgstab-w12-non12-f32", "non12", F32, CG32_KW, {}, None, "hipk_bi_mid_kernel<float,12,true>"),
    ("pbicgstab-w12-non10-f32", "non10", F32, CG32_KW, {}, None, "hipk_bi_mid_kernel<float,12,true>"),
    # ---- BiCGStab boundaries and edges
    ("bicgstab-chunks8-f64", "non5_c8", F64, CG_KW, {}, None, BI_LDS),
    ("bicgstab-chunks9-f64", "non5_c9", F64, CG_KW, {}, None, "hipk_bi_mid_kernel<double,5,false>"),
    ("pbicgstab-chunks9-f64", "non5_c9", F64, CG_KW, {}, None, "hipk_bi_mid_kernel<double,5,true>"),
    ("bicgstab-chunks-ncu-f64", "non5_ncu", F64, CG_KW, {}, None, "hipk_bi_mid_kernel<double,5,false>"),
    ("bicgstab-chunks-ncu1-f64", "non5_ncu1", F64, CG_KW, {}, None, LS),
    ("bicgstab-row13-f64", "non13", F64, CG_KW, {}, None, LS),
    ("bicgstab-warm-f64", "non5", F64, CG_KW, {}, "rand", "hipk_bi_mid_kernel<double,5,false>"),
    ("bicgstab-warm-f32", "non7", F32, CG32_KW, {}, "rand", "hipk_bi_mid_kernel<float,7,false>"),
    ("bicgstab-maxiter1-f64", "non5", F64, dict(tol=1e-12, maxiter=1), {}, "rand", "hipk_bi_mid_kernel<double,5,false>"),
    ("bicgstab-maxiter6-f64", "non5", F64, dict(tol=1e-12, maxiter=6), {}, None, "hipk_bi_mid_kernel<double,5,false>"),
    ("bicgstab-maxiter0-f64", "non5", F64, dict(tol=1e-12, maxiter=0), {}, None, LS),
    ("bicgstab-stop0-f64", "non5", F64, dict(tol=0.5, maxiter=300), {}, "exact", "hipk_bi_mid_kernel<double,5,false>"),
    ("bicgstab-tol1e-30-f64", "non5", F64, dict(tol=1e-30, maxiter=120), {}, None, "hipk_bi_mid_kernel<double,5,false>"),
    ("bicgstab-tol1e-30-f32", "non5", F32, dict(tol=1e-30, maxiter=120), {}, None, "hipk_bi_mid_kernel<float,5,false>"),
    ("bicgstab-launch-its5-f64", "non5", F64, CG_KW, {"HIPK_BICGSTAB_LAUNCH_ITS": "5"}, None, "hipk_bi_mid_kernel<double,5,false>"),
    ("pbicgstab-launch-its5-f64", "non7", F64, CG_KW, {"HIPK_BICGSTAB_LAUNCH_ITS": "5"}, "rand", "hipk_bi_mid_kernel<double,7,true>"),
    ("bicgstab-not-resident1-f64", "non5", F64, CG_KW, NR1, None, "hipk_bi_mid_kernel<double,5,false> -> " + LS),
    ("bicgstab-not-resident2-f64", "non5", F64, CG_KW, {"HIPK_BICGSTAB_LAUNCH_ITS": "5", "HIPK_TEST_LDS_NOT_RESIDENT": "2"}, None,
     "hipk_bi_mid_kernel<double,5,false> -> " + LS),
    ("pbicgstab-not-resident1-f64", "non5", F64, CG_KW, NR1, "rand", "hipk_bi_mid_kernel<double,5,true> -> " + LS),
    # ---- GMRES, M = identity and Jacobi: W in {5, 7, 9, 12} x PRE (33 .. min(256, n_cu) chunks, restart <= 31)
    ("gmres-w5-non5-f64", "non5", F64, GM_KW, {}, None, "hipk_gm_mid_kernel<double,5,false>"),
    ("gmres-w5-non5-f32", "non5", F32, GM32_KW, {}, None, "hipk_gm_mid_kernel<float,5,false>"),
    ("gmres-w5-ldc-f64", "ldc", F64, GM_KW, {}, "consistent", "hipk_gm_mid_kernel<double,5,false>"),
    ("gmres-w5-ldc-f32", "ldc", F32, GM32_KW, {}, "consistent", "hipk_gm_mid_kernel<float,5,false>"),
    ("gmres-w7-non7-f64", "non7", F64, GM_KW, {}, None, "hipk_gm_mid_kernel<double,7,false>"),
    ("gmres-w7-non6-f64", "non6", F64, GM_KW, {}, None, "hipk_gm_mid_kernel<double,7,false>"),
    ("gmres-w7-non7-f32", "non7", F32, GM32_KW, {}, None, "hipk_gm_mid_kernel<float,7,false>"),
    ("gmres-w7-non6-f32", "non6", F32, GM32_KW, {}, None, "hipk_gm_mid_kernel<float,7,false>"),
    ("gmres-w9-lap9-f64", "lap9", F64, GM_KW, {}, None, "hipk_gm_mid_kernel<double,9,false>"),
    ("gmres-w9-upwind8-f64", "upwind8", F64, GM_KW, {}, None, "hipk_gm_mid_kernel<double,9,false>"),
    ("gmres-w9-lap9-f32", "lap9", F32, GM32_KW, {}, None, "hipk_gm_mid_kernel<float,9,false>"),
    ("gmres-w9-upwind8-f32", "upwind8", F32, GM32_KW, {}, None, "hipk_gm_mid_kernel<float,9,false>"),
    ("gmres-w12-non12-f64", "non12", F64, GM_KW, {}, None, "hipk_gm_mid_kernel<double,12,false>"),
    ("gmres-w12-non10-f64", "non10", F64, GM_KW, {}, None, "hipk_gm_mid_kernel<double,12,false>"),
    ("gmres-w12-non12-f32", "non12", F32, GM32_KW, {}, None, "hipk_gm_mid_kernel<float,12,false>"),
    ("gmres-w12-non10-f32", "non10", F32, GM32_KW, {}, None, "hipk_gm_mid_kernel<float,12,false>"),
    ("pgmres-w5-non5-f64", "non5", F64, GM_KW, {}, None, "hipk_gm_mid_kernel<double,5,true>"),
    ("pgmres-w5-non5-f32", "non5", F32, GM32_KW, {}, None, "hipk_gm_mid_kernel<float,5,true>"),
    ("pgmres-w5-ldc-f64", "ldc", F64, dict(tol=1e-10, restart=20, maxiter=3), {}, "consistent", "hipk_gm_mid_kernel<double,5,true>"),
    ("pgmres-w7-non7-f64", "non7", F64, GM_KW, {}, None, "hipk_gm_mid_kernel<double,7,true>"),
    ("pgmres-w7-non6-f64", "non6", F64, GM_KW, {}, None, "hipk_gm_mid_kernel<double,7,true>"),
    ("pgmres-w7-non7-f32", "non7", F32, GM32_KW, {}, None, "hipk_gm_mid_kernel<float,7,true>"),
    ("pgmres-w7-non6-f32", "non6", F32, GM32_KW, {}, None, "hipk_gm_mid_kernel<float,7,true>"),
    ("pgmres-w9-lap9-f64", "lap9", F64, GM_KW, {}, None, "hipk_gm_mid_kernel<double,9,true>"),
    ("pgmres-w9-upwind8-f64", "upwind8", F64, GM_KW, {}, None, "hipk_gm_mid_kernel<double,9,true>"),
    ("pgmres-w9-lap9-f32", "lap9", F32, GM32_KW, {}, None, "hipk_gm_mid_kernel<float,9,true>"),
    ("pgmres-w9-upwind8-f32", "upwind8", F32, GM32_KW, {}, None, "hipk_gm_mid_kernel<float,9,true>"),
    ("pgmres-w12-non12-f64", "non12", F64, GM_KW, {}, None, "hipk_gm_mid_kernel<double,12,true>"),
    ("pgmres-w12-non10-f64", "non10", F64, GM_KW, {}, None, "hipk_gm_mid_kernel<double,12,true>"),
    ("pgmres-w12-non12-f32", "non12", F32, GM32_KW, {}, None, "hipk_gm_mid_kernel<float,12,true>"),
    ("pgmres-w12-non10-f32", "non10", F32, GM32_KW, {}, None, "hipk_gm_mid_kernel<float,12,true>"),
    # ---- GMRES boundaries and edges
    ("gmres-chunks32-f64", "non5_c32", F64, GM_KW, {}, None, GM_LDS),
    ("gmres-chunks33-f64", "non5_c33", F64, GM_KW, {}, None, "hipk_gm_mid_kernel<double,5,false>"),
    ("gmres-chunks-ncu-f64", "non5_ncu", F64, dict(tol=1e-8, restart=20, maxiter=2), {}, None, "hipk_gm_mid_kernel<double,5,false>"),
    ("gmres-chunks-ncu1-f64", "non5_ncu1", F64, dict(tol=1e-8, restart=20, maxiter=2), {}, None, LS),
    ("gmres-restart31-f64", "non5_c40", F64, dict(tol=1e-12, restart=31, maxiter=2), {}, None, "hipk_gm_mid_kernel<double,5,false>"),
    ("gmres-restart32-f64", "non5_c40", F64, dict(tol=1e-12, restart=32, maxiter=2), {}, None, LS),
    ("gmres-row13-f64", "non13", F64, GM_KW, {}, None, LS),
    ("gmres-slots64-f32", "gslots64", F32, GM32_KW, {}, None, "hipk_gm_mid_kernel<float,9,false>"),
    ("gmres-slots65-f32", "gslots65", F32, GM32_KW, {}, None, LS),
    ("gmres-warm-f64", "non5", F64, GM_KW, {}, "rand", "hipk_gm_mid_kernel<double,5,false>"),
    ("gmres-warm-incremental-f32", "non7", F32, {**GM32_KW, "solve_method": "incremental"}, {}, "rand",
     "hipk_gm_mid_kernel<float,7,false>"),
    ("gmres-maxiter1-f64", "non5", F64, dict(tol=1e-12, restart=20, maxiter=1), {}, None, "hipk_gm_mid_kernel<double,5,false>"),
    ("gmres-maxiter2-restart5-f64", "non5", F64, dict(tol=1e-12, restart=5, maxiter=2), {}, "rand", "hipk_gm_mid_kernel<double,5,false>"),
    ("gmres-maxiter0-f64", "non5", F64, dict(tol=1e-8, restart=20, maxiter=0), {}, None, LS),   # no cycle ran
    ("gmres-stop0-f64", "non5", F64, GM_KW, {}, "exact", LS),                                   # no cycle ran
    ("gmres-inside-cycle-batched-f64", "non5", F64, dict(tol=1e-3, restart=30, maxiter=4), {}, None,
     "hipk_gm_mid_kernel<double,5,false>"),
    ("gmres-inside-cycle-incremental-f64", "non5", F64, dict(tol=1e-3, restart=30, maxiter=4, solve_method="incremental"), {},
     None, "hipk_gm_mid_kernel<double,5,false>"),
    ("pgmres-inside-cycle-incremental-f64", "non7", F64, dict(tol=1e-3, restart=30, maxiter=4, solve_method="incremental"), {},
     "rand", "hipk_gm_mid_kernel<double,7,true>"),
    ("gmres-not-resident1-f64", "non5", F64, dict(tol=1e-12, restart=5, maxiter=4), NR1, None,
     "hipk_gm_mid_kernel<double,5,false> -> " + LS),
    ("gmres-not-resident2-f64", "non5", F64, dict(tol=1e-12, restart=5, maxiter=4), {"HIPK_TEST_LDS_NOT_RESIDENT": "2"}, None,
     "hipk_gm_mid_kernel<double,5,false> -> " + LS),
    ("pgmres-not-resident1-f64", "non5", F64, dict(tol=1e-12, restart=5, maxiter=4), NR1, "rand",
     "hipk_gm_mid_kernel<double,5,true> -> " + LS),
]

ORACLE = {"cg": "cg", "pcg": "pcg_jacobi", "bicgstab": "bicgstab", "pbicgstab": "bicgstab_jacobi", "gmres": "gmres",
          "pgmres": "gmres_jacobi"}
_built = {}


def form_of(path):
    """The expected hipk_last_solve_form of a row: a mid loop that finishes the solve names its instantiation as path AND form
    (hipk_*_one_launch: hipk_set_solve_form(path.mid_entry->name)), so the form of such a row is its path literal.  The other rows
    (the launch sequence, the LDS kernels, the hand-backs) finish in forms that tests/_form_cases.py pins by literal; here None:
    the form of the first workspace state, in every state."""
    return path if "_mid_kernel<" in path and " -> " not in path else None


def _matrix(key, dt):
    """(scipy CSR with the stored values, device CSR tensor) for matrix `key` in storage dtype dt (cached per process)."""
    if (key, dt) not in _built:
        if key not in _built:
            _built[key] = MATRICES[key]()
        M = _built[key].copy()
        M.data = M.data.astype(dt)
        A = torch.sparse_csr_tensor(torch.from_numpy(M.indptr.astype(np.int64)), torch.from_numpy(M.indices.astype(np.int64)),
                                    torch.from_numpy(M.data), size=M.shape).to(DEV)
        _built[(key, dt)] = (M, A)
    return _built[(key, dt)]


@pytest.mark.gpu
@pytest.mark.parametrize("cid, key, dtn, kw, env, x0kind, path", CASES, ids=[c[0] for c in CASES])
def test_mid_loop_vs_oracle(hipk, oracle, monkeypatch, cid, key, dtn, kw, env, x0kind, path):
    solver = cid.split("-")[0]
    dt = np.float64 if dtn == F64 else np.float32
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    M, h, b, x0, dinv = build_case(hipk, _matrix, cid, solver, key, dt, x0kind)
    gkw = {k: v for k, v in kw.items() if k in ("restart", "solve_method")}
    print("mid oracle case", cid, flush=True)   # (-s: which case a hang is in)
    st, x, _ = run_solve_case(hipk, cid, solver, h, b, x0, dinv, kw, path, form_of(path), FILLS)

    fn = getattr(oracle, ORACLE[solver] + ("32" if dt == np.float32 else ""))
    args = (M.indptr, M.indices, M.data) + ((dinv,) if dinv is not None else ()) + (b,)
    okw = dict(x0=x0, tol=kw["tol"], atol=0.0, maxiter=kw["maxiter"])
    if solver in ("gmres", "pgmres"):
        okw.update(gkw, gpu_tolerances=True)
    oracle.set_threads(16)
    try:
        ref = fn(*args, **okw)
    finally:
        oracle.set_threads(1)   # (both the fp64 and the fp32 library)
    assert (st.iterations, st.matvecs, st.info, st.breakdown) == (ref.iterations, ref.matvecs, ref.info, ref.breakdown), \
        (cid, (st.iterations, st.matvecs, st.info, st.breakdown), (ref.iterations, ref.matvecs, ref.info, ref.breakdown))
    assert np.array_equal(x, ref.x, equal_nan=True), cid
    _check_stats_long_double(solver, dt, M, dinv, b, x, st, kw)
