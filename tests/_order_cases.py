"""Entry order inside a CSR row: the transformations and the case tables of tests/test_gpu_entry_order.py (the device runs) and
tests/test_order_cases.py (the same tables checked without a GPU).

include/hipk.h promises that a row is summed in STORED order and that unsorted and repeated columns are accepted (DESIGN.md 4
and 7: the rank-count invariance of the row-partitioned solves rests on it -- a rank's boundary rows reach the library with
their ghost columns renumbered and not re-sorted).  Every other matrix builder of the suite produces strictly ascending, unique
columns; here a sorted base matrix of tests/_spmv_cases.py, tests/_form_cases.py, tests/test_gpu_mid_oracle.py or
tests/_cheb_cases.py is transformed, and the transformed arrays ARE the matrix under test: the oracle, the long-double
reference and the library all read the same (crow, col, val), so no equivalence to the sorted matrix is needed or asserted.

Expected kernel notes and forms are written literally, predicted from hipk_launch_spmv / hipk_build_coded (csrc/hipk_api.hip)
and the path-choice functions as tests/_spmv_cases.py and tests/_form_cases.py do.  What a transformation changes for the
dispatch:
  rev, diag_first, dup_diag   every row of a band is rearranged alike: tiles that were uniform stay uniform;
  shuf, dup, dup_shuf, zero   seeded per row: no tile is uniform, so no uniform words (UNI = false without any switch) and no
                              two-rows-per-lane kernel;
  dup, dup_diag, dup_shuf, zero   a row grows by one entry: the tile width, the entries per tile and the row-length guards
                              (12: the register rows of the mid loops; 32: HIPK_LONG_ROW; 1280 / 2048 per tile) move with it;
                              a pair-coded matrix gains at most two (offset, value) pairs per offset, far below 255.

This module imports neither torch nor anything that opens a GPU."""
import numpy as np

import _form_cases as FC
import _spmv_cases as S
from _oracle_cases import _band

DOUBLE, FLOAT = S.DOUBLE, S.FLOAT


# ---------------------------------------------------------------------------------------------- the transformations
def _rows(crow):
    return np.repeat(np.arange(len(crow) - 1), np.diff(crow))


def _take(crow, col, val, order):
    return crow.copy(), np.ascontiguousarray(col[order]), np.ascontiguousarray(val[order])


def rev(crow, col, val, seed=0):
    """Every row in descending storage order."""
    rows = _rows(crow)
    pos = np.arange(len(col)) - crow[:-1][rows]
    return _take(crow, col, val, crow[1:][rows] - 1 - pos)


def diag_first(crow, col, val, seed=0):
    """The diagonal entry at the front of its row, the rest ascending."""
    rows = _rows(crow)
    return _take(crow, col, val, np.lexsort((col, col != rows, rows)))


def shuf(crow, col, val, seed=0):
    """An independent seeded permutation of every row."""
    rng = np.random.default_rng(9_000_001 + seed)
    return _take(crow, col, val, np.lexsort((rng.random(len(col)), _rows(crow))))


def _split(crow, col, val, pick):
    """The entries `pick` (at most one per row) stored twice in place: 0.25 v, then v - 0.25 v."""
    cnt = np.ones(len(col), dtype=np.int64)
    cnt[pick] = 2
    src = np.repeat(np.arange(len(col)), cnt)
    second = np.zeros(len(src), dtype=bool)
    second[1:] = src[1:] == src[:-1]
    first = np.zeros(len(src), dtype=bool)
    first[:-1] = second[1:]
    v = val[src]
    q = val.dtype.type(0.25) * v
    v = np.where(first, q, np.where(second, v - q, v))
    lens = np.diff(crow)
    lens[_rows(crow)[pick]] += 1
    return np.concatenate([[0], np.cumsum(lens)]).astype(crow.dtype), np.ascontiguousarray(col[src]), v


def _seeded_entry(crow, seed):
    """(non-empty rows, one seeded entry index in each)."""
    lens = np.diff(crow)
    ne = np.flatnonzero(lens > 0)
    rng = np.random.default_rng(7_000_003 + seed)
    return ne, crow[:-1][ne] + np.minimum((rng.random(len(ne)) * lens[ne]).astype(np.int64), lens[ne] - 1)


def dup(crow, col, val, seed=0):
    """One seeded entry of every non-empty row split into two stored entries of the same column."""
    return _split(crow, col, val, _seeded_entry(crow, seed)[1])


def dup_diag(crow, col, val, seed=0):
    """The diagonal entry of every row that has one split into two stored entries."""
    return _split(crow, col, val, np.flatnonzero(col == _rows(crow)))


def dup_shuf(crow, col, val, seed=0):
    """dup, then shuf: the two halves are in general not adjacent."""
    return shuf(*dup(crow, col, val, seed), seed=seed)


def zero(crow, col, val, seed=0):
    """One explicitly stored 0.0 appended to every non-empty row, at the column of a seeded entry of that row."""
    ne, at = _seeded_entry(crow, seed + 1)
    rows = np.concatenate([_rows(crow), ne])
    key = np.concatenate([np.arange(len(col)), np.full(len(ne), len(col))])
    order = np.lexsort((key, rows))
    lens = np.diff(crow)
    lens[ne] += 1
    col2, val2 = np.concatenate([col, col[at]]), np.concatenate([val, np.zeros(len(ne), dtype=val.dtype)])
    return np.concatenate([[0], np.cumsum(lens)]).astype(crow.dtype), np.ascontiguousarray(col2[order]), np.ascontiguousarray(val2[order])


TRANSFORMS = {"rev": rev, "diag_first": diag_first, "shuf": shuf, "dup": dup, "dup_diag": dup_diag, "dup_shuf": dup_shuf, "zero": zero}
UNSORTED = ("rev", "diag_first", "shuf", "dup_shuf")     # most rows contain a descent
DUPLICATED = ("dup", "dup_diag", "dup_shuf")             # every non-empty row has a repeated column
SAME_IN_EVERY_ROW = ("rev", "diag_first", "dup_diag")    # a band's uniform tiles stay uniform
GROWS = ("dup", "dup_diag", "dup_shuf", "zero")          # a row gains one entry


def descents(crow, col):
    """Per row: does its stored column sequence step down somewhere?"""
    n = len(crow) - 1
    rows = _rows(crow)
    down = (col[1:] < col[:-1]) & (rows[1:] == rows[:-1])
    out = np.zeros(n, dtype=bool)
    out[rows[1:][down]] = True
    return out


def has_repeat(crow, col):
    """Per row: is a column stored more than once?"""
    n = len(crow) - 1
    rows = _rows(crow)
    order = np.lexsort((col, rows))
    r, c = rows[order], col[order]
    same = (c[1:] == c[:-1]) & (r[1:] == r[:-1])
    out = np.zeros(n, dtype=bool)
    out[r[1:][same]] = True
    return out


# ---------------------------------------------------------------------------------------------- SpMV sweep
# a ragged band for the CSR-ordered code layout: row i keeps the diagonal and a seeded subset of eleven offsets
RAGGED = "rag11c"
N_RAGGED = S.N_SMALL


def base_matrix(name):
    """(crow, col, val) in fp64, strictly ascending unique columns."""
    if name != RAGGED:
        return S.matrix(name)
    crow, col, val = S.matrix("s11c")
    rows = _rows(crow)
    keep = (np.random.default_rng(11).random(len(col)) < 0.55) | (col == rows)
    lens = np.bincount(rows[keep], minlength=len(crow) - 1)
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), col[keep], val[keep]


def base_rows(name):
    return N_RAGGED if name == RAGGED else S.MATRICES[name][0]


_arrays = {}


def arrays(matrix, transform, dtype):
    """The matrix under test: the base transformed in fp64, values then rounded to the storage type.  Of the 2.2 M-row ones the
    last is kept."""
    key = (matrix, transform)
    if key not in _arrays:
        if base_rows(matrix) > S.N_SMALL:
            for k in [k for k in _arrays if base_rows(k[0]) > S.N_SMALL]:
                del _arrays[k]
        _arrays[key] = TRANSFORMS[transform](*base_matrix(matrix), seed=len(matrix))
    crow, col, val = _arrays[key]
    return crow, col, val if dtype == DOUBLE else val.astype(np.float32)


def vectors(matrix, dtype):
    """(x, w, b): standard normal, rounded to the storage type."""
    n = base_rows(matrix)
    rng = np.random.default_rng(2_000_003 + n + len(matrix))
    f = np.float64 if dtype == DOUBLE else np.float32
    return tuple(rng.standard_normal(n).astype(f) for _ in range(3))


STRIDED, LAYOUT, NO_MODE = S.STRIDED, S.LAYOUT, S.NO_MODE
PLAIN64_1280, PLAIN64_2048, PLAIN64_GEN = "hipk_spmv_kernel<double,1280,true>", "hipk_spmv_kernel<double,2048,true>", "hipk_spmv_kernel<double,1280,false>"
PLAIN32_2048, PLAIN32_GEN = "hipk_spmv_kernel<float,2048,true>", "hipk_spmv_kernel<float,2048,false>"

# name: matrix, transform, dtype, env (set before the handle exists), fresh (None: in the test process; else the child's group), runs
# (every case: all eight modes and <x, A x>), steps, plain_only, also_plain (afterwards the same runs on the plain CSR kernels, equal
# bits required: every case that does not start there), idx32 (crow / col handed over as int32)
SPMV = {}


def _spmv(name, matrix, transform, dtype, notes, env=None, fresh=None, plain_only=False, idx32=False):
    assert name not in SPMV, name
    SPMV[name] = dict(matrix=matrix, transform=transform, dtype=dtype, env=dict(env or {}), fresh=fresh, runs=S.RUNS_WX,
                      steps=[({}, notes)], plain_only=plain_only, also_plain=not plain_only, idx32=idx32)


# ---- n = 70 001: the persistent walk (35 chunks never fill the resident workgroups) ...
_spmv("persistent_f64_s5c_rev", "s5c", "rev", DOUBLE, S.loop(DOUBLE, 5, False, False, True))               # uniform words kept
_spmv("persistent_f32_s5c_shuf", "s5c", "shuf", FLOAT, S.loop(FLOAT, 5, False, False, False))              # no tile uniform
_spmv("persistent_f64_s5r_dup", "s5r", "dup", DOUBLE, S.loop(DOUBLE, 0, False, True, False))               # 6 units: run-time width
_spmv("persistent_f32_s7r_dup_diag", "s7r", "dup_diag", FLOAT, S.loop(FLOAT, 8, False, True, True))        # 8 entries, offsets uniform
_spmv("persistent_f64_s3c_zero", "s3c", "zero", DOUBLE, S.loop(DOUBLE, 4, False, False, False))            # 4 entries, one a stored 0.0
_spmv("persistent_f32_s8c_zero", "s8c", "zero", FLOAT, S.loop(FLOAT, 0, False, False, False))              # 9 units
_spmv("persistent_f64_s11c_dup_shuf", "s11c", "dup_shuf", DOUBLE, S.loop(DOUBLE, 0, False, False, False))  # 12 units: three code groups
# ... HIPK_SPMV_SELL_STRIDED=1: the two-rows-per-lane kernel where half of the tiles are uniform (fp64, pair codes, 4 | 5 | 8
# units), else groups of four tiles on the one-row-per-lane kernel
_spmv("wide_s8c_diag_first_walk1", "s8c", "diag_first", DOUBLE, S.wide(8, 1), env={STRIDED: "1"})          # w = x from entry 0's load
_spmv("wide_s4c_dup_diag_walk1", "s4c", "dup_diag", DOUBLE, S.wide(5, 1), env={STRIDED: "1"})              # two entries of offset 0
_spmv("wide_s3c_rev_walk1", "s3c", "rev", DOUBLE, S.wide(4, 1), env={STRIDED: "1"})
_spmv("wide_s7c_rev_walk1", "s7c", "rev", DOUBLE, S.wide(8, 1), env={STRIDED: "1"})
_spmv("groups_f64_s5c_shuf", "s5c", "shuf", DOUBLE, S.loop(DOUBLE, 5, True, False, False, groups=True), env={STRIDED: "1"})
_spmv("groups_f32_s4r_dup_shuf", "s4r", "dup_shuf", FLOAT, S.loop(FLOAT, 5, True, True, False, groups=True), env={STRIDED: "1"})
_spmv("groups_f32_s6c_rev", "s6c", "rev", FLOAT, S.loop(FLOAT, 0, True, False, True, groups=True), env={STRIDED: "1"})
# ... outside the sliced-ELL forms: the CSR-ordered code layout on ragged rows, rows beyond HIPK_LONG_ROW, a row per wavefront
_spmv("codedcsr_f64_rag11c_shuf", RAGGED, "shuf", DOUBLE, S.same("hipk_spmv_coded_kernel<double,1>"), env={LAYOUT: "csr"})
_spmv("codedcsr_f32_rag11c_dup_shuf", RAGGED, "dup_shuf", FLOAT, S.same("hipk_spmv_coded_kernel<float,1>"), env={LAYOUT: "csr"})
_spmv("plain_f64_l41c_rev", "l41c", "rev", DOUBLE, S.same(PLAIN64_GEN), plain_only=True)       # no coded form: starts on the plain kernels
_spmv("plain_f32_l41c_dup_shuf", "l41c", "dup_shuf", FLOAT, S.same(PLAIN32_GEN), plain_only=True)
_spmv("rowwave_f64_d50c_shuf", "d50c", "shuf", DOUBLE, S.same("hipk_spmv_rowwave_kernel<double>"), plain_only=True)
_spmv("rowwave_f32_d50c_dup_shuf", "d50c", "dup_shuf", FLOAT, S.same("hipk_spmv_rowwave_kernel<float>"), plain_only=True)
# ... the plain tile kernels by entries per tile (set_path(plain_only=True)): 1280 stays, + 256 leaves the fp64 fast size, 2304
_spmv("plain_f64_s5c_rev", "s5c", "rev", DOUBLE, S.same(PLAIN64_1280), plain_only=True)
_spmv("plain_f64_s5c_dup", "s5c", "dup", DOUBLE, S.same(PLAIN64_2048), plain_only=True)
_spmv("plain_f32_s8c_diag_first", "s8c", "diag_first", FLOAT, S.same(PLAIN32_2048), plain_only=True)
_spmv("plain_f32_s8c_dup_shuf", "s8c", "dup_shuf", FLOAT, S.same(PLAIN32_GEN), plain_only=True)
# ---- n = 2 200 077: a workgroup per reduction chunk (one or two cases per chunk-walk family, six in all)
_spmv("pair_f32_b5c_shuf", "b5c", "shuf", FLOAT, S.pair(FLOAT, 5, False))
_spmv("pair_f64_b5c_shuf", "b5c", "shuf", DOUBLE, S.pair(DOUBLE, 5, False))                     # modes 1 and 2 compiled in
_spmv("pair_f32_b8c_rev", "b8c", "rev", FLOAT, S.pair(FLOAT, 8, True))
_spmv("wide_b5c_diag_first_walk0", "b5c", "diag_first", DOUBLE, S.wide(5, 0), env={STRIDED: "0"})
_spmv("wide_b7c_dup_diag_walk0", "b7c", "dup_diag", DOUBLE, S.wide(8, 0), env={STRIDED: "0"})
_spmv("chunk_f64_b5r_dup_shuf", "b5r", "dup_shuf", DOUBLE, S.loop(DOUBLE, 0, True, True, False))
# ---- a switch that a process reads once: run-time mode bits on the two-rows-per-lane kernel, in a child process
_spmv("nomode_wide_s5c_diag_first_walk1", "s5c", "diag_first", DOUBLE, S.wide(5, 1, no_mode=True), env={NO_MODE: "1", STRIDED: "1"}, fresh="no_mode")
_spmv("nomode_wide_s7c_dup_diag_walk1", "s7c", "dup_diag", DOUBLE, S.wide(8, 1, no_mode=True), env={NO_MODE: "1", STRIDED: "1"}, fresh="no_mode")
# ---- int32 crow / col (idx_bytes 4): the same references, so the same bits
for _base in ("persistent_f32_s5c_shuf", "persistent_f64_s5r_dup", "wide_s8c_diag_first_walk1", "groups_f32_s4r_dup_shuf",
              "codedcsr_f64_rag11c_shuf", "rowwave_f64_d50c_shuf"):
    _c = SPMV[_base]
    _spmv(_base + "_i32", _c["matrix"], _c["transform"], _c["dtype"], _c["steps"][0][1], env=_c["env"], plain_only=_c["plain_only"], idx32=True)

CASES = SPMV                      # the name tests/_spmv_inst_worker.py reads a table by
FRESH_GROUPS = sorted({c["fresh"] for c in SPMV.values() if c["fresh"]})
BIG_CASES = sorted(n for n, c in SPMV.items() if base_rows(c["matrix"]) > S.N_SMALL)


# ---------------------------------------------------------------------------------------------- Chebyshev epilogue
# name: offsets of tests/_cheb_cases.py: band(), n, transform, dtype, env, plain_only, the note of hipk_cheb_apply (degree 3).
# The two-rows-per-lane kernel needs uniform tiles: under dup_shuf no tile is uniform, the handle takes the one-row-per-lane coded
# kernels, which have no epilogue, and the apply is SpMV + hipk_cheb_step_kernel -- the case stays, with that note, and dup_diag
# stands in as the duplicate-carrying form of the epilogue kernel.
N_CHEB = S.N_SMALL
CHEB_OFFSETS = {"band4": [-40, -1, 0, 1], "band5": [-40, -1, 0, 1, 40], "band7": [-300, -40, -1, 0, 1, 40, 300]}
STEP64, STEP32 = " + hipk_cheb_step_kernel<double>", " + hipk_cheb_step_kernel<float>"
CHEB = {
    "wide5_diag_first": ("band5", "diag_first", DOUBLE, {STRIDED: "1"}, False, "hipk_spmv_sell_wide_kernel<5,28,1>"),
    "wide5_dup_diag": ("band4", "dup_diag", DOUBLE, {STRIDED: "1"}, False, "hipk_spmv_sell_wide_kernel<5,28,1>"),
    "wide8_diag_first": ("band7", "diag_first", DOUBLE, {STRIDED: "1"}, False, "hipk_spmv_sell_wide_kernel<8,28,1>"),
    "wide5_dup_shuf_no_epilogue": ("band4", "dup_shuf", DOUBLE, {STRIDED: "1"}, False,
                                   "hipk_spmv_sell_loop_kernel<double,5,true,false,false>/groups" + STEP64),
    "tile1280_diag_first": ("band5", "diag_first", DOUBLE, {}, True, "hipk_spmv_cheb_kernel<double,1280>"),
    "tile1280_dup_shuf": ("band4", "dup_shuf", DOUBLE, {}, True, "hipk_spmv_cheb_kernel<double,1280>"),            # 1280 entries per tile
    "tile2048_diag_first": ("band7", "diag_first", DOUBLE, {}, True, "hipk_spmv_cheb_kernel<double,2048>"),
    "tile2048_dup_shuf": ("band7", "dup_shuf", DOUBLE, {}, True, "hipk_spmv_cheb_kernel<double,2048>"),            # 2048: the inclusive edge
    "tile2048_f32_diag_first": ("band5", "diag_first", FLOAT, {}, True, "hipk_spmv_cheb_kernel<float,2048>"),
    "tile2048_f32_dup_shuf": ("band5", "dup_shuf", FLOAT, {}, True, "hipk_spmv_cheb_kernel<float,2048>"),
}


# ---------------------------------------------------------------------------------------------- solver sweep
N46 = FC.N46
CH = FC.CH
MATRICES = dict(FC.MATRICES)
MATRICES.update({      # the mid-loop matrices of tests/test_gpu_mid_oracle.py (46 chunks, the last ragged), and the guard edges
    "sym5": lambda: _band(N46, (1, 2)),
    "sym11": lambda: _band(N46, (1, 2, 3, 4, 5)),
    "sym12": lambda: _band(N46, (1, 2, 3, 4, 5), match=300),
    "non5": lambda: _band(N46, (1, 2), sym=False, seed=1),
    "non12": lambda: _band(N46, (1, 2, 3, 4, 5), match=300, sym=False, seed=1),
    "star31_c33": lambda: FC._star(32 * CH + 1, 20000, 28),
})


def solver_matrix(key, transform, dt):
    """(crow, col, val) of a solver case: the scipy base (sorted, unique), transformed, values in the storage dtype `dt`."""
    M = MATRICES[key]()
    crow, col, val = TRANSFORMS[transform](M.indptr.astype(np.int64), M.indices.astype(np.int64), M.data.astype(np.float64), seed=len(key))
    return crow, col, val.astype(dt)


F64, F32, LS = FC.F64, FC.F32, FC.LS
KW, KW32, GM, GM32, GMR = FC.KW, FC.KW32, FC.GM, FC.GM32, FC.GMR
CB = {"callback": True}


def _lds(kind, t, local, pre=None):
    k = f"hipk_{kind}_solve_lds_kernel"
    return (k, f"{k}<{t},{'true' if local else 'false'}" + ("" if pre is None else f",{'true' if pre else 'false'}") + ">")


def _mid(kind, t, w, pre, nch=None):
    f = f"hipk_{kind}_mid_kernel<{t},{w}," + ("" if nch is None else f"{nch},") + f"{'true' if pre else 'false'}>"
    return (f, f)


D, F = "double", "float"
# (id, solver, matrix, dtype, solve options, environment, x0, {transform: (expected hipk_last_solve_path, expected hipk_last_solve_form)})
_S = [
    # ---- the whole-solve LDS kernels, LOCAL true (one XCD) and false (spread over the chip); rows of 5 and, with the duplicate, 6
    ("cg-lds-c1r-f64", "cg", "s5_c1r", F64, KW, {}, None, {"rev": _lds("cg", D, True, False), "dup_shuf": _lds("cg", D, True, False)}),
    ("pcg-lds-c1r-f32", "pcg", "s5_c1r", F32, KW32, {}, "rand", {"rev": _lds("cg", F, True, True), "dup_shuf": _lds("cg", F, True, True)}),
    ("cg-spread-mid0-c9-f64", "cg", "s5_c9", F64, KW, FC.MID0, None, {"rev": _lds("cg", D, False, False), "dup_shuf": _lds("cg", D, False, False)}),
    ("bicgstab-lds-c1r-f64", "bicgstab", "n5_c1r", F64, KW, {}, None, {"rev": _lds("bi", D, True, False), "dup_shuf": _lds("bi", D, True, False)}),
    ("pbicgstab-spread-mid0-c9-f32", "pbicgstab", "n5_c9", F32, KW32, FC.BMID0, None,
     {"rev": _lds("bi", F, False, True), "dup_shuf": _lds("bi", F, False, True)}),
    ("gmres-lds-c1r-f64", "gmres", "n5_c1r", F64, GM, {}, None, {"rev": _lds("gm", D, True), "dup_shuf": _lds("gm", D, True)}),
    ("pgmres-spread-c9-f32", "pgmres", "n5_c9", F32, GM32, {}, "rand", {"rev": _lds("gm", F, False), "dup_shuf": _lds("gm", F, False)}),
    ("gmres-cycle-small-f64", "gmres", "n5_g1r", F64, GM, {"HIPK_GMRES_NO_LDS_CYCLE": "1"}, None,
     {"rev": (FC.GM_SMALL, "hipk_gm_cycle_small_kernel<double>"), "dup_shuf": (FC.GM_SMALL, "hipk_gm_cycle_small_kernel<double>")}),
    # ---- the mid loops at two row widths, with and without Jacobi: 5 entries + the duplicate take the W = 7 instantiation; 12 + the
    # duplicate = 13 leave the loop for the form of the 13-entry sorted sibling (cg-row13, bicgstab-row13, gmres-row13)
    ("cg-mid-sym5-f64", "cg", "sym5", F64, KW, {}, None, {"rev": _mid("cg", D, 5, False, 1), "dup_shuf": _mid("cg", D, 7, False, 1)}),
    ("pcg-mid-sym5-f32", "pcg", "sym5", F32, KW32, {}, None, {"rev": _mid("cg", F, 5, True, 1), "dup_shuf": _mid("cg", F, 7, True, 1)}),
    ("cg-mid-sym12-f64", "cg", "sym12", F64, KW, {}, "rand", {"rev": _mid("cg", D, 12, False, 1), "dup_shuf": (LS, FC.CG3)}),
    ("pcg-mid-sym12-f64", "pcg", "sym12", F64, KW, {}, None, {"rev": _mid("cg", D, 12, True, 1), "dup_shuf": (LS, FC.PCG3)}),
    ("bicgstab-mid-non5-f64", "bicgstab", "non5", F64, KW, {}, None, {"rev": _mid("bi", D, 5, False), "dup_shuf": _mid("bi", D, 7, False)}),
    ("pbicgstab-mid-non12-f32", "pbicgstab", "non12", F32, KW32, {}, None, {"rev": _mid("bi", F, 12, True), "dup_shuf": (LS, FC.BI5J)}),
    ("gmres-mid-non5-f64", "gmres", "non5", F64, GM, {}, None, {"rev": _mid("gm", D, 5, False), "dup_shuf": _mid("gm", D, 7, False)}),
    ("pgmres-mid-non12-f32", "pgmres", "non12", F32, GM32, {}, None, {"rev": _mid("gm", F, 12, True), "dup_shuf": (LS, FC.GLS)}),
    # guard edge of the register rows (kCgRowRegs = 12): 11 entries + the duplicate = 12 still take the mid loop
    ("cg-mid-sym11-f64", "cg", "sym11", F64, KW, {}, None, {"dup": _mid("cg", D, 12, False, 1)}),
    ("cg-mid-sym12-dup-f64", "cg", "sym12", F64, KW, {}, None, {"dup": (LS, FC.CG3)}),
    # ---- two-launch CG: hipk_cg2_spmv_kernel tiles rows through an LDS product buffer of 1280 (fp64) / 2048 (fp32) entries.  A full
    # tile of 1280 + 256 duplicates leaves the fp64 form and stays in the fp32 one; rows of 31 + 1 = 32 stay (HIPK_LONG_ROW), 32 + 1 leave
    ("cg2-c33-mid0-f64", "cg", "s5_c33", F64, KW, FC.MID0, None, {"rev": (LS, FC.CG2_64), "dup_shuf": (LS, FC.CG3), "dup": (LS, FC.CG3)}),
    ("cg2-c33-mid0-f32", "cg", "s5_c33", F32, KW32, FC.MID0, None, {"rev": (LS, FC.CG2_32), "dup_shuf": (LS, FC.CG2_32)}),
    ("cg2-row31-f64", "cg", "star31_c33", F64, KW, {}, None, {"rev": (LS, FC.CG2_64), "dup": (LS, FC.CG2_64), "dup_shuf": (LS, FC.CG2_64)}),
    ("cg2-row32-f64", "cg", "star32_c33", F64, KW, {}, None, {"rev": (LS, FC.CG2_64), "dup": (LS, FC.CG3)}),
    # ---- the three-launch and five-launch sequences, small (<= 8 chunks) and general, Jacobi and callback M (rows of 13: no loop)
    ("cg-small-row13-f64", "cg", "s13_c1r", F64, KW, {}, None, {"rev": (LS, FC.CG3S), "dup_shuf": (LS, FC.CG3S)}),
    ("cg-general-row13-c9-f32", "cg", "s13_c9", F32, KW32, {}, None, {"rev": (LS, FC.CG3), "dup_shuf": (LS, FC.CG3)}),
    ("pcg-seq-row13-f64", "pcg", "s13_c1r", F64, KW, {}, None, {"rev": (LS, FC.PCG3), "dup_shuf": (LS, FC.PCG3)}),
    ("bicgstab-small-row13-f64", "bicgstab", "n13_c1r", F64, KW, {}, None, {"rev": (LS, FC.BI5S), "dup_shuf": (LS, FC.BI5S)}),
    ("bicgstab-general-row13-c9-f32", "bicgstab", "n13_c9", F32, KW32, {}, None, {"rev": (LS, FC.BI5), "dup_shuf": (LS, FC.BI5)}),
    ("pbicgstab-small-row13-f64", "pbicgstab", "n13_c1r", F64, KW, {}, None, {"rev": (LS, FC.BI5SJ), "dup_shuf": (LS, FC.BI5SJ)}),
    ("pbicgstab-general-row13-c9-f64", "pbicgstab", "n13_c9", F64, KW, {}, "rand", {"rev": (LS, FC.BI5J), "dup_shuf": (LS, FC.BI5J)}),
    ("pbicgstab-callback-small-f64", "pbicgstab", "n5_c1r", F64, {**KW, **CB}, {}, None,
     {"rev": (LS, FC.BI5S + FC.CB), "dup_shuf": (LS, FC.BI5S + FC.CB)}),
    ("pbicgstab-callback-general-f64", "pbicgstab", "n5_c9", F64, {**KW, **CB}, {}, None,
     {"rev": (LS, FC.BI5 + FC.CB), "dup_shuf": (LS, FC.BI5 + FC.CB)}),
    # ---- GMRES launch sequences: small + wide and + 256-thread, large first kernels and streaming, restart > 31; callback M
    ("gmres-small-wide-f64", "gmres", "n5_g1r", F64, GM, {"HIPK_GMRES_NO_CYCLE": "1"}, None, {"rev": (LS, FC.GSW), "dup_shuf": (LS, FC.GSW)}),
    ("gmres-small-256-f32", "gmres", "n5_c1r", F32, GM32, {"HIPK_GMRES_NO_WIDE": "1"}, None, {"rev": (LS, FC.GS256), "dup_shuf": (LS, FC.GS256)}),
    ("gmres-large-first-f64", "gmres", "n5_c9", F64, GM, {**FC.NOSPREAD, "HIPK_GMRES_NO_STREAM": "1"}, None,
     {"rev": (LS, FC.GLF), "dup_shuf": (LS, FC.GLF)}),
    ("gmres-nospread-c9-f64", "gmres", "n5_c9", F64, GM, FC.NOSPREAD, None, {"rev": (LS, FC.GLS), "dup_shuf": (LS, FC.GLS)}),
    ("gmres-big-r32-c1r-f64", "gmres", "n5_c1r", F64, GMR(32, maxiter=3), {}, None, {"rev": (LS, FC.GBIG), "dup_shuf": (LS, FC.GBIG)}),
    ("pgmres-big-r64-c9-f32", "pgmres", "n5_c9", F32, GMR(64, tol=1e-5), {}, None, {"rev": (LS, FC.GBIG), "dup_shuf": (LS, FC.GBIG)}),
    ("pgmres-callback-small-wide-f64", "pgmres", "n5_c1r", F64, {**GM, **CB}, {}, None,
     {"rev": (LS, FC.GSW + FC.CB), "dup_shuf": (LS, FC.GSW + FC.CB)}),
    ("pgmres-callback-large-streaming-f64", "pgmres", "n5_c9", F64, {**GM, **CB}, {}, None,
     {"rev": (LS, FC.GLS + FC.CB), "dup_shuf": (LS, FC.GLS + FC.CB)}),
]
# one row per (case, transformation), in the layout of tests/_form_cases.py: CASES with the transformation after the matrix
SOLVES = [(f"{cid}-{tr}", solver, key, tr, dtn, kw, env, x0, path, form)
          for cid, solver, key, dtn, kw, env, x0, by in _S for tr, (path, form) in by.items()]
# solver cases repeated with int32 crow / col
SOLVES_I32 = ("cg-mid-sym5-f64-dup_shuf", "bicgstab-lds-c1r-f64-rev", "gmres-nospread-c9-f64-dup_shuf")


def form_family(form):
    """The family of a row of hipk_solve_form_name: a kernel's template name (the LDS kernels: with LOCAL), a launch sequence's name
    without what only says how M is applied from outside (", callback M"), how a norm is formed (" + split norm") or which cache
    policy the vector kernels take (", streams ...")."""
    if form.startswith("hipk_") and "_solve_lds_kernel<" in form:
        return form.split("<")[0] + " LOCAL=" + form.split("<")[1].split(",")[1].rstrip(">")
    if form.startswith("hipk_"):
        return form.split("<")[0]
    for cut in (", callback M", " + split norm", ", streams + flat direction", ", streams"):
        form = form.replace(cut, "")
    return form


def spmv_templates(notes):
    """The kernel templates a collection of notes names: the text before '<' of every ' + ' part, with a '/groups' suffix kept."""
    out = set()
    for note in notes:
        for part in note.split(" + "):
            out.add(part.split("<")[0] + ("/groups" if part.endswith("/groups") else ""))
    return out


def sweep_notes(spmv=None, cheb=None):
    """Every note the SpMV and Chebyshev tables of this module expect."""
    spmv = SPMV if spmv is None else spmv
    cheb = CHEB if cheb is None else cheb
    out = {notes[m] for c in spmv.values() for _, notes in c["steps"] for m, _wx in c["runs"]}
    return out | {c[5] for c in cheb.values()}


# A kernel template or form family that provably cannot be selected for unsorted or duplicate rows: {name: the dispatch condition,
# quoted}.  tests/test_gpu_entry_order.py asserts that none of these is ever reported.  Empty: every template that
# tests/_spmv_cases.py and tests/_cheb_cases.py name and every form family has a case above.
UNREACHABLE_UNSORTED = {}
