"""Case table of tests/test_gpu_spmv_instantiations.py (the device runs) and tests/test_spmv_cases.py (the same table checked
without a GPU): for every SpMV kernel instantiation that hipk_launch_spmv (csrc/hipk_api.hip) can choose, a matrix, a storage
type, the HIPK_* switches to set BEFORE the handle exists, the hipk_spmv_ex modes to run and, per mode, the kernel note the
dispatch must report (hipk_last_spmv_kernel).  The Chebyshev instantiations belong to tests/_cheb_cases.py.

This module imports neither torch nor anything that opens a GPU; matrix() imports the band builder when it is called.

What the dispatch keys on, as read from hipk_launch_spmv and hipk_build_coded:
  UNITS   the common tile width in units of 256 B (hipk_sell_units of the longest row: 3 -> 4, 7 -> 8, 11 -> 12), as a template
          argument when it is 4, 5 or 8, else 0;
  VALS    at most 255 distinct (offset, value) pairs: pair codes (false); else offsets only + value planes (true);
  UNI     uniform-tile words exist: HIPK_SPMV_UNIFORM not 0, tiles of at most 8 units, a quarter of the tiles uniform;
  T       storage type;
  walk    persistent (CHUNKED = false) unless the reduction chunks about fill the resident workgroups (n = 2 200 077: 1075 chunks);
          HIPK_SPMV_SELL_STRIDED=1: groups of 4 tiles -- "/groups" on the one-row-per-lane kernel, WALK = 1 on the two-rows-per-lane
          kernel; =0: WALK = 0;
  family  chunk walk + pair codes + UNITS in 4, 5, 8: the pair kernel; fp64 with half of the tiles uniform: the two-rows-per-lane
          ("wide") kernel instead, unless HIPK_SPMV_SELL_NO_WIDE is set;
  MODE    wide: modes 0 .. 3 compiled in, 4 .. 7 -> -1; pair<double,5,U,.>: modes 1 and 2 compiled in, else -1;
          HIPK_SPMV_SELL_NO_MODE: always -1."""
import numpy as np

N_SMALL = 70_001        # 274 tiles, the last of 113 rows; 35 reduction chunks: the persistent walk
N_BIG = 2_200_077       # 8595 tiles, the last of 13 rows; 1075 chunks of 2048 rows, the last ragged: a workgroup per chunk
MODES = tuple(range(8))
DOUBLE, FLOAT = "double", "float"
UNITS = {3: 4, 4: 4, 5: 5, 6: 0, 7: 8, 8: 8, 9: 0, 11: 0}      # entries per row -> the UNITS template argument

_SMALL = {3: [-1, 0, 1], 4: [-40, -1, 0, 1], 5: [-40, -1, 0, 1, 40], 6: [-40, -2, -1, 0, 1, 40],
          7: [-300, -40, -1, 0, 1, 40, 300], 8: [-300, -40, -2, -1, 0, 1, 40, 300],
          9: [-300, -40, -2, -1, 0, 1, 2, 40, 300], 11: [-300, -40, -9, -2, -1, 0, 1, 2, 9, 40, 300]}
_BIG = {3: [-1, 0, 1], 4: [-1500, -1, 0, 1], 5: [-1500, -1, 0, 1, 1500], 6: [-1500, -2, -1, 0, 1, 1500],
        7: [-9000, -1500, -1, 0, 1, 1500, 9000], 8: [-9000, -1500, -2, -1, 0, 1, 1500, 9000]}

# name: (n, offsets, values).  "c": one value per offset (pair codes); "r": a random value per entry (offset codes, value planes --
# the offsets of a band are the same in every row, so the offset codes are uniform per tile although the coefficients vary)
MATRICES = {}
for _w, _o in _SMALL.items():
    MATRICES[f"s{_w}c"] = (N_SMALL, _o, "c")
    MATRICES[f"s{_w}r"] = (N_SMALL, _o, "r")
for _w, _o in _BIG.items():
    MATRICES[f"b{_w}c"] = (N_BIG, _o, "c")
for _w in (4, 5, 6, 8):
    MATRICES[f"b{_w}r"] = (N_BIG, _BIG[_w], "r")
MATRICES["l41c"] = (20_011, list(range(-20, 21)), "c")      # 41 entries per row: longer than 32, no coded form
MATRICES["d50c"] = (5_000, list(range(-25, 25)), "c")       # mean row length 49.87 >= 48: a row per wavefront


def matrix(name):
    """(crow, col, val) in fp64.  "c": the k-th offset carries (k + 1) / 7 - 0.9; "r": standard normal values."""
    from test_gpu_coded import banded
    n, offsets, kind = MATRICES[name]
    if kind == "c":
        vals = (np.arange(len(offsets)) + 1.0) / 7.0 - 0.9
        return banded(n, offsets, lambda r, k: vals[k])
    rng = np.random.default_rng(n + 31 * len(offsets))
    return banded(n, offsets, lambda r, k: rng.standard_normal(len(r)))


def vectors(name, dtype):
    """(x, w, b) of a matrix: standard normal, rounded to the storage type."""
    n = MATRICES[name][0]
    rng = np.random.default_rng(1_000_003 + n + len(MATRICES[name][1]))
    f = np.float64 if dtype == DOUBLE else np.float32
    return tuple(rng.standard_normal(n).astype(f) for _ in range(3))


# ---------------------------------------------------------------------------------------------- the notes, written as the launcher prints them
def _b(v):
    return "true" if v else "false"


def loop(t, units, chunked, vals, uni, groups=False):
    return {m: f"hipk_spmv_sell_loop_kernel<{t},{units},{_b(chunked)},{_b(vals)},{_b(uni)}>" + ("/groups" if groups else "") for m in MODES}


def wide(units, walk, no_mode=False):
    return {m: f"hipk_spmv_sell_wide_kernel<{units},{m if m <= 3 and not no_mode else -1},{walk}>" for m in MODES}


def pair(t, units, uni, no_mode=False):
    return {m: f"hipk_spmv_sell_pair_kernel<{t},{units},{_b(uni)},{m if (t == DOUBLE and units == 5 and m in (1, 2) and not no_mode) else -1}>"
            for m in MODES}


def same(note):
    return {m: note for m in MODES}


RUNS = tuple((m, False) for m in MODES)          # (mode, w is x)
RUNS_WX = RUNS + ((1, True),)                    # the CG loop's <p, A p>: the wide kernel takes w from the diagonal entry's load
STRIDED, UNIFORM, NO_WIDE, LAYOUT = "HIPK_SPMV_SELL_STRIDED", "HIPK_SPMV_UNIFORM", "HIPK_SPMV_SELL_NO_WIDE", "HIPK_SPMV_CODED_LAYOUT"
NO_MODE, NO_PAIR, NO_PLAN, CHUNKED = "HIPK_SPMV_SELL_NO_MODE", "HIPK_SPMV_SELL_NO_PAIR", "HIPK_SPMV_NO_PLAN_CACHE", "HIPK_SPMV_SELL_CHUNKED"

# name: matrix, dtype, env (set before the handle exists), fresh (None: in this process; else the child process's group), runs,
# steps ((switches to change before the step: None unsets; expected note per mode), all on ONE handle), plain_only (set_path before
# the runs), also_plain (afterwards the same runs on the plain CSR kernels, equal bits required)
CASES = {}


def _case(name, matrix, dtype, notes, env=None, fresh=None, runs=RUNS, steps=None, plain_only=False, also_plain=False):
    assert name not in CASES, name
    CASES[name] = dict(matrix=matrix, dtype=dtype, env=dict(env or {}), fresh=fresh, runs=tuple(runs),
                       steps=steps if steps is not None else [({}, notes)], plain_only=plain_only, also_plain=also_plain)


def _off(env, uni):
    """env, with the uniform words removed unless `uni`."""
    return dict(env, **({} if uni else {UNIFORM: "0"}))


for _t in (DOUBLE, FLOAT):
    _s = "f64" if _t == DOUBLE else "f32"
    # A. persistent walk (35 chunks never fill the resident workgroups; HIPK_SPMV_SELL_STRIDED unset and 8 tiles per chunk: no
    #    grouped walk, so not the wide kernel either): loop<T,UNITS,false,VALS,UNI>.  Tiles of 9 and 12 units are never uniform.
    for _v in ("c", "r"):
        for _w in (3, 4, 5, 6, 7, 8, 9, 11):
            _case(f"persistent_{_s}_s{_w}{_v}", f"s{_w}{_v}", _t, loop(_t, UNITS[_w], False, _v == "r", _w <= 8))
        for _w in (4, 5, 6, 8):
            _case(f"persistent_{_s}_s{_w}{_v}_nouni", f"s{_w}{_v}", _t, loop(_t, UNITS[_w], False, _v == "r", False), env={UNIFORM: "0"})
    # B. grouped walk of the one-row-per-lane kernel, forced: loop<T,UNITS,true,VALS,UNI>/groups.  Where the wide kernel would take
    #    the grouped walk (fp64, pair codes, uniform, UNITS 4 | 5 | 8) HIPK_SPMV_SELL_NO_WIDE keeps it away.
    for _v in ("c", "r"):
        for _w in (4, 5, 6, 8):
            for _u in (True, False):
                _e = _off({STRIDED: "1"}, _u)
                if _t == DOUBLE and _v == "c" and _u and UNITS[_w] != 0:
                    _e[NO_WIDE] = "1"
                _case(f"groups_{_s}_s{_w}{_v}" + ("" if _u else "_nouni"), f"s{_w}{_v}", _t,
                      loop(_t, UNITS[_w], True, _v == "r", _u, groups=True), env=_e, also_plain=(_w == 5 and _u))
    # C. a workgroup per reduction chunk (1075 chunks; HIPK_SPMV_SELL_STRIDED unset: the chunk walk below 16 / 32 tiles per chunk)
    #    value planes, and pair codes of a width the pair kernel does not have: loop<T,UNITS,true,VALS,UNI>
    for _w in (4, 5, 6, 8):
        for _u in (True, False):
            _case(f"chunk_{_s}_b{_w}r" + ("" if _u else "_nouni"), f"b{_w}r", _t, loop(_t, UNITS[_w], True, True, _u), env=_off({}, _u),
                  also_plain=(_w == 5 and _u))
    for _u in (True, False):
        _case(f"chunk_{_s}_b6c" + ("" if _u else "_nouni"), "b6c", _t, loop(_t, 0, True, False, _u), env=_off({}, _u))
    #    pair codes, UNITS 4 | 5 | 8: the pair kernel -- fp32; fp64 without uniform words; fp64 with HIPK_SPMV_SELL_NO_WIDE
    for _w in (4, 5, 8):
        if _t == FLOAT:
            for _u in (True, False):
                _case(f"pair_f32_b{_w}c" + ("" if _u else "_nouni"), f"b{_w}c", _t, pair(_t, UNITS[_w], _u), env=_off({}, _u),
                      also_plain=(_w == 5 and _u))
        else:
            _case(f"pair_f64_b{_w}c_nouni", f"b{_w}c", _t, pair(_t, UNITS[_w], False), env={UNIFORM: "0"})
            _case(f"pair_f64_b{_w}c_nowide", f"b{_w}c", _t, pair(_t, UNITS[_w], True), env={NO_WIDE: "1"}, runs=RUNS_WX, also_plain=(_w == 5))
    # D. outside the sliced-ELL forms
    _case(f"codedcsr_{_s}_s5c", "s5c", _t, same(f"hipk_spmv_coded_kernel<{_t},1>"), env={LAYOUT: "csr"}, also_plain=True)
    _case(f"rowwave_{_s}_d50c", "d50c", _t, same(f"hipk_spmv_rowwave_kernel<{_t}>"))
    _case(f"plain_{_s}_l41c", "l41c", _t, same("hipk_spmv_kernel<double,1280,false>" if _t == DOUBLE else "hipk_spmv_kernel<float,2048,false>"))

# the plain tile kernels by entries per 256-row tile (set_path(plain_only=True)): 1280 (inclusive), 1536, 2048 (inclusive), 2304
for _w, _n64, _n32 in ((5, "double,1280,true", "float,2048,true"), (6, "double,2048,true", "float,2048,true"),
                       (8, "double,2048,true", "float,2048,true"), (9, "double,1280,false", "float,2048,false")):
    _case(f"plain_f64_s{_w}c", f"s{_w}c", DOUBLE, same(f"hipk_spmv_kernel<{_n64}>"), plain_only=True)
    _case(f"plain_f32_s{_w}c", f"s{_w}c", FLOAT, same(f"hipk_spmv_kernel<{_n32}>"), plain_only=True)

# E. the two-rows-per-lane kernel (fp64, pair codes, UNITS 4 | 5 | 8, half of the tiles uniform): WALK = 1 forced at both sizes,
#    WALK = 0 where a workgroup takes a chunk; rows of 3 and 7 entries round to 4 and 8 units
for _w in (3, 4, 5, 7, 8):
    _case(f"wide_s{_w}c_walk1", f"s{_w}c", DOUBLE, wide(UNITS[_w], 1), env={STRIDED: "1"}, runs=RUNS_WX)
    for _walk in (0, 1):
        _case(f"wide_b{_w}c_walk{_walk}", f"b{_w}c", DOUBLE, wide(UNITS[_w], _walk), env={STRIDED: str(_walk)}, runs=RUNS_WX,
              also_plain=(_w == 5 and _walk == 0))

# F. switches that a process reads once (static const in hipk_launch_spmv): one child process per setting
for _w in (4, 5, 8):       # run-time mode bits: all eight modes on the MODE = -1 kernels
    for _walk in (0, 1):
        _case(f"nomode_wide_b{_w}c_walk{_walk}", f"b{_w}c", DOUBLE, wide(UNITS[_w], _walk, no_mode=True),
              env={NO_MODE: "1", STRIDED: str(_walk)}, fresh="no_mode", runs=RUNS_WX)
_case("nomode_pair_f64_b5c_nowide", "b5c", DOUBLE, pair(DOUBLE, 5, True, no_mode=True), env={NO_MODE: "1", NO_WIDE: "1"}, fresh="no_mode",
      runs=RUNS_WX)
_case("nomode_pair_f64_b5c_nouni", "b5c", DOUBLE, pair(DOUBLE, 5, False, no_mode=True), env={NO_MODE: "1", UNIFORM: "0"}, fresh="no_mode")
for _w in (4, 5, 8):       # where the pair kernel would run: the one-tile-per-trip chunk kernel
    for _u in (True, False):
        _case(f"nopair_f32_b{_w}c" + ("" if _u else "_nouni"), f"b{_w}c", FLOAT, loop(FLOAT, UNITS[_w], True, False, _u),
              env=_off({NO_PAIR: "1"}, _u), fresh="no_pair")
    _case(f"nopair_f64_b{_w}c_nouni", f"b{_w}c", DOUBLE, loop(DOUBLE, UNITS[_w], True, False, False), env={NO_PAIR: "1", UNIFORM: "0"},
          fresh="no_pair")
    _case(f"nopair_f64_b{_w}c_nowide", f"b{_w}c", DOUBLE, loop(DOUBLE, UNITS[_w], True, False, True), env={NO_PAIR: "1", NO_WIDE: "1"},
          fresh="no_pair")
# no plan cache: ONE handle, the per-launch switches flipped between launches; note and bits follow
_case("noplan_f64_b5c", "b5c", DOUBLE, None, env={NO_PLAN: "1"}, fresh="no_plan_cache", runs=RUNS_WX,
      steps=[({STRIDED: "0"}, wide(5, 0)), ({STRIDED: "1"}, wide(5, 1)), ({NO_WIDE: "1"}, loop(DOUBLE, 5, True, False, True, groups=True)),
             ({STRIDED: "0"}, pair(DOUBLE, 5, True)), ({NO_WIDE: None}, wide(5, 0)), ({STRIDED: None}, wide(5, 0))])
# HIPK_SPMV_SELL_CHUNKED=0 (whether it is set at all is read once per process): the persistent walk at a size that would take a
# workgroup per chunk, also where the wide kernel would run
_case("chunked0_f64_b5c", "b5c", DOUBLE, loop(DOUBLE, 5, False, False, True), env={CHUNKED: "0"}, fresh="chunked0")
_case("chunked0_f32_b5r", "b5r", FLOAT, loop(FLOAT, 5, False, True, True), env={CHUNKED: "0"}, fresh="chunked0")
_case("chunked0_f64_b8r_strided", "b8r", DOUBLE, loop(DOUBLE, 8, False, True, True), env={CHUNKED: "0", STRIDED: "1"}, fresh="chunked0")

FRESH_GROUPS = sorted({c["fresh"] for c in CASES.values() if c["fresh"]})

# Instantiations that no input can reach: {name as the completeness check normalises it: the condition in hipk_launch_spmv that
# excludes it}.  At most 8 of the 128 may stand here.
UNREACHABLE = {}
UNREACHABLE_CAP = 8


def expected_notes():
    """Every note the table expects, "/groups" stripped: the instantiations it accounts for."""
    out = set()
    for c in CASES.values():
        for _, notes in c["steps"]:
            for mode, _wx in c["runs"]:
                out.add(notes[mode].replace("/groups", ""))
    return out
