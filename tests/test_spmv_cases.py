"""The case table of tests/test_gpu_spmv_instantiations.py (tests/_spmv_cases.py), checked without a GPU: it accounts for every
hipk_spmv_* kernel of the gfx950 code object of csrc/hipk_api.hip (the compiler's own kernel list), names nothing that does not
exist, stays in range, keeps the switches a process reads once in child processes, and names for every generated matrix the
template arguments that its structure gives (tile widths, pair count, uniform tiles -- recomputed in numpy).  The references the
GPU test compares with are held against np.longdouble here as well, at the small size."""
import os
import re
import shutil

import numpy as np
import pytest

import _spmv_cases as C
from test_chebyshev_kernel_resources import CHEB
from test_kernel_resources import HIPCC, _vgprs
from test_switch_table import _rows

needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("c++filt") is None, reason="hipcc / c++filt not installed")


def _norm(name):
    return name.replace("void ", "").replace(" ", "")


@pytest.fixture(scope="module")
def kernels():
    """The hipk_spmv_* kernels of hipk_api.hip's code object, 'void ' and spaces dropped."""
    return sorted(k for k in map(_norm, _vgprs("hipk_api.hip")) if k.startswith("hipk_spmv_"))


def orphans(kernels, expected):
    """The instantiations no case expects, that are not declared unreachable and not the Chebyshev tests'."""
    cheb = {_norm(k) for k in CHEB}
    return [k for k in kernels if k not in expected and k not in C.UNREACHABLE and k not in cheb]


@needs_hipcc
def test_every_instantiation_is_some_cases_expected_note(kernels):
    assert len(kernels) == 128, len(kernels)
    cheb = {_norm(k) for k in CHEB if _norm(k).startswith("hipk_spmv_")}
    assert len(cheb) == 9 and cheb <= set(kernels)
    left = orphans(kernels, C.expected_notes())
    assert not left, f"{len(left)} SpMV instantiations that no case of tests/_spmv_cases.py runs: {left}"
    assert len(C.UNREACHABLE) <= C.UNREACHABLE_CAP == 8
    for k, reason in C.UNREACHABLE.items():
        assert k in kernels and k not in C.expected_notes() and "hipk_launch_spmv" in reason, k


@needs_hipcc
def test_a_deleted_case_orphans_its_instantiation(kernels):
    """The completeness check goes red when it should: without the only case of an instantiation it names that instantiation."""
    for gone, kernel in (("rowwave_f32_d50c", "hipk_spmv_rowwave_kernel<float>"),
                         ("pair_f32_b8c_nouni", "hipk_spmv_sell_pair_kernel<float,8,false,-1>")):
        saved = C.CASES.pop(gone)
        try:
            assert orphans(kernels, C.expected_notes()) == [kernel]
        finally:
            C.CASES[gone] = saved
    assert orphans(kernels, C.expected_notes()) == []


@needs_hipcc
def test_every_expected_note_names_an_instantiation_that_exists(kernels):
    missing = sorted(C.expected_notes() - set(kernels))
    assert not missing, missing


def test_sizes_offsets_and_modes_are_in_range():
    for name, (n, offsets, kind) in C.MATRICES.items():
        assert 1 <= n < 2 ** 22 and kind in ("c", "r"), name               # one chunk size (2048 rows) for every case
        assert offsets == sorted(set(offsets)) and 0 in offsets and 1 <= len(offsets) <= 64, name
        assert max(abs(o) for o in offsets) < min(n, 2 ** 15), name
    for name, c in C.CASES.items():
        assert c["matrix"] in C.MATRICES and c["dtype"] in (C.DOUBLE, C.FLOAT), name
        assert c["runs"] and all(m in C.MODES and isinstance(wx, bool) and (not wx or m == 1) for m, wx in c["runs"]), name
        assert c["steps"], name
        for delta, notes in c["steps"]:
            assert set(notes) == set(C.MODES) and all(isinstance(v, str) and len(v) < 96 for v in notes.values()), name
            assert all(v is None or isinstance(v, str) for v in delta.values()), name
        assert not (c["plain_only"] and c["also_plain"]), name
    assert len({(c["matrix"], c["dtype"]) for c in C.CASES.values() if c["also_plain"]}) >= 6      # one per family at least


def test_switches_are_rows_and_process_wide_ones_run_in_a_child():
    rows = {r[0]: r for r in _rows()}
    once = {name for name, r in rows.items() if "of the process" in r[3]}
    assert {C.NO_MODE, C.NO_PAIR, C.NO_PLAN, C.CHUNKED} <= once
    for name, c in C.CASES.items():
        used = set(c["env"]) | {k for delta, _ in c["steps"] for k in delta}
        assert used <= set(rows), (name, used - set(rows))
        assert all(k.startswith("HIPK_") for k in used)
        if used & once:
            assert c["fresh"] is not None, f"{name} sets {sorted(used & once)}, read once per process, but runs in the test process"
            assert not {k for delta, _ in c["steps"] for k in delta} & once, name
    for group in C.FRESH_GROUPS:          # one setting per child
        settings = {tuple(sorted((k, v) for k, v in c["env"].items() if k in once)) for c in C.CASES.values() if c["fresh"] == group}
        assert len(settings) == 1 and settings != {()}, (group, settings)


def _keys(crow, col, val):
    """What the dispatch keys on: the longest row, the common tile width in units (None: the tiles keep different widths), the number
    of distinct (offset, value) pairs, the share of FULL tiles whose rows all carry the same offsets (and values, for pair codes)."""
    n = len(crow) - 1
    lens = np.diff(crow)
    ntiles = (n + 255) // 256
    starts = np.arange(ntiles) * 256
    w = np.maximum.reduceat(lens, starts)
    units = 4 * (w // 4 + (w % 4 == 3)) + np.where(w % 4 == 3, 0, w % 4)         # hipk_sell_units
    planes, wmax = int(units.sum()), int(units.max())
    common = wmax if (units.min() == wmax or ntiles * wmax <= planes + planes // 50 + 8) else None
    rows = np.repeat(np.arange(n), lens)
    off = col - rows
    pairs = len(np.unique(np.stack([off, val.view(np.int64)]), axis=1).T) if len(val) <= 4_000_000 else None
    full = n // 256
    same_len = lens[:full * 256].reshape(full, 256)
    uniform_off = int((same_len.min(axis=1) == same_len.max(axis=1)).sum())    # a band: equal lengths = equal offsets, but for
    return dict(max_row=int(lens.max()), max_tile=int(np.add.reduceat(lens, starts).max()), common=common, pairs=pairs,   # the ends
                uniform=uniform_off / ntiles, mean=len(col) // n)


@pytest.mark.parametrize("name", sorted(C.MATRICES))
def test_matrices_give_the_template_arguments_the_notes_name(name):
    n, offsets, kind = C.MATRICES[name]
    crow, col, val = C.matrix(name)
    k = _keys(crow, col, val)
    print(name, k)
    width = len(offsets)
    assert k["max_row"] == width and len(crow) == n + 1
    if name == "d50c":
        assert k["mean"] >= 48                                       # hipk_launch_spmv: rowwave = nnz / n_rows >= 48
        return
    assert k["mean"] < 48
    if name == "l41c":
        assert k["max_row"] > 32                                     # HIPK_LONG_ROW: no coded form, the general tile kernel
        return
    if kind == "c":
        assert k["pairs"] is None or k["pairs"] == width             # <= 255: pair codes
        assert len(np.unique(val)) == len(np.unique(val.astype(np.float32))) == width      # also in fp32 storage
    elif k["pairs"] is not None:
        assert k["pairs"] > 4096                                     # the dictionary overflows: offsets only + value planes
    units = 4 * (width // 4 + (width % 4 == 3)) + (0 if width % 4 == 3 else width % 4)
    assert k["common"] == units and C.UNITS[width] == (units if units in (4, 5, 8) else 0)
    assert k["max_tile"] == 256 * width
    # uniform words: tiles of at most two groups of four codes (8 units); kept from a quarter of the tiles, the wide kernel from half
    assert k["uniform"] >= 0.9
    for cname, c in C.CASES.items():
        if c["matrix"] != name:
            continue
        for _, notes in c["steps"]:
            for note in set(notes.values()):
                m = re.match(r"hipk_spmv_sell_(loop|pair|wide)_kernel<(.*)>", note)
                if not m:
                    continue
                a = m.group(2).split(",")
                got_units = int(a[0]) if m.group(1) == "wide" else int(a[1])
                assert got_units == C.UNITS[width], (cname, note)
                if m.group(1) == "loop":
                    assert a[3] == ("true" if kind == "r" else "false"), (cname, note)
                uni = {"loop": a[4:5], "pair": a[2:3], "wide": ["true"]}[m.group(1)][0] == "true"
                assert uni == (units <= 8 and c["env"].get(C.UNIFORM) != "0"), (cname, note)
                if m.group(1) != "loop":
                    assert kind == "c" and units in (4, 5, 8), (cname, note)
                if m.group(1) != "wide":
                    assert a[0] == c["dtype"], (cname, note)


@pytest.mark.parametrize("name,dtype", [("s5c", C.DOUBLE), ("s8r", C.DOUBLE), ("s5r", C.FLOAT), ("s11c", C.FLOAT), ("d50c", C.DOUBLE)])
def test_references_stay_within_the_derived_bound_of_high_precision(oracle, name, dtype):
    from _spmv_inst_worker import References
    n = C.MATRICES[name][0]
    ch, g = oracle.chunk_geom(n)
    assert ch == 2048
    ref = References(oracle, name, dtype, ch)
    assert all(len(p) == g for p in list(ref.part0.values()) + list(ref.part1.values()))
    worst = ref.check_against_high_precision()
    print(f"{name} {dtype}: largest error / bound {worst:.3f}")
    assert 0.0 < worst <= 1.0
    # the bound bites: y of the residual form moved by two units in the last place of its largest term is outside it
    ref.y[True] = ref.y[True] + np.abs(ref.b).astype(ref.f) * ref.f(8 * (2.0 ** -53 if dtype == C.DOUBLE else 2.0 ** -24) * 64)
    with pytest.raises(AssertionError):
        ref.check_against_high_precision()
