"""The transformations and case tables of tests/_order_cases.py (unsorted and duplicate CSR rows), checked without a GPU: every
transformed matrix really is unsorted / carries repeated columns, keeps the entries of its base, and has the row length, tile
width, pair count, uniform tiles, entries per tile, chunk count and window that its expected kernel note or solve form implies
(recomputed in numpy; the checks of tests/test_spmv_cases.py and tests/test_form_cases.py on the transformed arrays); the SpMV
and Chebyshev tables name every kernel template that tests/_spmv_cases.py and tests/_cheb_cases.py name, the solver table every
form family of the library, and removing the only case of one names it."""
import re

import numpy as np
import pytest
import scipy.sparse as sp

import _form_cases as FC
import _order_cases as OC
import _spmv_cases as S
from test_form_cases import _implied
from test_switch_table import _rows as switch_rows


# ---------------------------------------------------------------------------------------------- the transformations
def _small():
    M = OC._band(1000, (1, 2, 7))
    return M.indptr.astype(np.int64), M.indices.astype(np.int64), M.data.copy()


def _dense_of(crow, col, val):
    n = len(crow) - 1
    D = np.zeros((n, n), dtype=np.longdouble)
    np.add.at(D, (OC._rows(crow), col), val.astype(np.longdouble))
    return D


@pytest.mark.parametrize("name", sorted(OC.TRANSFORMS))
def test_transformation_keeps_the_entries_and_does_what_its_name_says(name):
    crow, col, val = _small()
    c2, j2, v2 = OC.TRANSFORMS[name](crow, col, val, seed=3)
    again = OC.TRANSFORMS[name](crow, col, val, seed=3)
    assert all(np.array_equal(a, b) for a, b in zip((c2, j2, v2), again))            # seeded
    n, lens, lens2 = len(crow) - 1, np.diff(crow), np.diff(c2)
    assert c2[0] == 0 and c2[-1] == len(j2) == len(v2) and c2.dtype == crow.dtype and j2.dtype == col.dtype and v2.dtype == val.dtype
    grow = 1 if name in OC.GROWS else 0
    assert np.array_equal(lens2, lens + grow)
    # the same matrix as a sum of entries: exactly for the permutations and the stored zero, to one rounding of v - 0.25 v else
    D, D2 = _dense_of(crow, col, val), _dense_of(c2, j2, v2)
    if name in OC.DUPLICATED:
        assert np.all(np.abs(D2 - D) <= 2.0 ** -53 * np.abs(D)) and np.array_equal(D2 != 0, D != 0)
    else:
        assert np.array_equal(D2, D)
    rows2 = OC._rows(c2)
    if name == "rev":
        assert all(np.array_equal(j2[c2[r]:c2[r + 1]], col[crow[r]:crow[r + 1]][::-1]) for r in range(n))
    if name == "diag_first":
        assert np.array_equal(j2[c2[:-1]], np.arange(n))
        assert all(np.all(np.diff(j2[c2[r] + 1:c2[r + 1]]) > 0) for r in range(n))
    if name in ("dup", "dup_diag", "dup_shuf"):
        assert OC.has_repeat(c2, j2).all()
        quarter = np.isin(v2, 0.25 * val)
        assert quarter.sum() >= n
    if name == "dup_diag":
        assert np.array_equal(np.bincount(rows2[j2 == rows2], minlength=n), np.full(n, 2))
    if name == "dup":
        assert not OC.descents(c2, j2).any()                                         # the two halves are adjacent, in place
    if name == "dup_shuf":
        adjacent = (j2[1:] == j2[:-1]) & (rows2[1:] == rows2[:-1])
        assert np.bincount(rows2[1:][adjacent], minlength=n).astype(bool).mean() < 0.6   # the halves are in general apart
    if name == "zero":
        last = c2[1:] - 1
        assert np.all(v2[last] == 0.0) and np.all(np.signbit(v2[last]) == False) and OC.has_repeat(c2, j2).all()  # noqa: E712
    if name == "shuf":
        orders = {tuple(np.argsort(j2[c2[r]:c2[r + 1]], kind="stable")) for r in range(300, 556)}
        assert len(orders) > 100                                                     # the rows of a tile do not share an order


def _used():
    """Every (kind, matrix, transformation) some table uses; the 2.2 M-row ones are checked with their structure, further down."""
    out = {("spmv", c["matrix"], c["transform"]) for c in OC.SPMV.values() if OC.base_rows(c["matrix"]) <= S.N_SMALL}
    out |= {("cheb", c[0], c[1]) for c in OC.CHEB.values()}
    out |= {("solve", c[2], c[3]) for c in OC.SOLVES}
    return sorted(out)


def _load(kind, matrix, transform):
    if kind == "spmv":
        return OC.arrays(matrix, transform, OC.DOUBLE)
    if kind == "cheb":
        import _cheb_cases as CC
        crow, col, val, _ = CC.band(OC.N_CHEB, OC.CHEB_OFFSETS[matrix])
        return OC.TRANSFORMS[transform](crow, col, val, seed=len(matrix))
    return OC.solver_matrix(matrix, transform, np.float64)


@pytest.mark.parametrize("kind, matrix, transform", _used(), ids=["-".join(u) for u in _used()])
def test_the_matrices_under_test_are_unsorted_or_duplicated(kind, matrix, transform):
    _unsorted_or_duplicated(*_load(kind, matrix, transform), matrix, transform)


def _unsorted_or_duplicated(crow, col, val, matrix, transform):
    n, lens = len(crow) - 1, np.diff(crow)
    assert col.min() >= 0 and col.max() < n and np.all(lens >= 0) and crow[-1] == len(col)
    starts = np.arange(0, n, 256)
    if transform in OC.UNSORTED:
        down = OC.descents(crow, col)
        assert down[lens >= 2].mean() >= 0.5, (matrix, transform, down[lens >= 2].mean())
        assert np.add.reduceat(down.astype(np.int64), starts).min() >= 1          # every 256-row tile contains one
    if transform in OC.DUPLICATED:
        assert OC.has_repeat(crow, col)[lens > 0].all()
    if transform == "zero":
        assert (np.add.reduceat((val == 0.0).astype(np.int64), crow[:-1])[lens > 0] == 1).all()


# ---------------------------------------------------------------------------------------------- SpMV sweep: dispatch properties
def keys(crow, col, val, offsets_only):
    """What hipk_build_coded and hipk_launch_spmv key on, from the arrays alone: the longest row, the mean row (integer division),
    the most entries in a 256-row tile, the common tile width in units (None: different widths), the number of distinct
    (offset, value) pairs, and the share of tiles whose 256 rows carry the same codes in the same storage positions -- codes of
    (offset, value) pairs, or of offsets alone for the offset-coded form."""
    n = len(crow) - 1
    lens = np.diff(crow)
    ntiles = (n + 255) // 256
    starts = np.arange(ntiles) * 256
    w = np.maximum.reduceat(lens, starts)
    units = 4 * (w // 4 + (w % 4 == 3)) + np.where(w % 4 == 3, 0, w % 4)                 # hipk_sell_units
    planes, wmax = int(units.sum()), int(units.max())
    common = wmax if (units.min() == wmax or ntiles * wmax <= planes + planes // 50 + 8) else None
    rows = OC._rows(crow)
    uo, oi = np.unique(col - rows, return_inverse=True)
    uv, vi = np.unique(np.ascontiguousarray(val).view(np.int64 if val.dtype == np.float64 else np.int32), return_inverse=True)
    pair_ids = np.unique(oi.astype(np.int64) * len(uv) + vi, return_inverse=True)
    pairs = len(pair_ids[0])
    ids = oi.astype(np.uint64) if offsets_only else pair_ids[1].astype(np.uint64)
    pos = (np.arange(len(col)) - crow[:-1][rows]).astype(np.uint64)
    term = (ids + np.uint64(1)) * np.power(np.uint64(1_000_003), pos)                  # a row's codes by position (a hash: wraps)
    sig = np.zeros(n, dtype=np.uint64)
    sig[lens > 0] = np.add.reduceat(term, crow[:-1][lens > 0])
    full = n // 256
    s = sig[:full * 256].reshape(full, 256)
    uniform = int((s.min(axis=1) == s.max(axis=1)).sum()) / ntiles
    return dict(max_row=int(lens.max()), mean=len(col) // n, max_tile=int(np.add.reduceat(lens, starts).max()), common=common, pairs=pairs,
                uniform=uniform, n=n, ragged=float((np.minimum.reduceat(lens, starts) < w).mean()))


_keys_of = {}


HEAD = 300 * 256      # rows of a 2.2 M-row band whose codes are looked at: 300 tiles, the band's structure repeats


def _case_keys(case):
    k = (case["matrix"], case["transform"], case["dtype"])
    if k not in _keys_of:
        crow, col, val = OC.arrays(*k)
        whole = None
        if len(crow) - 1 > S.N_SMALL:       # row lengths of the whole matrix; pairs and uniform tiles of its leading 300 tiles
            if (k[0], k[1]) not in _checked_big:
                _unsorted_or_duplicated(crow, col, val, k[0], k[1])
                _checked_big.add((k[0], k[1]))
            lens, n = np.diff(crow), len(crow) - 1
            starts = np.arange(0, n, 256)
            w = np.maximum.reduceat(lens, starts)
            units = 4 * (w // 4 + (w % 4 == 3)) + np.where(w % 4 == 3, 0, w % 4)
            planes, wmax = int(units.sum()), int(units.max())     # hipk_build_coded: nearly equal widths are padded to the largest
            whole = dict(max_row=int(lens.max()), mean=len(col) // n, max_tile=int(np.add.reduceat(lens, starts).max()), n=n,
                         common=wmax if (units.min() == wmax or len(w) * wmax <= planes + planes // 50 + 8) else None)
            crow, col, val = crow[:HEAD + 1], col[:crow[HEAD]], val[:crow[HEAD]]
        pairs_fit = keys(crow, col, val, False)
        _keys_of[k] = pairs_fit if pairs_fit["pairs"] <= 256 else dict(keys(crow, col, val, True), pairs=pairs_fit["pairs"])
        if whole:                           # (of the leading tiles the first few are narrower: the band's far offsets start later)
            _keys_of[k].update(whole)
    return _keys_of[k]


_checked_big = set()


def _base_width(matrix):
    return 11 if matrix == OC.RAGGED else len(S.MATRICES[matrix][1])


@pytest.mark.parametrize("name", sorted(OC.SPMV))
def test_spmv_case_has_the_structure_its_expected_note_implies(name):
    c = OC.SPMV[name]
    k = _case_keys(c)
    print(name, k)
    t, env, grows = c["transform"], c["env"], c["transform"] in OC.GROWS
    width = _base_width(c["matrix"]) + (1 if grows else 0)
    assert k["max_row"] == width and k["n"] == OC.base_rows(c["matrix"])
    assert c["runs"] == S.RUNS_WX and len(c["steps"]) == 1 and not (c["plain_only"] and c["also_plain"])
    note = c["steps"][0][1]
    assert set(note) == set(S.MODES)
    # a seeded order per row leaves no tile uniform; the same rearrangement in every row keeps a band's
    if c["matrix"] != OC.RAGGED and k["max_row"] <= 32 and k["mean"] < 48:
        assert (k["uniform"] >= 0.9) if t in OC.SAME_IN_EVERY_ROW else (k["uniform"] < 0.01), (name, k["uniform"])
    kind_r = c["matrix"] != OC.RAGGED and S.MATRICES[c["matrix"]][2] == "r"
    assert (k["pairs"] > 4096) if kind_r else (k["pairs"] <= 3 * width <= 255), (name, k["pairs"])
    f64 = c["dtype"] == OC.DOUBLE
    plain = ("hipk_spmv_kernel<double,1280,true>" if f64 and k["max_tile"] <= 1280 and width <= 32 else
             ("hipk_spmv_kernel<double,2048,true>" if f64 else "hipk_spmv_kernel<float,2048,true>") if k["max_tile"] <= 2048 and width <= 32 else
             "hipk_spmv_kernel<double,1280,false>" if f64 else "hipk_spmv_kernel<float,2048,false>")
    one = set(note.values())
    if k["mean"] >= 48:                                      # hipk_launch_spmv: rowwave = nnz / n_rows >= 48
        assert one == {f"hipk_spmv_rowwave_kernel<{c['dtype']}>"}
        return
    if width > 32 or c["plain_only"]:                        # HIPK_LONG_ROW: no coded form; or set_path(plain_only=True)
        assert one == {plain}, (name, plain)
        assert c["plain_only"]
        return
    if env.get(OC.LAYOUT) == "csr":                          # hipk_build_coded: want_sell = OFFS_ONLY || !lay_csr; pair codes fit
        assert one == {f"hipk_spmv_coded_kernel<{c['dtype']},1>"} and k["pairs"] <= 256 and k["ragged"] >= 0.9
        return
    units = k["common"]
    assert units is not None
    want_units = units if units in (4, 5, 8) else 0
    uni = k["uniform"] >= 0.25 and units <= 8 and env.get(S.UNIFORM) != "0"
    wide_ok = f64 and uni and k["uniform"] >= 0.5 and not kind_r and units in (4, 5, 8) and S.NO_WIDE not in env
    big = k["n"] == S.N_BIG
    assert k["n"] in (S.N_SMALL, S.N_BIG)
    strided = env.get(OC.STRIDED)
    assert strided in (None, "0", "1") and not (big and strided == "1") and not (not big and strided == "0")
    no_mode = OC.NO_MODE in env
    if wide_ok and (big or strided == "1"):
        want = S.wide(want_units, 0 if big else 1, no_mode=no_mode)
    elif strided == "1":
        want = S.loop(c["dtype"], want_units, True, kind_r, uni, groups=True)
    elif big and not kind_r and units in (4, 5, 8):
        want = S.pair(c["dtype"], want_units, uni, no_mode=no_mode)
    else:
        want = S.loop(c["dtype"], want_units, big, kind_r, uni)
    assert note == want, (name, note[1], want[1])
    if no_mode:
        assert c["fresh"] == "no_mode"


def test_spmv_table_covers_what_the_issue_asks_for():
    by = OC.SPMV
    assert len(OC.BIG_CASES) <= 8
    for n in OC.BIG_CASES:       # only families that need a workgroup per chunk run at 2.2 M rows
        assert re.match(r"hipk_spmv_sell_(pair_kernel<|wide_kernel<\d,-?\d,0>|loop_kernel<\w+,\d,true,\w+,\w+>$)", by[n]["steps"][0][1][0]), n
    assert {c["dtype"] for c in by.values()} == {OC.DOUBLE, OC.FLOAT}
    assert {c["transform"] for c in by.values()} == set(OC.TRANSFORMS)
    for m in ("l41c", "d50c", OC.RAGGED):
        assert {c["dtype"] for c in by.values() if c["matrix"] == m} == {OC.DOUBLE, OC.FLOAT}, m
    assert all(c["env"].get(OC.LAYOUT) == "csr" for c in by.values() if c["matrix"] == OC.RAGGED)
    i32 = [n for n, c in by.items() if c["idx32"]]
    assert len(i32) >= 6 and all(by[n[:-4]]["steps"] == by[n]["steps"] and not by[n[:-4]]["idx32"] for n in i32)
    assert len([n for n in OC.SOLVES_I32 if n in {c[0] for c in OC.SOLVES}]) == len(OC.SOLVES_I32) >= 3
    # w == x on the two-rows-per-lane kernel with the diagonal stored first, last, and twice
    wide = {c["transform"] for c in by.values() if "sell_wide" in c["steps"][0][1][0]}
    assert {"diag_first", "rev", "dup_diag"} <= wide


def test_switches_are_rows_and_process_wide_ones_run_in_a_child():
    rows = {r[0]: r for r in switch_rows()}
    once = {name for name, r in rows.items() if "of the process" in r[3]}
    for name, c in OC.SPMV.items():
        used = set(c["env"])
        assert used <= set(rows), (name, used - set(rows))
        assert bool(used & once) == (c["fresh"] is not None), name
        assert all("test" in rows[k][5] for k in used), (name, [k for k in used if "test" not in rows[k][5]])
    for cid, solver, key, tr, dtn, kw, env, x0, path, form in OC.SOLVES:
        assert set(env) <= set(rows) and not set(env) & once, cid
        assert all("test" in rows[k][5] for k in env), (cid, [k for k in env if "test" not in rows[k][5]])
    for c in OC.CHEB.values():
        assert set(c[3]) <= set(rows) and not set(c[3]) & once


# ---------------------------------------------------------------------------------------------- Chebyshev table
@pytest.mark.parametrize("name", sorted(OC.CHEB))
def test_cheb_case_has_the_structure_its_expected_note_implies(name):
    matrix, transform, dtype, env, plain_only, note = OC.CHEB[name]
    crow, col, val = _load("cheb", matrix, transform)
    k = keys(crow, col, val.astype(np.float64 if dtype == OC.DOUBLE else np.float32), False)
    width = len(OC.CHEB_OFFSETS[matrix]) + (1 if transform in OC.GROWS else 0)
    assert k["max_row"] == width and k["pairs"] <= 3 * width and k["max_tile"] == 256 * width
    f64 = dtype == OC.DOUBLE
    if plain_only:          # hipk_launch_spmv: cap = (f64 && max_tile_nnz <= 1280) ? 1280 : 2048, none above 2048
        assert not env and k["max_tile"] <= 2048
        assert note == f"hipk_spmv_cheb_kernel<{dtype},{1280 if f64 and k['max_tile'] <= 1280 else 2048}>"
        return
    assert f64 and env == {OC.STRIDED: "1"} and k["common"] in (4, 5, 8)
    if transform in OC.SAME_IN_EVERY_ROW:
        assert k["uniform"] >= 0.9 and note == f"hipk_spmv_sell_wide_kernel<{k['common']},28,1>"
    else:                   # no uniform tile: the one-row-per-lane coded kernels, which have no epilogue
        assert k["uniform"] < 0.01 and note == S.loop(dtype, k["common"], True, False, False, groups=True)[0] + OC.STEP64


def test_cheb_table_has_a_case_per_epilogue_family_under_both_orders():
    fam = {}
    for matrix, transform, dtype, env, plain_only, note in OC.CHEB.values():
        fam.setdefault(note.split("<")[0], set()).add(transform)
    assert fam["hipk_spmv_cheb_kernel"] >= {"diag_first", "dup_shuf"}
    assert fam["hipk_spmv_sell_wide_kernel"] >= {"diag_first", "dup_diag"}
    notes = {c[5] for c in OC.CHEB.values()}
    assert {"hipk_spmv_cheb_kernel<double,1280>", "hipk_spmv_cheb_kernel<double,2048>", "hipk_spmv_cheb_kernel<float,2048>"} <= notes


# ---------------------------------------------------------------------------------------------- coverage of the kernel templates
def _named_templates():
    """Every kernel template that tests/_spmv_cases.py: CASES and tests/_cheb_cases.py name."""
    import _cheb_cases as CC
    notes = set(S.expected_notes())
    notes |= {n for c in S.CASES.values() for _, by in c["steps"] for n in by.values()}       # with "/groups"
    for b in CC.BANDS.values():
        for n in (b["wide"] or ()) + (b["plain"],):
            notes |= {n, CC.two_launches(n)}
    for g in CC.GRIDS.values():
        notes |= set(g[4])
    notes |= {CC.SMALL_WIDE, CC.two_launches(CC.SMALL_WIDE)} | set(CC.POISSON_SIZES.values()) | {s[6] for s in CC.SOLVES.values()}
    notes |= {"hipk_spmv_cheb_kernel<float,2048>", "hipk_spmv_kernel<float,2048,true>" + CC.STEP32}   # test_apply_fp32_plain_ragged
    return OC.spmv_templates(notes)


def missing_templates(spmv=None, cheb=None):
    return sorted(_named_templates() - OC.spmv_templates(OC.sweep_notes(spmv, cheb)) - set(OC.UNREACHABLE_UNSORTED))


def test_every_kernel_template_is_some_cases_expected_note():
    named = _named_templates()
    assert {"hipk_spmv_sell_loop_kernel", "hipk_spmv_sell_loop_kernel/groups", "hipk_spmv_sell_pair_kernel", "hipk_spmv_sell_wide_kernel",
            "hipk_spmv_coded_kernel", "hipk_spmv_rowwave_kernel", "hipk_spmv_kernel", "hipk_spmv_cheb_kernel", "hipk_cheb_step_kernel"} == named
    assert missing_templates() == []
    for k, reason in OC.UNREACHABLE_UNSORTED.items():
        assert reason and k not in OC.spmv_templates(OC.sweep_notes()) and k not in {OC.form_family(c[9]) for c in OC.SOLVES}


def test_removing_the_only_case_of_a_template_names_it():
    without = {n: c for n, c in OC.SPMV.items() if "rowwave" not in n}
    assert missing_templates(spmv=without) == ["hipk_spmv_rowwave_kernel"]
    without = {n: c for n, c in OC.SPMV.items() if not n.startswith("codedcsr_")}
    assert missing_templates(spmv=without) == ["hipk_spmv_coded_kernel"]
    without = {n: c for n, c in OC.CHEB.items() if not n.startswith("tile")}
    assert missing_templates(cheb=without) == ["hipk_spmv_cheb_kernel"]
    assert missing_templates(cheb={}) == ["hipk_cheb_step_kernel", "hipk_spmv_cheb_kernel"]


# ---------------------------------------------------------------------------------------------- solver sweep
def _forms():
    import torch  # noqa: F401  (HIP runtime first)
    from pytorch_sparse_solver import _hipk
    return _hipk.solve_forms()


def missing_families(solves):
    have = {OC.form_family(c[9]) for c in solves}
    return sorted({OC.form_family(f) for f in _forms()} - have - set(OC.UNREACHABLE_UNSORTED))


def test_every_form_family_has_a_case_and_every_expected_form_is_a_row():
    forms = _forms()
    fams = {OC.form_family(f) for f in forms}
    for want in ("hipk_cg_solve_lds_kernel LOCAL=true", "hipk_cg_solve_lds_kernel LOCAL=false", "hipk_bi_solve_lds_kernel LOCAL=true",
                 "hipk_bi_solve_lds_kernel LOCAL=false", "hipk_gm_solve_lds_kernel LOCAL=true", "hipk_gm_solve_lds_kernel LOCAL=false",
                 "hipk_gm_cycle_small_kernel", "hipk_cg_mid_kernel", "hipk_bi_mid_kernel", "hipk_gm_mid_kernel", FC.CG2_64, FC.CG2_32, FC.CG3S,
                 FC.CG3, FC.PCG3, FC.BI5S, FC.BI5, FC.BI5SJ, FC.BI5J, FC.GSW, FC.GLS, FC.GBIG):
        assert want in fams, want
    assert len(fams) == 24, sorted(fams)
    assert missing_families(OC.SOLVES) == []
    assert sorted({c[9] for c in OC.SOLVES} - set(forms)) == []
    # each family under rev and under dup_shuf -- but for the fp64 two-launch form, whose 1280-entry tile a duplicate overflows on the
    # 5-entry band: it runs duplicates on the rows-of-31 matrix
    by = {}
    for c in OC.SOLVES:
        by.setdefault(OC.form_family(c[9]), set()).add(c[3])
    assert all({"rev", "dup_shuf"} <= t for t in by.values()), {f: t for f, t in by.items() if not {"rev", "dup_shuf"} <= t}
    # Jacobi and callback M, fp32 storage per solver
    assert {c[1] for c in OC.SOLVES} == {"cg", "pcg", "bicgstab", "pbicgstab", "gmres", "pgmres"}
    for solver in ("cg", "bicgstab", "gmres"):
        assert any(c[4] == OC.F32 and c[1] in (solver, "p" + solver) for c in OC.SOLVES), solver
    assert {c[1] for c in OC.SOLVES if c[5].get("callback")} == {"pbicgstab", "pgmres"}
    for kernel in ("cg", "bi", "gm"):        # the mid loops: two row widths, with and without Jacobi
        mids = [c[9] for c in OC.SOLVES if c[9].startswith(f"hipk_{kernel}_mid_kernel<")]
        assert len({f.split(",")[1] for f in mids}) >= 2 and {f.rstrip(">").split(",")[-1] for f in mids} == {"true", "false"}, mids


def test_removing_the_only_case_of_a_form_family_names_it():
    assert missing_families([c for c in OC.SOLVES if not c[0].startswith("gmres-cycle-small-")]) == ["hipk_gm_cycle_small_kernel"]
    assert missing_families([c for c in OC.SOLVES if not c[0].startswith("gmres-small-256-")]) == [FC.GS256]
    assert missing_families([c for c in OC.SOLVES if c[9] != FC.CG2_32]) == [FC.CG2_32]


_props = {}


def _solver_props(key, transform):
    if (key, transform) not in _props:
        crow, col, val = OC.solver_matrix(key, transform, np.float64)
        n = len(crow) - 1
        _props[(key, transform)] = FC.matrix_props(sp.csr_matrix((val, col, crow), shape=(n, n)))
    return _props[(key, transform)]


@pytest.mark.parametrize("case", OC.SOLVES, ids=[c[0] for c in OC.SOLVES])
def test_solver_matrix_has_the_shape_the_expected_form_implies(case):
    cid, solver, key, tr, dtn, kw, env, x0, path, form = case
    p = _solver_props(key, tr)
    base = FC.matrix_props(OC.MATRICES[key]())
    grow = 1 if tr in OC.GROWS else 0
    assert (p["g"], p["W"], p["slots"], p["range"]) == (base["g"], base["W"] + grow, base["slots"], base["range"]), (cid, p, base)
    assert _implied((cid, solver, key, dtn, kw, env, x0, path, form), p) == [], cid
    assert path.split(" -> ")[-1] in (FC.LS, FC.CG_LDS, FC.BI_LDS, FC.GM_LDS, FC.GM_SMALL) or path == form, cid
    m = re.match(r"hipk_(cg|bi|gm)_mid_kernel<(double|float),(\d+),", form)
    if m:       # the register rows: the smallest of 5, 7, 9, 12 that holds the longest row
        assert int(m.group(3)) == min(w for w in (5, 7, 9, 12) if w >= p["W"]), (cid, p["W"])
        assert m.group(2) == ("double" if dtn == OC.F64 else "float")


def test_the_duplicate_moves_each_guard_edge_it_is_meant_to_move():
    def W(key, tr):
        return _solver_props(key, tr)["W"]
    by = {c[0]: c for c in OC.SOLVES}
    # kCgRowRegs = 12: 11 + 1 stays in the mid loop, 12 + 1 reports the form of the 13-entry sorted sibling
    assert (W("sym11", "dup"), W("sym12", "dup")) == (12, 13)
    assert by["cg-mid-sym11-f64-dup"][9] == "hipk_cg_mid_kernel<double,12,1,false>"
    sibling = [c for c in __import__("test_gpu_mid_oracle").CASES if c[0] == "cg-row13-f64"][0]
    assert by["cg-mid-sym12-dup-f64-dup"][8] == sibling[6] == FC.LS and by["cg-mid-sym12-dup-f64-dup"][9] == FC.CG3
    # HIPK_LONG_ROW = 32: 31 + 1 stays in two-launch CG, 32 + 1 leaves it
    assert (W("star31_c33", "rev"), W("star31_c33", "dup"), W("star32_c33", "dup")) == (31, 32, 33)
    assert by["cg2-row31-f64-dup"][9] == FC.CG2_64 and by["cg2-row32-f64-dup"][9] == FC.CG3
    # a full tile of 1280 entries + 256 duplicates leaves the fp64 form, not the fp32 one
    assert (_solver_props("s5_c33", "rev")["tile"], _solver_props("s5_c33", "dup")["tile"]) == (1280, 1536)
    assert by["cg2-c33-mid0-f64-dup"][9] == FC.CG3 and by["cg2-c33-mid0-f32-dup_shuf"][9] == FC.CG2_32
    assert _solver_props("star31_c33", "dup_shuf")["tile"] <= 1280


# ---------------------------------------------------------------------------------------------- the oracle on such rows
def high_precision_worst(crow, col, val, x, b, y, y_resid, u):
    """The largest error / bound of y = A x and y_resid = b - A x against long-double products and sums, with the bound derived
    for a row of L stored entries summed in any order: gamma_k = k u / (1 - k u),
        |y - y_ld| <= gamma_L sum |a_ij x_j|,      |y_resid - (b - A x)_ld| <= gamma_(L+1) (|b_i| + sum |a_ij x_j|)."""
    Ld = np.longdouble
    assert np.finfo(Ld).nmant > 60
    n, lens = len(crow) - 1, np.diff(crow)
    p = val.astype(Ld) * x[col].astype(Ld)
    s, a = np.zeros(n, Ld), np.zeros(n, Ld)
    s[lens > 0] = np.add.reduceat(p, crow[:-1][lens > 0])
    a[lens > 0] = np.add.reduceat(np.abs(p), crow[:-1][lens > 0])
    worst = 0.0
    for got, ref, k, mag in ((y, s, lens, a), (y_resid, b.astype(Ld) - s, lens + 1, np.abs(b).astype(Ld) + a)):
        gamma = k * Ld(u) / (1 - k * Ld(u))
        err = np.abs(got.astype(Ld) - ref)
        bound = gamma * mag
        bad = np.flatnonzero(err > bound)
        assert bad.size == 0, f"rows {bad[:5].tolist()} beyond the bound"
        worst = max(worst, float(np.max(err / np.where(bound > 0, bound, 1))))
    return worst


@pytest.mark.parametrize("name", ["persistent_f64_s11c_dup_shuf", "persistent_f32_s8c_zero", "wide_s4c_dup_diag_walk1", "rowwave_f32_d50c_dup_shuf",
                                  "codedcsr_f64_rag11c_shuf"])
def test_the_oracle_sums_such_rows_in_stored_order_within_the_derived_bound(oracle, name):
    c = OC.SPMV[name]
    crow, col, val = OC.arrays(c["matrix"], c["transform"], c["dtype"])
    x, w, b = OC.vectors(c["matrix"], c["dtype"])
    f64 = c["dtype"] == OC.DOUBLE
    spmv = oracle.spmv if f64 else oracle.spmv32
    y, yr = spmv(crow, col, val, x), spmv(crow, col, val, x, bsub=b)
    worst = high_precision_worst(crow, col, val, x, b, y, yr, 2.0 ** -53 if f64 else 2.0 ** -24)
    print(f"{name}: largest error / bound {worst:.3f}")
    assert 0.0 < worst <= 1.0
    # stored order, in the working precision: a few rows by hand
    f = np.float64 if f64 else np.float32
    for r in (0, 1, 299, 300, 301, len(crow) - 2):
        if crow[r + 1] - crow[r] > 32:      # the short-row rule: longer rows are summed as 64 lane-strided partial sums
            continue
        s = f(0)
        for j in range(crow[r], crow[r + 1]):
            s = f(s + f(val[j] * x[col[j]]))
        assert y[r] == s and yr[r] == f(b[r] - s), r
    # the bound bites
    with pytest.raises(AssertionError):
        high_precision_worst(crow, col, val, x, b, y, yr + np.abs(b).astype(f) * f(64 * (2.0 ** -53 if f64 else 2.0 ** -24) * 64), 2.0 ** -53 if f64 else 2.0 ** -24)
