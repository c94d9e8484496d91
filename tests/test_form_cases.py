"""The form table of the library (csrc/hipk_forms.h, hipk_solve_form_name) and the case tables that pin its rows to the oracle
(tests/_form_cases.py; the mid kernels: tests/test_gpu_mid_oracle.py) kept in step -- no GPU needed: every form has a case or a
stated reason, every expected form exists, and each case's matrix has the chunk count, longest row, fullest tile and window that
its expected form implies (computed in numpy from the CSR arrays, not asked of the library)."""
import os
import re

import numpy as np
import pytest

import _form_cases as FC
from conftest import PKG


def _forms():
    import torch  # noqa: F401  (HIP runtime first)
    from pytorch_sparse_solver import _hipk
    return _hipk.solve_forms()


def _mid_cases():
    import test_gpu_mid_oracle as MO
    return [(c[0], c[6]) for c in MO.CASES if " -> " not in c[6] and "_mid_kernel<" in c[6]]   # a mid kernel's form is its path


def _owners(cases=FC.CASES):
    own = {}
    for c in cases:
        own.setdefault(c[8], []).append(c[0])
    for cid, form in _mid_cases():
        own.setdefault(form, []).append(cid)
    return own


def _orphans(cases):
    own = _owners(cases)
    return [f for f in _forms() if f not in own and f not in FC.UNREACHABLE]


def test_every_form_has_a_case_or_a_reason_and_every_expected_form_is_a_row():
    forms = _forms()
    assert len(forms) == len(set(forms)) and len(forms) >= 100
    assert _orphans(FC.CASES) == []
    own = _owners()
    assert sorted(f for f in own if f not in forms) == []
    # only what needs more than 384 MiB of vectors may go without a bitwise case, and nothing listed there has one
    assert set(FC.UNREACHABLE) <= {"cg three-launch, streams", "cg three-launch, streams + flat direction"}
    assert all(f in forms and f not in own and reason for f, reason in FC.UNREACHABLE.items())


def test_removing_the_only_case_of_a_form_names_it():
    own = _owners()
    sole = {f: ids[0] for f, ids in own.items() if len(ids) == 1 and ids[0] in {c[0] for c in FC.CASES}}
    assert sole, "no form with a single case: the check below would be vacuous"
    for form, cid in sole.items():
        assert _orphans([c for c in FC.CASES if c[0] != cid]) == [form]
    # ... and of a form with several: all of them
    form = FC.CG2_64
    assert _orphans([c for c in FC.CASES if c[8] != form]) == [form]


def test_case_ids_solvers_and_switches():
    ids = [c[0] for c in FC.CASES]
    assert len(ids) == len(set(ids))
    text = open(os.path.join(PKG, "csrc", "hipk_switch.h")).read()
    switches = set(re.findall(r'^\s*\{"(HIPK_[A-Z0-9_]+)"', text, flags=re.M))
    for cid, solver, key, dtn, kw, env, x0kind, path, form in FC.CASES:
        assert solver in ("cg", "pcg", "bicgstab", "pbicgstab", "gmres", "pgmres") and (cid.startswith(solver + "-") or cid.startswith("cg2-")), cid
        assert key in FC.MATRICES and key in FC.MATRIX_PROPS and dtn in (FC.F64, FC.F32), cid
        assert set(env) <= switches, (cid, set(env) - switches)
        assert x0kind in (None, "rand", "exact", "fixture") and (x0kind != "fixture" or key in FC.FIXED_B), cid
        assert path.split(" -> ")[-1] in (FC.LS, FC.CG_LDS, FC.BI_LDS, FC.GM_LDS, FC.GM_SMALL) or path == form, cid
        # a kernel form finishes in that kernel; a launch-sequence form in "launch sequence"
        last = path.split(" -> ")[-1]
        assert form.startswith(last + "<") or form == last or (last == FC.LS and not form.startswith("hipk_")), cid


_props = {}


def _matrix_props(key):
    if key not in _props:
        _props[key] = FC.matrix_props(FC.MATRICES[key]())
    return _props[key]


@pytest.mark.parametrize("key", sorted(FC.MATRICES))
def test_matrix_is_what_the_table_says(key):
    got = _matrix_props(key)
    for k, v in FC.MATRIX_PROPS[key].items():
        assert got[k] == (FC._g1() if v == "g1" else v), (key, k, got)


def _implied(case, p):
    """What the expected form of `case` implies about its matrix (p: matrix_props), from the guards of hipk_cg_path_*,
    hipk_bi_path_* and hipk_gm_path_choose; a list of the violated ones."""
    cid, solver, key, dtn, kw, env, x0kind, path, form = case
    g, W, tile, g1 = p["g"], p["W"], p["tile"], FC._g1()
    T = "double" if dtn == FC.F64 else "float"
    pre = solver in ("pcg", "pbicgstab", "pgmres")
    m = kw.get("restart", 0)
    bad = []

    def need(cond, what):
        if not cond:
            bad.append(what)
    fam = {"cg": "CG", "pcg": "CG", "bicgstab": "BICGSTAB", "pbicgstab": "BICGSTAB", "gmres": "GMRES", "pgmres": "GMRES"}[solver]
    # the mid loop cannot have finished the solve: switched off, refused by the matrix, made to hand back, or not offered at all
    mid_min = 32 if fam == "GMRES" else 8
    mid_away = (g <= mid_min or W > 12 or p["slots"] > 64 or p["range"] > 512 or env.get(f"HIPK_{fam}_MID") == "0" or
                "HIPK_TEST_LDS_NOT_RESIDENT" in env or f"HIPK_{fam}_NO_LDS_LOOP" in env or f"HIPK_{fam}_NO_SMALL" in env or
                "HIPK_GMRES_NO_CYCLE" in env or kw.get("callback") or m > 31 or kw["maxiter"] == 0 or x0kind == "exact" and fam == "GMRES")
    mk = re.match(r"hipk_(cg|bi|gm)_solve_lds_kernel<(double|float),(true|false)(?:,(true|false))?>$", form)
    if mk:
        kind, t, local, fpre = mk.groups()
        need(kind == {"CG": "cg", "BICGSTAB": "bi", "GMRES": "gm"}[fam] and t == T, "kernel family / dtype")
        need(kind == "gm" or fpre == ("true" if pre else "false"), "PRE")
        need(g <= 32 and kw["maxiter"] > 0 and mid_away, "<= 32 chunks, maxiter > 0, no mid loop")
        need(W <= (32 if kind == "gm" else 12), "row length")
        need(kind != "gm" or m <= 31, "restart <= 31")
        agent = {"cg": "HIPK_CG_LOOP_AGENT", "bi": "HIPK_BICGSTAB_LOOP_AGENT", "gm": "HIPK_GM_CYCLE_AGENT"}[kind] in env
        need((local == "true") == (g <= g1 and g <= 8 and not agent), "LOCAL: one XCD and no agent switch")
        need(g <= 8 or "HIPK_NO_LDS_SPREAD" not in env, "spread allowed")
        return bad
    if form.startswith("hipk_gm_cycle_small_kernel<"):
        need(form == f"hipk_gm_cycle_small_kernel<{T}>" and g <= 8 and m <= 31 and W <= 32 and "HIPK_GMRES_NO_LDS_CYCLE" in env, "cycle_small")
        return bad
    if "_mid_kernel<" in form:
        need(g > mid_min and W <= 12 and p["slots"] <= 64 and p["range"] <= 512, "mid loop's envelope")
        return bad
    need(path.split(" -> ")[-1] == FC.LS, "a launch-sequence form finishes in the launch sequence")
    need(mid_away, "the mid loop would have finished this solve")
    # the LDS loop cannot have finished it either
    if fam in ("CG", "BICGSTAB"):
        lds_away = (g > 32 or W > 12 or kw["maxiter"] == 0 or f"HIPK_{fam}_NO_LDS_LOOP" in env or f"HIPK_{fam}_NO_SMALL" in env or
                    (g > 8 and "HIPK_NO_LDS_SPREAD" in env) or bool(kw.get("callback")) or "HIPK_TEST_LDS_NOT_RESIDENT" in env)
        need(lds_away, "the LDS loop would have finished this solve")
        small = g <= 8 and f"HIPK_{fam}_NO_SMALL" not in env
    if fam == "CG" and not pre:
        cap = 1280 if T == "double" else 2048
        two = (not small and 32 < g <= 150 and tile <= cap and W <= 32 and env.get("HIPK_CG_TWO_LAUNCH") != "0" and
               env.get("HIPK_TEST_LDS_NOT_RESIDENT") != "2")
        want = (FC.CG2_64 if T == "double" else FC.CG2_32) if two else FC.CG3S if small else FC.CG3
        need(form == want, f"guards of hipk_cg_path_two / small say {want!r}")
    elif fam == "CG":
        need(form == FC.PCG3, "pcg has one launch sequence")
    elif fam == "BICGSTAB":
        want = (FC.BI5S if small else FC.BI5) + (FC.CB if kw.get("callback") else ", Jacobi" if pre else "")
        need(form == want, f"small / M say {want!r}")
    else:
        small = g <= 8 and m <= 31 and "HIPK_GMRES_NO_SMALL" not in env
        wide = small and "HIPK_GMRES_NO_WIDE" not in env
        cyc = wide and not kw.get("callback") and W <= 32 and "HIPK_GMRES_NO_CYCLE" not in env
        spread = 8 < g <= 32 and m <= 31 and not kw.get("callback") and W <= 32 and not ({"HIPK_GMRES_NO_SMALL", "HIPK_GMRES_NO_CYCLE", "HIPK_NO_LDS_SPREAD"} & set(env))
        ran_none = kw["maxiter"] == 0 or x0kind == "exact" or "HIPK_TEST_LDS_NOT_RESIDENT" in env   # (or the kernel handed back)
        need(ran_none or not (cyc or spread), "a one-launch cycle would have run")
        split = not small and env.get("HIPK_GM_SPLIT_NORM", "0" if g < 1536 else "1") != "0"
        want = (FC.GSW if wide else FC.GS256 if small else FC.GBIG if m > 31 else FC.GLF if "HIPK_GMRES_NO_STREAM" in env else FC.GLS)
        want += (FC.SPLIT if split else "") + (FC.CB if kw.get("callback") else "")
        need(form == want, f"hipk_gm_path_choose says {want!r}")
    return bad


@pytest.mark.parametrize("case", FC.CASES, ids=[c[0] for c in FC.CASES])
def test_matrix_has_the_shape_the_expected_form_implies(case):
    assert _implied(case, _matrix_props(case[2])) == [], case[0]


def test_the_capacity_cases_sit_exactly_on_and_one_past_each_guard():
    """Two-launch CG: 33 / 150 / 151 chunks, tiles of 1280 / 1281 (fp64) and 2048 / 2049 (fp32) entries, rows of 32 / 33."""
    by_id = {c[0]: c for c in FC.CASES}

    def p(cid):
        return _matrix_props(by_id[cid][2])
    assert (p("cg2-c32-mid0-nospread-f64")["g"], p("cg2-c33-mid0-f64")["g"], p("cg2-c150-mid0-f64")["g"], p("cg2-c151-mid0-f64")["g"]) == (32, 33, 150, 151)
    assert (p("cg2-c33-mid0-f64")["tile"], p("cg2-tile1281-mid0-f64")["tile"], p("cg2-tile2048-mid0-f32")["tile"], p("cg2-tile2049-mid0-f32")["tile"]) == \
        (1280, 1281, 2048, 2049)
    assert (p("cg2-row32-f64")["W"], p("cg2-row33-f64")["W"]) == (32, 33)
    assert p("cg2-reach-out-f64")["range"] > 512 and p("cg-spread-far-c32-f64")["slots"] > 64
    assert (p("cg-lds-row12-f64")["W"], p("cg-small-row13-f64")["W"], p("gmres-lds-row32-f32")["W"], p("gmres-small-row33-f64")["W"]) == (12, 13, 32, 33)


def test_oracle_gmres_takes_restart_up_to_255(oracle):
    n = 300
    M = FC._dense(n, False, 5)
    b = np.random.default_rng(0).standard_normal(n)
    ref = oracle.gmres(M.indptr, M.indices, M.data, b, tol=1e-12, restart=255, maxiter=1)
    assert ref.info == 0 and np.linalg.norm(M @ ref.x - b) <= 1e-9 * np.linalg.norm(b)
    for fn, args in ((oracle.gmres, (M.data, b)), (oracle.gmres32, (M.data.astype(np.float32), b.astype(np.float32)))):
        with pytest.raises(ValueError, match="restart <= 255"):
            fn(M.indptr, M.indices, *args, restart=256)
    dinv = 1.0 / M.diagonal()
    with pytest.raises(ValueError, match="restart <= 255"):
        oracle.gmres_jacobi(M.indptr, M.indices, M.data, dinv, b, restart=256)
    with pytest.raises(ValueError, match="restart <= 255"):
        oracle.gmres_jacobi32(M.indptr, M.indices, M.data.astype(np.float32), dinv.astype(np.float32), b.astype(np.float32), restart=256)
