"""The block-Jacobi batch table (tests/_bj_batch_cases.py) and the BiCGStab mirror (tests/_bj_mirror.py) cannot hide a failure:
checked here on the CPU oracle, no GPU needed.

The mirror is pinned from three sides: with 1 x 1 blocks holding dinv it is orc_bicgstab_jacobi, with identity blocks orc_bicgstab
(bit for bit in everything but residual_norm, whose final dot is plain here and tiled there), and on the reference's own
block-Jacobi runs (tests/golden/bj_*.npz) it gives the reference's verdict.  The table's conditions are those of
tests/test_batch_cases.py: systems of a batch stop at different iterations, and every exit of the loops occurs."""
import json
import os

import numpy as np
import pytest

import _batch_cases as BC
import _bj_batch_cases as T
import _bj_mirror as MI
from conftest import BICGSTAB_MATVEC_BAND, GOLDEN, load_case

SAME = ("iterations", "matvecs", "breakdown", "info", "recurrence_rs", "b_norm", "x_norm", "threshold")


@pytest.fixture(scope="module")
def results(oracle):
    return {c.id: T.reference(c, oracle) for c in T.CASES}


def _same_but_the_final_norm(a, b, where):
    assert a.x.dtype == b.x.dtype and a.x.tobytes() == b.x.tobytes(), where
    for name in SAME:
        assert np.float64(getattr(a, name)).tobytes() == np.float64(getattr(b, name)).tobytes(), (where, name)
    assert np.isclose(a.residual_norm, b.residual_norm, rtol=1e-3, atol=1e-300), where      # plain against tiled


@pytest.mark.parametrize("cid", ["bicgstab-jac-f64-7x5-S5-x0random", "bicgstab-jac-f32-16x16-S4-x0none", "bicgstab-jac-f64-257x1-S4-x0random",
                                 "bicgstab-jac-f32-rag31n2049-dup_diag-S4-x0none", "bicgstab-jac-f64-17x15-S4-x0none-atol"])
def test_mirror_with_one_by_one_blocks_is_the_jacobi_oracle(oracle, cid):
    case = BC.BY_ID[cid]
    data, ref = BC.reference(case, oracle)
    dinv = BC.jacobi_dinv(data)
    for s, r in enumerate(ref):
        x0 = None if data["X0"] is None else data["X0"][s]
        m = MI.bicgstab_block(oracle, data["crow"], data["col"], data["vals"][s], dinv[s].reshape(-1, 1, 1), data["B"][s], x0,
                              dtype=data["vals"].dtype, **case.solve_kwargs)
        assert r.iterations > 0
        _same_but_the_final_norm(m, r, (cid, s))


@pytest.mark.parametrize("cid,bs", [("bicgstab-f64-bd-10", 2), ("bicgstab-f64-bd-11", 1), ("bicgstab-f64-7x5-S4-x0none", 4),
                                    ("bicgstab-f32-41x25-S4-x0random", 32), ("bicgstab-f64-17x15-S4-x0exact", 3),
                                    ("bicgstab-f64-16x16-S5-x0none-b0", 7), ("bicgstab-f64-32x32-S4-x0exact-maxiter5", 4)])
def test_mirror_with_identity_blocks_is_the_plain_oracle(oracle, cid, bs):
    case = BC.BY_ID[cid]
    data, ref = BC.reference(case, oracle)
    binv = T.identity_binv(case.S, data["n"], bs, data["vals"].dtype)
    for s, r in enumerate(ref):
        x0 = None if data["X0"] is None else data["X0"][s]
        m = MI.bicgstab_block(oracle, data["crow"], data["col"], data["vals"][s], binv[s], data["B"][s], x0, dtype=data["vals"].dtype,
                              **case.solve_kwargs)
        _same_but_the_final_norm(m, r, (cid, s))
    if "bd" in cid:
        assert ref[0].breakdown == int(cid[-3:]) and ref[1].breakdown == 0


def _bj_runs():
    with open(os.path.join(GOLDEN, "bj_index.json")) as f:
        return [r for r in json.load(f)["runs"] if r["solver"] == "bicgstab" and r["preconditioned"]]


@pytest.mark.parametrize("r", _bj_runs(), ids=lambda r: r["case"])
def test_mirror_reproduces_the_reference_block_jacobi_runs(oracle, r):
    d = load_case(r["case"])
    m = MI.bicgstab_block(oracle, d["crow"], d["col"], d["val"], d["binv"], d["b"], **r["kwargs"])
    x_ref = d[r["tag"] + "_x"]
    assert m.info == r["info"]
    assert abs(m.matvecs - r["matvecs"]) <= max(2, BICGSTAB_MATVEC_BAND * r["matvecs"])
    assert np.linalg.norm(m.x - x_ref) <= 1e-5 * np.linalg.norm(x_ref)


def test_fp32_apply_of_the_mirror_is_the_fp64_chain_rounded_per_step(oracle):
    """orc32_block_jacobi_apply through ctypes: every product is exact in fp64, so rounding each fma of the chain to fp32 by hand
    must give the same bits (the binding passes the right pointers and block size)."""
    rng = np.random.default_rng(5)
    n, bs = 77, 32
    binv = rng.standard_normal((3, bs, bs)).astype(np.float32)
    v = rng.standard_normal(n).astype(np.float32)
    z = MI.block_apply(oracle, binv, v, np.float32)
    want = np.zeros(n, np.float32)
    for i in range(n):
        b0 = i // bs * bs
        acc = np.float32(0)
        for j in range(min(bs, n - b0)):
            acc = np.float32(np.float64(binv.reshape(-1, bs)[i, j]) * np.float64(v[b0 + j]) + np.float64(acc))
        want[i] = acc
    assert z.dtype == np.float32 and z.tobytes() == want.tobytes()


# ------------------------------------------------------------------ the table
def test_case_ids_are_unique_and_cover_the_instantiations(results):
    ids = [c.id for c in T.CASES]
    assert len(set(ids)) == len(ids)
    assert len(T.BUDGET_IDS) == 8 and set(T.BUDGET_IDS) <= set(ids)
    assert {T.BY_ID[i].path for i in T.BUDGET_IDS} == {c.path for c in T.CASES} == {
        "hipk_cg_bjbatch_kernel<double>", "hipk_cg_bjbatch_kernel<float>", "hipk_bi_bjbatch_kernel<double>", "hipk_bi_bjbatch_kernel<float>"}
    for i in T.BUDGET_IDS:
        assert max(r.iterations for r in results[i][2]) > 7, i
    for c in T.CASES:
        data = results[c.id][0]
        assert 1 <= data["n"] <= BC.MAX_N and int(np.diff(data["crow"]).max()) <= BC.MAX_ROW and 1 <= c.bs <= 32, c.id


def test_the_shapes_cover_the_edges_of_the_apply(results):
    have = {(results[c.id][0]["n"], c.bs) for c in T.CASES}
    assert {(35, 4), (35, 1), (35, 3), (1, 1), (1, 4), (3, 32), (77, 32), (257, 3), (2049, 3), (4096, 32), (4096, 7), (1024, 4)} <= have
    assert {c.S for c in T.CASES} >= {1, 2, 5, 300, 1030} and {c.x0 for c in T.CASES} == {"none", "random", "exact"}
    for solver in ("cg", "bicgstab"):
        for dtype in ("f64", "f32"):
            mine = [c for c in T.CASES if (c.solver, c.dtype) == (solver, dtype)]
            assert any(results[c.id][0]["n"] % c.bs for c in mine), (solver, dtype, "a ragged last block")
            assert any(results[c.id][0]["n"] > 256 and 256 % c.bs for c in mine), (solver, dtype, "a block across the tile edge")
    c = T.BY_ID["cg-bj3-f64-rag31n2049-dup_shuf"]
    import _order_cases as OC
    data = results[c.id][0]
    assert OC.descents(data["crow"], data["col"]).mean() > 0.5 and OC.has_repeat(data["crow"], data["col"]).any()
    assert any(c.pattern and c.solver == "bicgstab" for c in T.CASES)


def test_systems_of_a_batch_stop_at_different_iterations(results):
    for c in T.CASES:
        if c.S >= 4 and c.kwargs.get("maxiter") is None:
            its = {r.iterations for r in results[c.id][2]}
            assert len(its) >= 2, (c.id, its)


def test_every_exit_of_the_loops_occurs_in_the_table(results):
    for solver in ("cg", "bicgstab"):
        allr = [(c, r) for c in T.CASES if c.solver == solver for r in results[c.id][2]]
        assert any(r.info == 0 and r.iterations > 0 for _, r in allr)
        assert any(c.kwargs.get("maxiter") is not None and r.iterations == c.kwargs["maxiter"] and r.info == -1 for c, r in allr)
        zero = [(c, r) for c, r in allr if r.iterations == 0]
        assert any(c.x0 == "exact" for c, _ in zero) and any(c.zero_b is not None for c, _ in zero), solver
        assert any("atol" in c.kwargs for c, _ in allr)
    for c in T.CASES:
        ref = results[c.id][2]
        if c.zero_b is not None:
            assert (ref[c.zero_b].iterations, ref[c.zero_b].info) == (0, 0), c.id
        if c.x0 == "exact":
            its = [r.iterations for r in ref]
            assert its[1 % c.S] == 0 and all(k > 0 for i, k in enumerate(its) if i != 1 % c.S), (c.id, its)
        if "atol" in c.kwargs:
            assert all(r.threshold == float(np.float32(c.kwargs["atol"])) for r in ref), c.id
    bi = [r for c in T.CASES if c.solver == "bicgstab" for r in results[c.id][2]]
    assert any(r.exit_early for r in bi), "no BiCGStab system leaves through exit_early"
    for name, code in (("bicgstab-bj2-f64-bd-10", -10), ("bicgstab-bj2-f64-bd-11", -11)):
        assert T.BY_ID[name].identity
        r = results[name][2]
        assert r[0].breakdown == code and r[1].breakdown == 0 and r[1].info == 0, (name, r[0], r[1])


def test_every_system_not_stopped_by_maxiter_or_a_breakdown_converges(results):
    for c in T.CASES:
        for s, r in enumerate(results[c.id][2]):
            assert np.isfinite(r.x).all(), (c.id, s)
            if c.kwargs.get("maxiter") is None and r.breakdown == 0:
                assert r.info == 0, (c.id, s, r.residual_norm, r.threshold)
    clean = [c for c in T.CASES if all(r.breakdown == 0 for r in results[c.id][2])]
    assert 4 * len(clean) >= 3 * len(T.CASES), "most cases must be free of breakdowns"


def test_identity_blocks_make_the_preconditioner_the_identity(oracle):
    rng = np.random.default_rng(2)
    v = rng.standard_normal(35)
    for bs in (1, 4, 32):
        binv = T.identity_binv(1, 35, bs, np.float64)[0]
        assert MI.block_apply(oracle, binv, v, np.float64).tobytes() == v.tobytes()
