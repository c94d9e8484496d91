"""The case table of gmres_batch (tests/_gmres_batch_cases.py) cannot hide a failure: checked here on the CPU oracle, no GPU needed.

Conditions, not measurements: systems of one batch must end at different cycles (and, with 'incremental', leave a cycle early), and
every exit of the solve must occur somewhere in the table."""
import numpy as np
import pytest

import _gmres_batch_cases as GC


@pytest.fixture(scope="module")
def results(oracle):
    return {c.id: GC.reference(c, oracle) for c in GC.CASES}


def test_case_ids_are_unique_and_budget_cases_exist():
    ids = [c.id for c in GC.CASES]
    assert len(set(ids)) == len(ids), sorted(i for i in ids if ids.count(i) > 1)
    assert set(GC.BUDGET_IDS) <= set(ids) and len(GC.BUDGET_IDS) >= 10
    budget = [GC.BY_ID[i] for i in GC.BUDGET_IDS]
    assert {(c.dtype, c.pre) for c in budget} == {(d, p) for d in ("f64", "f32") for p in (False, True)}
    assert {c.method for c in budget} == {"batched", "incremental"}


def test_kernel_cases_lie_inside_the_envelope_and_the_others_outside(results):
    for c in GC.CASES:
        data, _ = results[c.id]
        longest = int(np.diff(data["crow"]).max())
        inside = 1 <= data["n"] <= GC.MAX_N and longest <= GC.MAX_ROW and 1 <= c.restart <= GC.MAX_RESTART
        assert inside == c.kernel, (c.id, data["n"], longest, c.restart)
    outside = [c for c in GC.CASES if not c.kernel]
    assert any(c.restart == 32 and c.grid == (16, 16) for c in outside) and any(c.grid == (17, 241) for c in outside)


def test_the_table_covers_the_edges_of_the_layout():
    kernel = [c for c in GC.CASES if c.kernel]
    ns = {c.grid[0] * c.grid[1] for c in kernel if c.grid}
    assert {35, 255, 256, 257, 1024, 1025, 2025, 2048, 2049, 2304, 4096} <= ns, sorted(ns)
    assert {c.restart for c in kernel} >= {1, 2, 5, 7, 8, 9, 16, 20, 30, 31}
    assert {c.dense for c in kernel if c.dense} == {1, 2, 3} and any(c.dense == 3 and c.restart == 5 for c in kernel)
    assert {c.S for c in kernel} >= {1, 2, 5, 300, 1030}
    assert any(c.S == 300 and c.grid == (32, 32) and c.restart == 20 for c in kernel)
    assert any(c.S == 1030 and c.grid == (7, 5) and c.restart == 5 for c in kernel)
    assert {c.x0 for c in kernel} == {"none", "random", "exact"}
    for dtype in ("f64", "f32"):
        for pre in (False, True):
            for method in ("batched", "incremental"):
                assert any((c.dtype, c.pre, c.method) == (dtype, pre, method) for c in kernel), (dtype, pre, method)


def test_systems_of_a_batch_end_at_different_cycles(results):
    multi = [c for c in GC.CASES if c.kernel and c.grid and c.S >= 4 and not c.special]
    differ = [c for c in multi if len({r.iterations for r in results[c.id][1]}) >= 2]
    assert 2 * len(differ) >= len(multi), (len(differ), len(multi))


def test_incremental_cases_leave_a_cycle_early(results):
    early = [c.id for c in GC.CASES if c.kernel and c.method == "incremental" and c.grid and not c.special and
             any(0 < r.iterations and r.matvecs < 2 + r.iterations * (c.restart + 1) for r in results[c.id][1])]
    assert len(early) >= 3, early


def test_every_exit_of_the_solve_occurs_in_the_table(results):
    allr = [(c, r) for c in GC.CASES if c.kernel for r in results[c.id][1]]
    assert any(r.info == 0 and r.iterations > 0 for _, r in allr)
    assert any(c.kwargs.get("maxiter") is not None and r.iterations == c.kwargs["maxiter"] and r.info == -1 for c, r in allr), "stopped by maxiter"
    assert any(r.iterations == 0 for _, r in allr)
    # 'exact' x0: system 1 alone runs no cycle, 2 operator applications
    for c in GC.CASES:
        if c.x0 == "exact" and c.kernel:
            rs = results[c.id][1]
            e = 1 % c.S
            assert (rs[e].iterations, rs[e].matvecs, rs[e].info) == (0, 2, 0), (c.id, rs[e])
            assert all(r.iterations > 0 for i, r in enumerate(rs) if i != e), c.id
    # the b = 0 systems stop at once with info 0
    for c in GC.CASES:
        if c.zero_b is not None:
            r = results[c.id][1][c.zero_b]
            assert (r.iterations, r.info) == (0, 0), (c.id, r)
    # happy breakdown: the diagonal-only system, next to a partner that converges normally
    for c in GC.CASES:
        if c.special == "diag":
            r = results[c.id][1]
            assert (r[0].breakdown, r[0].iterations, r[0].matvecs, r[0].info) == (1, 1, 4, 0), (c.id, r[0])
            assert r[1].breakdown == 0 and r[1].info == 0 and r[1].iterations > 1, (c.id, r[1])
    # the all-zero system: 'batched' meets the non-positive pivot and the elimination gives NaN, 'incremental' gives inf
    seen = set()
    for c in GC.CASES:
        if c.special == "zero":
            r = results[c.id][1]
            seen.add(c.method)
            if c.method == "batched":
                assert np.isnan(r[0].x).all() and r[0].info == -1 and r[0].iterations == 1, (c.id, r[0])
            else:
                assert np.isinf(r[0].x).all() and r[0].info == 0 and r[0].iterations == 1, (c.id, r[0])
            assert r[1].info == 0 and np.isfinite(r[1].x).all() and r[1].iterations > 1, (c.id, r[1])
    assert seen == {"batched", "incremental"}
    # atol decides in the atol case: the threshold is ten times atol itself (TSL:768)
    for c in GC.CASES:
        if "atol" in c.kwargs:
            assert all(r.threshold == float(np.float32(c.kwargs["atol"])) * 10 for r in results[c.id][1]), c.id
