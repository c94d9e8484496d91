"""The case table of the batch solves (tests/_batch_cases.py) cannot hide a failure: checked here on the CPU oracle, no GPU needed.

Conditions, not measurements: systems of one batch must stop at different iterations (a kernel that lets one system's stop decide
for another fails), and every exit of the loops must occur somewhere in the table."""
import numpy as np
import pytest

import _batch_cases as BC


@pytest.fixture(scope="module")
def results(oracle):
    return {c.id: BC.reference(c, oracle) for c in BC.CASES}


def test_case_ids_are_unique_and_budget_cases_exist():
    ids = [c.id for c in BC.CASES]
    assert len(set(ids)) == len(ids), sorted(i for i in ids if ids.count(i) > 1)
    assert set(BC.BUDGET_IDS) <= set(ids)


def test_kernel_cases_lie_inside_the_envelope_and_the_others_outside(results):
    for c in BC.CASES:
        data, _ = results[c.id]
        longest = int(np.diff(data["crow"]).max())
        inside = 1 <= data["n"] <= BC.MAX_N and longest <= BC.MAX_ROW
        assert inside == c.kernel, (c.id, data["n"], longest)
    assert any(not c.kernel for c in BC.CASES)


def test_the_grids_cover_the_edges_of_the_layout():
    ns = {c.grid[0] * c.grid[1] for c in BC.CASES if c.grid}
    assert {35, 255, 256, 257, 1024, 1025, 2025, 2048, 2049, 2304, 4096, 4097} <= ns, sorted(ns)
    assert {c.dense for c in BC.CASES if c.dense} >= {"spd1", "spd2", "spd3", "bd-10", "bd-11"}
    assert {c.S for c in BC.CASES} >= {1, 2, 5, 300, 1030}
    for solver in ("cg", "bicgstab"):
        for dtype in ("f64", "f32"):
            for pre in (False, True):
                assert any((c.solver, c.dtype, c.pre) == (solver, dtype, pre) and c.kernel for c in BC.CASES), (solver, dtype, pre)


def test_systems_of_a_batch_stop_at_different_iterations(results):
    for c in BC.CASES:
        if c.S >= 4:
            its = {r.iterations for r in results[c.id][1]}
            assert len(its) >= 2, (c.id, its)


def test_every_exit_of_the_loops_occurs_in_the_table(results):
    allr = [(c, r) for c in BC.CASES if c.kernel for r in results[c.id][1]]
    assert any(r.info == -1 for _, r in allr)
    assert any(r.breakdown == -10 for _, r in allr)
    assert any(r.breakdown == -11 for _, r in allr)
    assert any(r.iterations == 0 for _, r in allr)
    assert any(r.info == 0 and r.iterations > 0 for _, r in allr)
    assert any(c.kwargs.get("maxiter") is not None and r.iterations == c.kwargs["maxiter"] for c, r in allr), "stopped by maxiter"
    # the breakdown fixtures: the fixture system breaks down, its partner converges
    for name, code in (("bicgstab-f64-bd-10", -10), ("bicgstab-f64-bd-11", -11)):
        r = results[name][1]
        assert r[0].breakdown == code and r[1].breakdown == 0 and r[1].info == 0, (name, r[0], r[1])
    # the b = 0 systems stop at once with info 0
    for c in BC.CASES:
        if c.zero_b is not None:
            r = results[c.id][1][c.zero_b]
            assert (r.iterations, r.info) == (0, 0), (c.id, r)
    # 'exact' x0: system 1 alone runs no iteration
    for c in BC.CASES:
        if c.x0 == "exact" and c.kernel:
            its = [r.iterations for r in results[c.id][1]]
            assert its[1 % c.S] == 0 and all(k > 0 for i, k in enumerate(its) if i != 1 % c.S), (c.id, its)
    # atol decides in the atol cases: the threshold is atol itself
    for c in BC.CASES:
        if "atol" in c.kwargs:
            assert all(r.threshold == float(np.float32(c.kwargs["atol"])) for r in results[c.id][1]), c.id
