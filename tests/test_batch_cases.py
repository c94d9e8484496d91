"""The case table of the batch solves (tests/_batch_cases.py) cannot hide a failure: checked here on the CPU oracle, no GPU needed.

Conditions, not measurements: systems of one batch must stop at different iterations (a kernel that lets one system's stop decide
for another fails), and every exit of the loops must occur somewhere in the table."""
import numpy as np
import pytest

import _batch_cases as BC
import _order_cases as OC
from _batch_patterns import sorted_rows

T = BC
SOLVERS = ("cg", "bicgstab")


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
        if c.S >= 4 and not (c.pattern and c.pattern[0] == "empty"):      # singular: all of them run to maxiter (asserted below)
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


# ------------------------------------------------------------------ the pattern axis (tests/_batch_patterns.py)
def _row_lengths(data):
    return np.diff(data["crow"])


def _diag_counts(data):
    rows = np.repeat(np.arange(data["n"]), _row_lengths(data))
    return np.bincount(rows[data["col"] == rows], minlength=data["n"])


@pytest.mark.parametrize("solver", SOLVERS)
def test_pattern_cases_hold_the_rows_they_are_named_for(results, solver):
    new = [c for c in T.PATTERN_CASES if c.solver == solver]
    kernel = [c for c in new if c.kernel]
    assert len(kernel) >= 8 and {c.pattern for c in kernel} >= {("rag31", 300), ("rag31", 2049), ("rag32", 300), ("dense32",), ("empty", 300)}
    assert {c.transform for c in kernel} >= {"rev", "shuf", "dup_diag", "dup_shuf", "zero"}
    assert {(c.dtype, c.pre) for c in kernel} == {(d, p) for d in ("f64", "f32") for p in (False, True)}
    if solver == "gmres":
        assert {c.method for c in kernel} == {"batched", "incremental"}
        assert all(c.restart == 10 for c in kernel if c.pattern[0] in ("rag31", "rag32"))
    # the 33-entry case lies outside for the row length alone
    outside = [c for c in new if not c.kernel]
    assert len(outside) == 1
    d33 = results[outside[0].id][0]
    assert d33["n"] <= T.MAX_N and _row_lengths(d33).max() == T.MAX_ROW + 1 and getattr(outside[0], "restart", 1) <= 31
    longest = [int(_row_lengths(results[c.id][0]).max()) for c in kernel]
    assert max(longest) == T.MAX_ROW and sum(w == T.MAX_ROW for w in longest) >= 3, longest
    shortest = [int(_row_lengths(results[c.id][0])[_row_lengths(results[c.id][0]) > 0].min()) for c in kernel]
    assert sum(w == 1 for w in shortest) >= 3, shortest
    for c in kernel:
        data = results[c.id][0]
        crow, col = data["crow"], data["col"]
        assert _diag_counts(data).max() <= 2, c.id          # three addends would make index_add_ order-dependent
        if c.transform in ("rev", "shuf", "dup_shuf"):
            assert OC.descents(crow, col).mean() > 0.5, c.id
        if c.transform and c.transform.startswith("dup"):
            assert OC.has_repeat(crow, col).any(), c.id
            assert _diag_counts(data).max() == 2, c.id
        if c.transform == "dup_diag":
            assert (_diag_counts(data) == 2).all(), c.id
        if c.transform == "zero":
            assert (data["vals"] == 0.0).any(), c.id
        else:
            assert not (data["vals"] == 0.0).any(), c.id
        assert (_row_lengths(data) == 0).any() == (c.pattern[0] == "empty"), c.id
        if c.pattern[0] == "rag31" and c.transform in ("dup_diag", "dup_shuf", "zero"):
            assert _row_lengths(data)[c.pattern[1] // 2] == T.MAX_ROW, c.id      # the full interior row: 31 + 1
    # a row of one entry and a row of 32 in one wavefront
    for c in kernel:
        if c.pattern[0] == "rag32":
            lens = _row_lengths(results[c.id][0])
            w = (c.pattern[1] // 2) // 64
            assert lens[c.pattern[1] // 2] == T.MAX_ROW and (lens[64 * w:64 * w + 64] == 1).any(), c.id
    # the padded copy of `values`: an odd nnz in fp64, nnz % 4 != 0 in fp32
    assert any(c.dtype == "f64" and results[c.id][0]["nnz"] % 2 == 1 for c in kernel)
    assert any(c.dtype == "f32" and results[c.id][0]["nnz"] % 4 != 0 for c in kernel)
    # the save / resume path sees a 32-entry row with Jacobi, and the second chunk
    budget = [T.BY_ID[i] for i in T.BUDGET_IDS if T.BY_ID[i].pattern and T.BY_ID[i].solver == solver]
    assert any(c.pre and _row_lengths(results[c.id][0]).max() == T.MAX_ROW for c in budget) and any(c.pattern[-1] == 2049 for c in budget)


@pytest.mark.parametrize("solver", SOLVERS)
def test_pattern_cases_end_as_the_table_says(results, solver):
    kernel = [c for c in T.PATTERN_CASES if c.solver == solver and c.kernel]
    for c in kernel:
        data, ref = results[c.id]
        if c.pattern[0] == "empty":
            # singular systems: every one runs to maxiter, info -1, x finite
            assert all((r.iterations, r.info) == (c.kwargs["maxiter"], -1) and np.isfinite(r.x).all() for r in ref), c.id
        else:
            assert all(r.info == 0 and r.breakdown == 0 and np.isfinite(r.x).all() for r in ref), (c.id, [(r.info, r.breakdown) for r in ref])
        if c.x0 == "exact":
            assert ref[1].iterations == 0 and all(r.iterations > 0 for i, r in enumerate(ref) if i != 1), c.id
    multi = [c for c in kernel if c.S >= 4]
    differ = [c for c in multi if len({r.iterations for r in results[c.id][1]}) >= 2]
    assert len(multi) >= 6 and 2 * len(differ) >= len(multi), (len(differ), len(multi))


@pytest.mark.parametrize("solver", SOLVERS)
def test_stored_order_decides_the_bits_of_a_pattern_case(results, oracle, solver):
    """The oracle sums a row in stored order.  On the same stored entries with every row sorted it must give other bits for some
    system, else the case could not tell a kernel that sums a row in another order than it is stored."""
    differ = []
    for c in T.PATTERN_CASES:
        if c.solver == solver and c.kernel and c.transform in ("rev", "shuf", "dup_shuf"):
            data, ref = results[c.id]
            crow, col, vals = sorted_rows(data["crow"], data["col"], data["vals"])
            assert not OC.descents(crow, col).any()
            ref2 = T.oracle_run(c, dict(data, crow=crow, col=col, vals=vals), oracle)
            if any(r.x.tobytes() != r2.x.tobytes() for r, r2 in zip(ref, ref2)):
                differ.append(c.id)
    assert differ


def test_an_empty_row_has_no_jacobi_form():
    import torch
    from pytorch_sparse_solver.module_a import BatchedCSR, BatchedJacobiPreconditioner
    data = T.build(next(c for c in T.PATTERN_CASES if c.pattern[0] == "empty"))
    A = BatchedCSR(torch.from_numpy(data["crow"]), torch.from_numpy(data["col"]), torch.from_numpy(data["vals"]))
    with pytest.raises(ValueError, match="zero on the diagonal"):
        BatchedJacobiPreconditioner(A)
