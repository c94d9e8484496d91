"""gmres_batch on the GPU: every case of tests/_gmres_batch_cases.py through hipk_gm_batch_kernel (csrc/hipk_batch_gm.hip), bitwise
against the CPU oracle per system (gmres_impl with gpu_tolerances = 1); the three routes and the launch budgets agree; the C entry
point keeps the memory contract."""
import ctypes

import numpy as np
import pytest
import torch

import _batch_cases as BC
import _gmres_batch_cases as GC
from _arena import Arena, check_memory, guard_bytes_for, run_states
from test_gpu_batch import _Abi, check_abi_accepts_dense32, check_jacobi_vectors_on_repeated_diagonals, check_stats_in_long_double

pytestmark = pytest.mark.gpu
DEV = "cuda"
KERNEL_CASES = [c for c in GC.CASES if c.kernel]
PATTERN_KERNEL_CASES = [c for c in GC.PATTERN_CASES if c.kernel]
NORMS = ("residual_norm", "x_norm", "b_norm", "threshold")


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _same(a, b):
    """Bitwise equal, NaNs in equal places (a NaN's sign and payload are not part of the contract)."""
    a, b = np.atleast_1d(np.asarray(a)), np.atleast_1d(np.asarray(b))
    na, nb = np.isnan(a), np.isnan(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(na, nb) and _bits(a[~na]) == _bits(b[~nb])


def _operands(case, data):
    from pytorch_sparse_solver.module_a import BatchedCSR, BatchedJacobiPreconditioner
    A = BatchedCSR(torch.from_numpy(data["crow"]).to(DEV), torch.from_numpy(data["col"]).to(DEV), torch.from_numpy(data["vals"]).to(DEV))
    B = torch.from_numpy(data["B"]).to(DEV)
    X0 = None if data["X0"] is None else torch.from_numpy(data["X0"]).to(DEV)
    M = BatchedJacobiPreconditioner(A) if case.pre else None
    return A, B, X0, M


def _solve(case, ops, route):
    from pytorch_sparse_solver.module_a import get_last_stats, gmres_batch
    A, B, X0, M = ops
    X, info = gmres_batch(A, B, X0, M=M, route=route, **case.solve_kwargs)
    return X, info, get_last_stats()


def _assert_oracle(case, ref, X, info, st):
    assert info.dtype == torch.int64 and info.device.type == "cpu" and tuple(info.shape) == (case.S,)
    assert st.method == ("pgmres_jacobi_batch" if case.pre else "gmres_batch")
    Xh = X.cpu().numpy()
    assert Xh.dtype == (np.float64 if case.dtype == "f64" else np.float32)
    for s, r in enumerate(ref):
        where = f"{case.id} system {s}"
        got = (st.iterations[s], st.matvecs[s], st.info[s], st.breakdown[s])
        assert got == (r.iterations, r.matvecs, r.info, r.breakdown), (where, got, (r.iterations, r.matvecs, r.info, r.breakdown))
        assert int(info[s]) == r.info, where
        assert _same(Xh[s], r.x.astype(Xh.dtype)), f"{where}: x differs (max {np.nanmax(np.abs(Xh[s] - r.x)):.3e})"
        for name in NORMS:
            assert _same(np.float64(getattr(st, name)[s]), np.float64(getattr(r, name))), (where, name, getattr(st, name)[s], getattr(r, name))


def _reference(case, oracle, M):
    """The oracle per system, with the Jacobi vectors the solve itself used."""
    data, ref = GC.reference(case, oracle)
    if case.pre:
        dinv = M.dinv.cpu().numpy()
        if _bits(dinv) != _bits(GC.jacobi_dinv(data)):
            ref = GC.oracle_run(case, data, oracle, dinv=dinv)
    return ref


# ------------------------------------------------------------------ every case of the table through the kernel
@pytest.mark.parametrize("case", KERNEL_CASES, ids=lambda c: c.id)
def test_gmres_batch_kernel_matches_the_oracle(hipk, oracle, case):
    data, _ = GC.reference(case, oracle)
    ops = _operands(case, data)
    X, info, st = _solve(case, ops, "kernel")
    assert hipk.last_solve_path() == case.path and st.path == case.path
    assert st.launches == 1
    _assert_oracle(case, _reference(case, oracle, ops[3]), X, info, st)


def test_batched_jacobi_is_the_single_preconditioner_on_convection_diffusion(hipk):
    from pytorch_sparse_solver.module_a import BatchedCSR, BatchedJacobiPreconditioner, JacobiPreconditioner
    for cid in ("gmres-jac-f64-16x16-r20-i-S4-x0none", "gmres-jac-f32-257x1-r8-b-S4-x0random"):
        data = GC.build(GC.BY_ID[cid])
        A = BatchedCSR(torch.from_numpy(data["crow"]).to(DEV), torch.from_numpy(data["col"]).to(DEV), torch.from_numpy(data["vals"]).to(DEV))
        M = BatchedJacobiPreconditioner(A)
        for s in range(A.batch):
            assert torch.equal(M.dinv[s], JacobiPreconditioner(A.system(s)).dinv)


@pytest.mark.parametrize("cid", ["gmres-jac-f64-rag31n300-dup_diag-r10-b-S4-x0random", "gmres-f64-rag31n300-dup_shuf-r10-i-S4-x0none"])
def test_batched_jacobi_adds_a_diagonal_stored_twice_like_the_single_preconditioner(hipk, oracle, cid):
    check_jacobi_vectors_on_repeated_diagonals(GC.reference(GC.BY_ID[cid], oracle)[0])


@pytest.mark.parametrize("case", PATTERN_KERNEL_CASES, ids=lambda c: c.id)
def test_pattern_cases_hold_in_long_double(hipk, oracle, case):
    assert "atol" not in case.kwargs
    data, _ = GC.reference(case, oracle)
    ops = _operands(case, data)
    X, info, st = _solve(case, ops, "kernel")
    assert st.path == case.path
    check_stats_in_long_double(case, data, X, st, ops[3], "pgmres" if case.pre else "gmres")


# ------------------------------------------------------------------ routes
@pytest.mark.parametrize("case", KERNEL_CASES, ids=lambda c: c.id)
def test_loop_and_auto_routes_agree_with_the_kernel(hipk, oracle, case):
    from pytorch_sparse_solver.module_a import batch as batch_mod
    data, _ = GC.reference(case, oracle)
    ops = _operands(case, data)
    Xk, ik, sk = _solve(case, ops, "kernel")
    Xl, il, sl = _solve(case, ops, "loop")
    assert sl.path == "loop" and sl.launches == 0
    Xa, ia, sa = _solve(case, ops, "auto")
    assert sa.path == (case.path if case.S >= batch_mod.GMRES_BATCH_MIN_SYSTEMS else "loop")
    for X, i, st in ((Xl, il, sl), (Xa, ia, sa)):
        assert _same(X.cpu().numpy(), Xk.cpu().numpy()) and torch.equal(i, ik), case.id
        assert st.method == sk.method
        for name in ("iterations", "matvecs", "info", "breakdown"):
            assert getattr(st, name) == getattr(sk, name), (case.id, name)
        for name in NORMS + ("recurrence_rs",):
            assert _same(np.asarray(getattr(st, name), dtype=np.float64), np.asarray(getattr(sk, name), dtype=np.float64)), (case.id, name)


def test_auto_switches_exactly_at_gmres_batch_min_systems(hipk, oracle, monkeypatch):
    from pytorch_sparse_solver.module_a import batch as batch_mod
    case = GC.BY_ID["gmres-f64-17x15-r7-i-S5-x0exact"]
    data, ref = GC.reference(case, oracle)
    ops = _operands(case, data)
    for least, path in ((5, case.path), (6, "loop")):
        monkeypatch.setattr(batch_mod, "GMRES_BATCH_MIN_SYSTEMS", least)
        X, info, st = _solve(case, ops, "auto")
        assert st.path == path
        _assert_oracle(case, ref, X, info, st)


def test_outside_the_envelope_auto_loops_and_kernel_raises(hipk, oracle):
    outside = [c for c in GC.CASES if not c.kernel]
    assert len(outside) == 3
    for case, bound in zip(outside, ("at most 31", "at most 4096 rows", r"at most 32 stored entries per row \(n = 32, longest row 33\)")):
        data, ref = GC.reference(case, oracle)
        ops = _operands(case, data)
        with pytest.raises(ValueError, match=bound):
            _solve(case, ops, "kernel")
        X, info, st = _solve(case, ops, "auto")
        assert st.path == "loop"
        assert [int(i) for i in info] == [r.info for r in ref] and st.iterations == [r.iterations for r in ref]
        for s, r in enumerate(ref):
            assert _bits(X[s].cpu().numpy()) == _bits(r.x), (case.id, s)


def test_values_updated_in_place_are_the_values_every_route_solves(hipk, oracle, monkeypatch):
    """nnz = 151 (odd): the kernel route works on a padded copy of `values`, which must follow an in-place update."""
    from pytorch_sparse_solver.module_a import batch as batch_mod
    case = GC.BY_ID["gmres-f64-7x5-r5-b-S4-x0none"]
    data, ref = GC.reference(case, oracle)
    assert data["nnz"] % 2 == 1
    ops = _operands(case, data)
    X, info, st = _solve(case, ops, "kernel")
    _assert_oracle(case, ref, X, info, st)
    new = dict(data, vals=np.ascontiguousarray(data["vals"][::-1] * 1.5))      # other matrices in every slot
    ref2 = GC.oracle_run(case, new, oracle)
    assert [r.matvecs for r in ref2] != [r.matvecs for r in ref]
    ops[0].values.copy_(torch.from_numpy(new["vals"]).to(DEV))
    monkeypatch.setattr(batch_mod, "GMRES_BATCH_MIN_SYSTEMS", 2)
    for route, path in (("kernel", case.path), ("loop", "loop"), ("auto", case.path)):
        X, info, st = _solve(case, ops, route)
        assert st.path == path
        _assert_oracle(case, ref2, X, info, st)


# ------------------------------------------------------------------ launch budgets: the resume path
@pytest.mark.parametrize("budget", [7, 1])
@pytest.mark.parametrize("cid", GC.BUDGET_IDS)
def test_bits_do_not_depend_on_the_launch_budget(hipk, oracle, monkeypatch, cid, budget):
    case = GC.BY_ID[cid]
    data, _ = GC.reference(case, oracle)
    ops = _operands(case, data)
    ref = _reference(case, oracle, ops[3])
    monkeypatch.setenv("HIPK_BATCH_LAUNCH_ITS", str(budget))
    X, info, st = _solve(case, ops, "kernel")
    assert max(r.iterations for r in ref) > 1, "the case must need more than one cycle"
    assert st.launches > 1, st.launches
    _assert_oracle(case, ref, X, info, st)


# ------------------------------------------------------------------ the C entry point: memory contract
class _GmAbi(_Abi):
    """hipk_gmres_solve_batch between guards (see _Abi): `work` exactly hipk_gmres_batch_work_bytes."""

    def __init__(self, hipk, case, data, dinv):
        super().__init__(hipk, case, data, dinv)
        self.wb = hipk.gmres_batch_work_bytes(self.n, self.nnz, self.S, self.dt, case.restart, self.pre)

    def call(self, work_ptr, work_bytes, stream=None, ldb=None, n=None, restart=None):
        hipk = self.hipk
        prm = hipk.Params()
        kw = self.case.solve_kwargs
        prm.tol, prm.atol = float(kw["tol"]), float(kw.get("atol", 0.0))
        prm.maxiter = -1 if kw.get("maxiter") is None else int(kw["maxiter"])
        prm.restart = int(kw["restart"] if restart is None else restart)
        prm.gmres_method = {"batched": hipk.GMRES_BATCHED, "incremental": hipk.GMRES_INCREMENTAL}[kw["solve_method"]]
        prm.gpu_tolerances = 1
        st = (hipk.Stats * self.S)()
        self.a_x.put(self.x_start)
        rc = hipk.lib().hipk_gmres_solve_batch(
            self.n if n is None else n, self.nnz, self.crow.data_ptr(), self.col.data_ptr(), self.a_vals.data_ptr(), self.ldv,
            self.a_dinv.data_ptr() if self.pre else None, self.ldd if self.pre else 0, self.S, self.a_b.data_ptr(),
            self.ldb if ldb is None else ldb, self.a_x.data_ptr(), self.ldx, hipk._dtype_code(self.dt), work_ptr, work_bytes,
            ctypes.byref(prm), st, hipk._stream(torch.device(DEV)) if stream is None else stream)
        torch.cuda.synchronize()
        return rc, st


ABI_IDS = ["gmres-f64-17x15-r7-i-S5-x0exact", "gmres-jac-f32-41x25-r30-i-S4-x0none", "gmres-f64-45x45-r31-b-S4-x0random",
           "gmres-jac-f64-7x5-r2-b-S5-x0random", "gmres-f64-7x5-r5-b-S2-x0none-zero",
           # rows of 2 to 32 entries, unsorted, a column stored twice; ldv > nnz
           "gmres-f64-rag31n300-dup_shuf-r10-i-S4-x0none"]


@pytest.mark.parametrize("cid", ABI_IDS)
def test_abi_workspace_states_guards_and_pads(hipk, oracle, cid):
    case = GC.BY_ID[cid]
    data, ref = GC.reference(case, oracle)
    dinv = GC.jacobi_dinv(data) if case.pre else None
    abi = _GmAbi(hipk, case, data, dinv)
    assert abi.wb % 256 == 0 and abi.wb > 0 and abi.ldv > abi.nnz
    work = Arena(DEV, abi.wb, 256, guard_bytes_for(abi.n, 8))
    x_pads0 = _bits(abi.x_start[:, abi.n:])

    def run(i):
        rc, st = abi.call(work.data_ptr(), abi.wb)
        assert rc == 0, hipk.lib().hipk_last_error().decode()
        assert hipk.last_solve_path() == case.path
        res = abi.result(st)
        assert res["x pads"] == x_pads0, "pad elements of X were written"
        if case.special == "zero":      # NaNs may differ in sign and payload between two runs no more than between two machines
            res = {"x": res["x"], "x pads": res["x pads"]}
        return res

    res = run_states(work, abi.guarded(), abi.readonly(), run, label=cid)[0]
    X = np.frombuffer(res["x"], dtype=data["B"].dtype).reshape(case.S, abi.n)
    for s, r in enumerate(ref):
        assert _same(X[s], r.x.astype(X.dtype)), (cid, s)


def test_abi_one_workspace_shared_with_cg_and_bicgstab_and_a_side_stream(hipk, oracle):
    gm_case = GC.BY_ID["gmres-f64-257x1-r9-i-S4-x0none"]
    others = [BC.BY_ID[i] for i in ("cg-jac-f64-16x16-S4-x0none", "bicgstab-f64-683x3-S5-x0none")]
    runs = []
    data, ref = GC.reference(gm_case, oracle)
    runs.append((gm_case, _GmAbi(hipk, gm_case, data, None), ref))
    for c in others:
        data, ref = BC.reference(c, oracle)
        runs.append((c, _Abi(hipk, c, data, BC.jacobi_dinv(data) if c.pre else None), ref))
    runs = [runs[1], runs[0], runs[2]]                                   # cg, gmres, bicgstab
    wb = max(a.wb for _, a, _ in runs)
    work = Arena(DEV, wb, 256, guard_bytes_for(2049, 8)).fill(0xA5)
    side = torch.cuda.Stream()
    for rnd in range(2):
        for c, abi, ref in runs:
            for a in abi.readonly().values():
                a.snapshot()
            if rnd == 1:
                torch.cuda.synchronize()
                rc, st = abi.call(work.data_ptr(), abi.wb, stream=side.cuda_stream)
            else:
                rc, st = abi.call(work.data_ptr(), abi.wb)
            assert rc == 0, hipk.lib().hipk_last_error().decode()
            check_memory(dict(abi.guarded(), work=work), abi.readonly(), f"{c.id} round {rnd}")
            X = abi.x_rows()
            for s, r in enumerate(ref):
                assert _bits(X[s, :abi.n]) == _bits(r.x.astype(X.dtype)) and st[s].iterations == r.iterations, (c.id, rnd, s)


def test_abi_accepts_rows_of_exactly_32_entries(hipk, oracle):
    case = GC.BY_ID["gmres-f64-dense32-rev-r8-i-S2-x0none"]
    data, ref = GC.reference(case, oracle)
    check_abi_accepts_dense32(hipk, case, data, ref, _GmAbi(hipk, case, data, None))


def test_abi_error_codes_write_nothing(hipk, oracle):
    case = GC.BY_ID["gmres-f64-17x15-r7-i-S5-x0exact"]
    data, _ = GC.reference(case, oracle)
    abi = _GmAbi(hipk, case, data, None)
    work = Arena(DEV, abi.wb, 256, guard_bytes_for(abi.n, 8)).fill(0x3C)
    work.snapshot()
    for a in abi.readonly().values():
        a.snapshot()

    def untouched(when):
        check_memory(dict(abi.guarded(), work=work), dict(abi.readonly(), work=work), when)
        assert _bits(abi.x_rows()) == _bits(abi.x_start), f"{when}: X was written"

    rc, _ = abi.call(work.data_ptr(), abi.wb, ldb=abi.ldb + 1)
    assert rc == -3, rc                                    # HIPK_ERR_ALIGN
    untouched("misaligned ldb")
    rc, _ = abi.call(work.data_ptr(), abi.wb - 256)
    assert rc == -5, rc                                    # HIPK_ERR_WORKSPACE
    untouched("short work")
    rc, _ = abi.call(work.data_ptr(), 1 << 40, n=4097)
    assert rc == -4, rc                                    # HIPK_ERR_UNSUPPORTED: n beyond the envelope
    untouched("n = 4097")
    for restart in (0, 32):
        rc, _ = abi.call(work.data_ptr(), 1 << 40, restart=restart)
        assert rc == -4 and "[1, 31]" in hipk.lib().hipk_last_error().decode(), (restart, rc)
        untouched(f"restart = {restart}")
    # a 33-entry row: dense 33 x 33 pattern
    n = 33
    crow, col = BC._dense_pattern(n)
    vals = (np.eye(n) * 40.0 + 0.5)[None].repeat(2, 0).reshape(2, -1)
    d33 = {"crow": crow, "col": col, "vals": vals, "B": np.ones((2, n)), "X0": None, "n": n, "nnz": n * n}
    c33 = GC.Case(id="dense33", dtype="f64", pre=False, restart=5, method="batched", dense=33, S=2)
    abi33 = _GmAbi(hipk, c33, d33, None)
    work33 = Arena(DEV, abi33.wb, 256, guard_bytes_for(n * n, 8))
    for a in abi33.readonly().values():
        a.snapshot()
    work33.fill(0x3C).snapshot()
    rc, _ = abi33.call(work33.data_ptr(), abi33.wb)
    assert rc == -4 and "32 stored entries" in hipk.lib().hipk_last_error().decode(), rc
    check_memory(dict(abi33.guarded(), work=work33), dict(abi33.readonly(), work=work33), "33-entry row")
    assert _bits(abi33.x_rows()) == _bits(abi33.x_start)
