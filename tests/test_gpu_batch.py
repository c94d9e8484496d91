"""cg_batch / bicgstab_batch on the GPU: every case of tests/_batch_cases.py through the batch kernels (csrc/hipk_batch.hip), bitwise
against the CPU oracle per system; the three routes and the launch budgets agree; the C entry points keep the memory contract."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import _batch_cases as BC
from _arena import Arena, check_memory, guard_bytes_for, run_states
from _oracle_cases import _check_stats_long_double

pytestmark = pytest.mark.gpu
DEV = "cuda"
KERNEL_CASES = [c for c in BC.CASES if c.kernel]
# the loop route runs S single solves per case (the 300- and 1030-system batches included: about a second each)
LOOP_CASES = KERNEL_CASES
PATTERN_KERNEL_CASES = [c for c in BC.PATTERN_CASES if c.kernel]


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _dbits(v):
    return np.float64(v).tobytes()


def _operands(case, data):
    from pytorch_sparse_solver.module_a import BatchedCSR, BatchedJacobiPreconditioner
    A = BatchedCSR(torch.from_numpy(data["crow"]).to(DEV), torch.from_numpy(data["col"]).to(DEV), torch.from_numpy(data["vals"]).to(DEV))
    B = torch.from_numpy(data["B"]).to(DEV)
    X0 = None if data["X0"] is None else torch.from_numpy(data["X0"]).to(DEV)
    M = BatchedJacobiPreconditioner(A) if case.pre else None
    return A, B, X0, M


def _solve(case, ops, route):
    from pytorch_sparse_solver.module_a import bicgstab_batch, cg_batch, get_last_stats
    A, B, X0, M = ops
    fn = cg_batch if case.solver == "cg" else bicgstab_batch
    X, info = fn(A, B, X0, M=M, route=route, **case.solve_kwargs)
    return X, info, get_last_stats()


def _assert_oracle(case, ref, X, info, st):
    assert info.dtype == torch.int64 and info.device.type == "cpu" and tuple(info.shape) == (case.S,)
    Xh = X.cpu().numpy()
    assert Xh.dtype == (np.float64 if case.dtype == "f64" else np.float32)
    for s, r in enumerate(ref):
        where = f"{case.id} system {s}"
        assert (st.iterations[s], st.matvecs[s], st.info[s], st.breakdown[s]) == (r.iterations, r.matvecs, r.info, r.breakdown), \
            (where, (st.iterations[s], st.matvecs[s], st.info[s], st.breakdown[s]), (r.iterations, r.matvecs, r.info, r.breakdown))
        assert int(info[s]) == r.info, where
        assert _bits(Xh[s]) == _bits(r.x.astype(Xh.dtype)), f"{where}: x differs (max {np.abs(Xh[s] - r.x).max():.3e})"
        for name in ("recurrence_rs", "residual_norm", "x_norm", "b_norm", "threshold"):
            assert _dbits(getattr(st, name)[s]) == _dbits(getattr(r, name)), (where, name, getattr(st, name)[s], getattr(r, name))


def _reference(case, oracle, M):
    """The oracle per system, with the Jacobi vectors the solve itself used."""
    data, ref = BC.reference(case, oracle)
    if case.pre:
        dinv = M.dinv.cpu().numpy()
        if _bits(dinv) != _bits(BC.jacobi_dinv(data)):
            ref = BC.oracle_run(case, data, oracle, dinv=dinv)
    return ref


# ------------------------------------------------------------------ every case of the table through the kernel
@pytest.mark.parametrize("case", KERNEL_CASES, ids=lambda c: c.id)
def test_batch_kernel_matches_the_oracle(hipk, oracle, case):
    data, _ = BC.reference(case, oracle)
    ops = _operands(case, data)
    X, info, st = _solve(case, ops, "kernel")
    assert hipk.last_solve_path() == case.path and st.path == case.path and hipk.last_solve_form() == case.path
    assert st.launches == 1
    _assert_oracle(case, _reference(case, oracle, ops[3]), X, info, st)


def test_batched_jacobi_matches_the_single_preconditioner(hipk):
    from pytorch_sparse_solver.module_a import BatchedCSR, BatchedJacobiPreconditioner, JacobiPreconditioner
    for cid in ("cg-jac-f64-16x16-S4-x0none", "bicgstab-jac-f32-16x16-S4-x0none"):
        data = BC.build(BC.BY_ID[cid])
        A = BatchedCSR(torch.from_numpy(data["crow"]).to(DEV), torch.from_numpy(data["col"]).to(DEV), torch.from_numpy(data["vals"]).to(DEV))
        M = BatchedJacobiPreconditioner(A)
        for s in range(A.batch):
            assert torch.equal(M.dinv[s], JacobiPreconditioner(A.system(s)).dinv)


def check_jacobi_vectors_on_repeated_diagonals(data):
    """dinv[s] of the batch preconditioner is bitwise the single one's where a diagonal is stored twice, in both dtypes."""
    from pytorch_sparse_solver.module_a import BatchedCSR, BatchedJacobiPreconditioner, JacobiPreconditioner
    rows = np.repeat(np.arange(data["n"]), np.diff(data["crow"]))
    assert np.bincount(rows[data["col"] == rows]).max() == 2
    for dt in (np.float64, np.float32):
        A = BatchedCSR(torch.from_numpy(data["crow"]).to(DEV), torch.from_numpy(data["col"]).to(DEV),
                       torch.from_numpy(data["vals"].astype(dt)).to(DEV))
        M = BatchedJacobiPreconditioner(A)
        assert M.dinv.dtype == A.dtype and bool(torch.isfinite(M.dinv).all())
        for s in range(A.batch):
            assert torch.equal(M.dinv[s], JacobiPreconditioner(A.system(s)).dinv), (dt, s)


@pytest.mark.parametrize("cid", ["cg-jac-f64-rag31n300-dup_diag-S4-x0random", "cg-f64-rag31n300-dup_shuf-S4-x0none",
                                 "bicgstab-jac-f32-rag31n2049-dup_diag-S4-x0none", "bicgstab-f64-rag31n300-dup_shuf-S4-x0none"])
def test_batched_jacobi_adds_a_diagonal_stored_twice_like_the_single_preconditioner(hipk, oracle, cid):
    check_jacobi_vectors_on_repeated_diagonals(BC.reference(BC.BY_ID[cid], oracle)[0])


def check_stats_in_long_double(case, data, X, st, M, solver):
    """x and the stats of every system against long-double arithmetic on the stored arrays (independent of the oracle, which shares
    the kernels' summation order); the bound is derived in _oracle_cases._check_stats_long_double."""
    n = data["n"]
    Xh = X.cpu().numpy()
    dinv = M.dinv.cpu().numpy() if case.pre else None
    for s in range(case.S):
        A = sp.csr_matrix((data["vals"][s], data["col"], data["crow"]), shape=(n, n))
        one = SimpleNamespace(**{k: getattr(st, k)[s] for k in ("b_norm", "residual_norm", "x_norm", "threshold", "info")})
        _check_stats_long_double(solver, data["vals"].dtype.type, A, dinv[s] if case.pre else None, data["B"][s], Xh[s], one,
                                 case.solve_kwargs)


@pytest.mark.parametrize("case", PATTERN_KERNEL_CASES, ids=lambda c: c.id)
def test_pattern_cases_hold_in_long_double(hipk, oracle, case):
    assert "atol" not in case.kwargs
    data, _ = BC.reference(case, oracle)
    ops = _operands(case, data)
    X, info, st = _solve(case, ops, "kernel")
    assert st.path == case.path
    check_stats_in_long_double(case, data, X, st, ops[3], ("p" if case.pre else "") + case.solver)


# ------------------------------------------------------------------ routes
@pytest.mark.parametrize("case", LOOP_CASES, ids=lambda c: c.id)
def test_loop_and_auto_routes_agree_with_the_kernel(hipk, oracle, case):
    from pytorch_sparse_solver.module_a import batch as batch_mod
    data, _ = BC.reference(case, oracle)
    ops = _operands(case, data)
    Xk, ik, sk = _solve(case, ops, "kernel")
    Xl, il, sl = _solve(case, ops, "loop")
    assert sl.path == "loop" and sl.launches == 0
    Xa, ia, sa = _solve(case, ops, "auto")
    assert sa.path == (case.path if case.S >= batch_mod.BATCH_MIN_SYSTEMS else "loop")
    for X, i, st in ((Xl, il, sl), (Xa, ia, sa)):
        assert torch.equal(X, Xk) and torch.equal(i, ik)
        for name in ("iterations", "matvecs", "info", "breakdown"):
            assert getattr(st, name) == getattr(sk, name), (case.id, name)
        for name in ("recurrence_rs", "residual_norm", "x_norm", "b_norm", "threshold"):
            assert [_dbits(v) for v in getattr(st, name)] == [_dbits(v) for v in getattr(sk, name)], (case.id, name)


@pytest.mark.parametrize("cid", ["cg-f64-7x5-S1030-x0random", "bicgstab-f64-32x32-S300-x0random"])
def test_auto_takes_the_kernel_for_a_large_batch(hipk, oracle, cid):
    from pytorch_sparse_solver.module_a import batch as batch_mod
    case = BC.BY_ID[cid]
    assert case.S >= batch_mod.BATCH_MIN_SYSTEMS
    data, ref = BC.reference(case, oracle)
    X, info, st = _solve(case, _operands(case, data), "auto")
    assert st.path == case.path == hipk.last_solve_path()
    _assert_oracle(case, ref, X, info, st)


def test_auto_switches_exactly_at_batch_min_systems(hipk, oracle, monkeypatch):
    from pytorch_sparse_solver.module_a import batch as batch_mod
    case = BC.BY_ID["cg-f64-17x15-S5-x0exact"]
    data, ref = BC.reference(case, oracle)
    ops = _operands(case, data)
    for least, path in ((5, case.path), (6, "loop")):
        monkeypatch.setattr(batch_mod, "BATCH_MIN_SYSTEMS", least)
        X, info, st = _solve(case, ops, "auto")
        assert st.path == path
        _assert_oracle(case, ref, X, info, st)


def test_outside_the_envelope_auto_loops_and_kernel_raises(hipk, oracle):
    case = next(c for c in BC.CASES if not c.kernel)
    _check_outside(case, oracle, "at most 4096 rows")


@pytest.mark.parametrize("cid", ["cg-f64-dense32-dup-S2-x0none", "bicgstab-f64-dense32-dup-S2-x0none"])
def test_a_row_of_33_entries_auto_loops_and_kernel_raises(hipk, oracle, cid):
    assert {c.id for c in BC.CASES if not c.kernel} == {"cg-f64-17x241-S2-x0none", "cg-f64-dense32-dup-S2-x0none",
                                                        "bicgstab-f64-dense32-dup-S2-x0none"}
    _check_outside(BC.BY_ID[cid], oracle, r"at most 32 stored entries per row \(n = 32, longest row 33\)")


def _check_outside(case, oracle, bound):
    assert not case.kernel
    data, ref = BC.reference(case, oracle)
    ops = _operands(case, data)
    with pytest.raises(ValueError, match=bound):
        _solve(case, ops, "kernel")
    X, info, st = _solve(case, ops, "auto")
    assert st.path == "loop"
    assert [int(i) for i in info] == [r.info for r in ref] and st.iterations == [r.iterations for r in ref]
    for s, r in enumerate(ref):
        assert _bits(X[s].cpu().numpy()) == _bits(r.x)


def test_values_updated_in_place_are_the_values_every_route_solves(hipk, oracle, monkeypatch):
    """nnz = 151 (odd): the kernel route works on a padded copy of `values`, which must follow an in-place update."""
    from pytorch_sparse_solver.module_a import batch as batch_mod
    case = BC.BY_ID["cg-f64-7x5-S4-x0none"]
    data, ref = BC.reference(case, oracle)
    assert data["nnz"] % 2 == 1
    ops = _operands(case, data)
    X, info, st = _solve(case, ops, "kernel")
    _assert_oracle(case, ref, X, info, st)
    new = dict(data, vals=np.ascontiguousarray(data["vals"][::-1] * 1.5))      # other matrices in every slot
    ref2 = BC.oracle_run(case, new, oracle)
    assert [r.iterations for r in ref2] != [r.iterations for r in ref]
    ops[0].values.copy_(torch.from_numpy(new["vals"]).to(DEV))
    monkeypatch.setattr(batch_mod, "BATCH_MIN_SYSTEMS", 2)
    for route, path in (("kernel", case.path), ("loop", "loop"), ("auto", case.path)):
        X, info, st = _solve(case, ops, route)
        assert st.path == path
        _assert_oracle(case, ref2, X, info, st)


# ------------------------------------------------------------------ launch budgets: the resume path
@pytest.mark.parametrize("budget", [7, 1])
@pytest.mark.parametrize("cid", BC.BUDGET_IDS)
def test_bits_do_not_depend_on_the_launch_budget(hipk, oracle, monkeypatch, cid, budget):
    case = BC.BY_ID[cid]
    data, _ = BC.reference(case, oracle)
    ops = _operands(case, data)
    ref = _reference(case, oracle, ops[3])
    monkeypatch.setenv("HIPK_BATCH_LAUNCH_ITS", str(budget))
    X, info, st = _solve(case, ops, "kernel")
    most = max(r.iterations for r in ref)
    assert most > budget, "the case must need more than one launch"
    assert st.launches > 1 and st.launches >= -(-most // budget), (st.launches, most)
    _assert_oracle(case, ref, X, info, st)


# ------------------------------------------------------------------ the C entry points: memory contract
class _Abi:
    """One batch solve at the C level between guards: vals, B, X, dinv with leading dimensions larger than their rows (pads hold a
    pattern), `work` exactly hipk_batch_work_bytes."""

    def __init__(self, hipk, case, data, dinv, extra=(8, 4, 12, 6)):
        self.hipk, self.case, self.data = hipk, case, data
        self.dt = torch.float64 if case.dtype == "f64" else torch.float32
        es = 8 if case.dtype == "f64" else 4
        self.S, self.n, self.nnz = case.S, data["n"], data["nnz"]
        per = 16 // es
        up = lambda v, e: (v + e * per + per - 1) // per * per
        self.ldv, self.ldb, self.ldx, self.ldd = up(self.nnz, extra[0]), up(self.n, extra[1]), up(self.n, extra[2]), up(self.n, extra[3])
        g = guard_bytes_for(max(self.n, self.nnz), es)
        self.method = case.solver
        self.pre = dinv is not None
        self.wb = hipk.batch_work_bytes(self.n, self.nnz, self.S, self.dt, self.method, self.pre)
        mk = lambda ld: Arena(DEV, self.S * ld * es, 16, g)
        self.a_vals, self.a_b, self.a_x = mk(self.ldv), mk(self.ldb), mk(self.ldx)
        self.a_dinv = mk(self.ldd) if self.pre else None
        self.crow = Arena(DEV, (self.n + 1) * 4, 16, g)
        self.col = Arena(DEV, max(self.nnz, 1) * 4, 16, g)
        self.crow.put(data["crow"])
        self.col.put(data["col"] if self.nnz else np.zeros(1, np.int32))
        self.x_start = self._padded(data["X0"] if data["X0"] is not None else np.zeros_like(data["B"]), self.ldx, 3)
        self.a_vals.put(self._padded(data["vals"], self.ldv, 1))
        self.a_b.put(self._padded(data["B"], self.ldb, 2))
        if self.pre:
            self.a_dinv.put(self._padded(dinv, self.ldd, 4))

    def _padded(self, rows, ld, seed):
        """(S, ld) with the rows in front and a seeded pattern (NaNs among it) in the pads."""
        rows = np.asarray(rows)
        out = np.random.default_rng(seed).standard_normal((rows.shape[0], ld)).astype(rows.dtype) * 1e30
        out[:, ld - 1] = np.nan
        out[:, :rows.shape[1]] = rows
        return out

    def guarded(self):
        g = {"vals": self.a_vals, "B": self.a_b, "X": self.a_x, "crow": self.crow, "col": self.col}
        if self.pre:
            g["dinv"] = self.a_dinv
        return g

    def readonly(self):
        r = {"vals": self.a_vals, "B": self.a_b, "crow": self.crow, "col": self.col}
        if self.pre:
            r["dinv"] = self.a_dinv
        return r

    def call(self, work_ptr, work_bytes, stream=None, ldb=None, n=None, tol=None):
        hipk = self.hipk
        L = hipk.lib()
        prm = hipk.Params()
        kw = self.case.solve_kwargs
        prm.tol, prm.atol = float(kw["tol"] if tol is None else tol), float(kw.get("atol", 0.0))
        prm.maxiter = -1 if kw.get("maxiter") is None else int(kw["maxiter"])
        prm.gpu_tolerances = 1
        st = (hipk.Stats * self.S)()
        self.a_x.put(self.x_start)
        fn = getattr(L, f"hipk_{self.method}_solve_batch")
        rc = fn(self.n if n is None else n, self.nnz, self.crow.data_ptr(), self.col.data_ptr(), self.a_vals.data_ptr(), self.ldv,
                self.a_dinv.data_ptr() if self.pre else None, self.ldd if self.pre else 0, self.S, self.a_b.data_ptr(),
                self.ldb if ldb is None else ldb, self.a_x.data_ptr(), self.ldx, hipk._dtype_code(self.dt), work_ptr, work_bytes,
                ctypes.byref(prm), st, hipk._stream(torch.device(DEV)) if stream is None else stream)
        torch.cuda.synchronize()
        return rc, st

    def x_rows(self):
        return self.a_x.view(self.dt, self.S * self.ldx).view(self.S, self.ldx).cpu().numpy()

    def result(self, st):
        X = self.x_rows()
        return {"x": _bits(X[:, :self.n]), "x pads": _bits(X[:, self.n:]),
                "stats": bytes(b"".join(bytes(memoryview(s))[:64] for s in st))}     # everything before solve_ms


ABI_IDS = ["cg-f64-17x15-S5-x0exact", "cg-jac-f32-41x25-S4-x0none", "bicgstab-f64-45x45-S4-x0none", "bicgstab-jac-f64-7x5-S5-x0random",
           "bicgstab-f64-bd-10",
           # rows of 2 to 32 entries, unsorted, a column stored twice; ldv > nnz
           "cg-f64-rag31n300-dup_shuf-S4-x0none", "bicgstab-f64-rag31n300-dup_shuf-S4-x0none"]


@pytest.mark.parametrize("cid", ABI_IDS)
def test_abi_workspace_states_guards_and_pads(hipk, oracle, cid):
    case = BC.BY_ID[cid]
    data, ref = BC.reference(case, oracle)
    dinv = BC.jacobi_dinv(data) if case.pre else None
    abi = _Abi(hipk, case, data, dinv)
    assert abi.wb % 256 == 0 and abi.ldv > abi.nnz
    work = Arena(DEV, abi.wb, 256, guard_bytes_for(abi.n, 8))
    x_pads0 = _bits(abi.x_start[:, abi.n:])

    def run(i):
        rc, st = abi.call(work.data_ptr(), abi.wb)
        assert rc == 0, hipk.lib().hipk_last_error().decode()
        assert hipk.last_solve_path() == case.path
        res = abi.result(st)
        assert res["x pads"] == x_pads0, "pad elements of X were written"
        return res

    res = run_states(work, abi.guarded(), abi.readonly(), run, label=cid)[0]
    X = np.frombuffer(res["x"], dtype=data["B"].dtype).reshape(case.S, abi.n)
    for s, r in enumerate(ref):
        assert _bits(X[s]) == _bits(r.x.astype(X.dtype)), (cid, s)


def test_abi_one_workspace_across_solvers_sizes_and_a_side_stream(hipk, oracle):
    cases = [BC.BY_ID[i] for i in ("cg-jac-f64-16x16-S4-x0none", "bicgstab-f64-683x3-S5-x0none", "cg-f32-7x5-S5-x0none")]
    abis = []
    for c in cases:
        data, _ = BC.reference(c, oracle)
        abis.append(_Abi(hipk, c, data, BC.jacobi_dinv(data) if c.pre else None))
    wb = max(a.wb for a in abis)
    work = Arena(DEV, wb, 256, guard_bytes_for(2049, 8)).fill(0xA5)
    side = torch.cuda.Stream()
    for rnd in range(2):
        for c, abi in zip(cases, abis):
            _, ref = BC.reference(c, oracle)
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


def test_abi_error_codes_write_nothing(hipk, oracle):
    case = BC.BY_ID["cg-f64-17x15-S5-x0exact"]
    data, _ = BC.reference(case, oracle)
    abi = _Abi(hipk, case, data, None)
    work = Arena(DEV, abi.wb, 256, guard_bytes_for(abi.n, 8)).fill(0x3C)
    work.snapshot()
    for a in abi.readonly().values():
        a.snapshot()

    def untouched(when, work_too=True):
        check_memory(dict(abi.guarded(), work=work), dict(abi.readonly(), **({"work": work} if work_too else {})), when)
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
    # a 33-entry row: dense 33 x 33 pattern
    n = 33
    crow, col = BC._dense_pattern(n)
    vals = (np.eye(n) * 40.0 + 0.5)[None].repeat(2, 0).reshape(2, -1)
    d33 = {"crow": crow, "col": col, "vals": vals, "B": np.ones((2, n)), "X0": None, "n": n, "nnz": n * n}
    c33 = BC.Case(id="dense33", solver="cg", dtype="f64", pre=False, dense="spd33", S=2)
    abi33 = _Abi(hipk, c33, d33, None)
    work33 = Arena(DEV, abi33.wb, 256, guard_bytes_for(n * n, 8))
    for a in abi33.readonly().values():
        a.snapshot()
    work33.fill(0x3C).snapshot()
    rc, _ = abi33.call(work33.data_ptr(), abi33.wb)
    assert rc == -4 and "32 stored entries" in hipk.lib().hipk_last_error().decode(), rc
    check_memory(dict(abi33.guarded(), work=work33), dict(abi33.readonly(), work=work33), "33-entry row")
    assert _bits(abi33.x_rows()) == _bits(abi33.x_start)


def check_abi_accepts_dense32(hipk, case, data, ref, abi):
    """The inclusive partner of the 33-entry rejection: every row exactly 32 stored entries, rc 0 and the oracle's bits."""
    assert np.diff(data["crow"]).min() == np.diff(data["crow"]).max() == BC.MAX_ROW
    work = Arena(DEV, abi.wb, 256, guard_bytes_for(abi.n, 8)).fill(0x3C)
    for a in abi.readonly().values():
        a.snapshot()
    rc, st = abi.call(work.data_ptr(), abi.wb)
    assert rc == 0, hipk.lib().hipk_last_error().decode()
    assert hipk.last_solve_path() == case.path
    check_memory(dict(abi.guarded(), work=work), abi.readonly(), case.id)
    X = abi.x_rows()
    for s, r in enumerate(ref):
        assert (st[s].iterations, st[s].matvecs, st[s].info) == (r.iterations, r.matvecs, r.info), (case.id, s)
        assert _bits(X[s, :abi.n]) == _bits(r.x.astype(X.dtype)), (case.id, s)


@pytest.mark.parametrize("cid", ["cg-f64-dense32-rev-S2-x0none", "bicgstab-f64-dense32-rev-S2-x0none"])
def test_abi_accepts_rows_of_exactly_32_entries(hipk, oracle, cid):
    case = BC.BY_ID[cid]
    data, ref = BC.reference(case, oracle)
    check_abi_accepts_dense32(hipk, case, data, ref, _Abi(hipk, case, data, None))


# ------------------------------------------------------------------ a batch solve leaves nothing behind that a single solve reads
def test_single_solves_around_a_batch_solve_report_their_own_path(hipk, oracle):
    from pytorch_sparse_solver.module_a import cg
    case = BC.BY_ID["cg-f64-41x25-S4-x0none"]
    data, ref = BC.reference(case, oracle)
    ops = _operands(case, data)
    A0, b0 = ops[0].system(0), ops[1][0].clone()
    x1, _ = cg(A0, b0, tol=case.solve_kwargs["tol"])
    path1, form1 = hipk.last_solve_path(), hipk.last_solve_form()
    assert "batch" not in path1 and path1 != ""
    _solve(case, ops, "kernel")
    assert hipk.last_solve_path() == case.path
    x2, _ = cg(A0, b0, tol=case.solve_kwargs["tol"])
    assert (hipk.last_solve_path(), hipk.last_solve_form()) == (path1, form1)
    assert torch.equal(x1, x2) and _bits(x1.cpu().numpy()) == _bits(ref[0].x)
