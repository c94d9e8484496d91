"""cg_batch / bicgstab_batch with a BatchedBlockJacobiPreconditioner on the GPU: every case of tests/_bj_batch_cases.py through
hipk_cg_bjbatch_kernel / hipk_bi_bjbatch_kernel (csrc/hipk_batch_bj.hip), bitwise against orc_pcg_blockjacobi resp. the BiCGStab
mirror (tests/_bj_mirror.py) per system with the blocks the preconditioner holds; the three routes and the launch budgets agree
(the loop route is the single solves' callback form, so this pins the two forms to each other); the C entry points keep the memory
contract."""
import ctypes

import numpy as np
import pytest
import torch

import _batch_cases as BC
import _bj_batch_cases as T
from _arena import Arena, check_memory, guard_bytes_for, run_states
from conftest import load_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
STATS = ("recurrence_rs", "residual_norm", "x_norm", "b_norm", "threshold")


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _dbits(v):
    return np.float64(v).tobytes()


def _operands(case, data):
    from pytorch_sparse_solver.module_a import BatchedBlockJacobiPreconditioner, BatchedCSR
    A = BatchedCSR(torch.from_numpy(data["crow"]).to(DEV), torch.from_numpy(data["col"]).to(DEV), torch.from_numpy(data["vals"]).to(DEV))
    B = torch.from_numpy(data["B"]).to(DEV)
    X0 = None if data["X0"] is None else torch.from_numpy(data["X0"]).to(DEV)
    given = torch.from_numpy(T.identity_binv(case.S, data["n"], case.bs, data["vals"].dtype)).to(DEV) if case.identity else None
    M = BatchedBlockJacobiPreconditioner(A, block_size=case.bs, binv=given)
    assert M.binv.is_cuda and M.binv.dtype == A.dtype and M.binv.is_contiguous()
    return A, B, X0, M


def _solve(case, ops, route):
    from pytorch_sparse_solver.module_a import bicgstab_batch, cg_batch, get_last_stats
    A, B, X0, M = ops
    fn = cg_batch if case.solver == "cg" else bicgstab_batch
    X, info = fn(A, B, X0, M=M, route=route, **case.solve_kwargs)
    return X, info, get_last_stats()


_refs = {}


def _reference(case, oracle, M):
    """data and the reference per system with the blocks the solve itself uses (the device's batched inverse need not give the
    bits of the CPU's); once per case."""
    data, binv, ref = T.reference(case, oracle)
    mine = M.binv.cpu().numpy()
    rtol = 1e-4 if case.dtype == "f32" else 1e-10
    assert mine.shape == binv.shape and np.allclose(mine, binv, rtol=rtol, atol=rtol * np.abs(binv).max())
    if _bits(mine) != _bits(binv):
        key = (case.id, _bits(mine))
        if key not in _refs:
            _refs[key] = T.oracle_run(case, data, oracle, mine)
        ref = _refs[key]
    return data, ref


def _assert_oracle(case, ref, X, info, st):
    assert info.dtype == torch.int64 and info.device.type == "cpu" and tuple(info.shape) == (case.S,)
    Xh = X.cpu().numpy()
    assert Xh.dtype == (np.float64 if case.dtype == "f64" else np.float32)
    for k, r in enumerate(ref):
        where = f"{case.id} system {k}"
        got = (st.iterations[k], st.matvecs[k], st.info[k], st.breakdown[k])
        assert got == (r.iterations, r.matvecs, r.info, r.breakdown), (where, got, (r.iterations, r.matvecs, r.info, r.breakdown))
        assert int(info[k]) == r.info, where
        assert _bits(Xh[k]) == _bits(r.x.astype(Xh.dtype)), f"{where}: x differs (max {np.abs(Xh[k] - r.x).max():.3e})"
        for name in STATS:
            assert _dbits(getattr(st, name)[k]) == _dbits(getattr(r, name)), (where, name, getattr(st, name)[k], getattr(r, name))


def _assert_same(case, a, b):
    (Xa, ia, sa), (Xb, ib, sb) = a, b
    assert torch.equal(Xa, Xb) and torch.equal(ia, ib), case.id
    for name in ("iterations", "matvecs", "info", "breakdown"):
        assert getattr(sa, name) == getattr(sb, name), (case.id, name)
    for name in STATS:
        assert [_dbits(v) for v in getattr(sa, name)] == [_dbits(v) for v in getattr(sb, name)], (case.id, name)


# ------------------------------------------------------------------ every case of the table through the kernel
@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.id)
def test_bj_batch_kernel_matches_the_oracle(hipk, oracle, case):
    ops = _operands(case, T.reference(case, oracle)[0])
    _, ref = _reference(case, oracle, ops[3])
    X, info, st = _solve(case, ops, "kernel")
    assert hipk.last_solve_path() == case.path and st.path == case.path and hipk.last_solve_form() == case.path
    assert st.launches == 1 and "blockjacobi" in st.method
    _assert_oracle(case, ref, X, info, st)


def test_system_of_a_device_preconditioner_shares_its_blocks(hipk, oracle):
    from pytorch_sparse_solver.module_a import BlockJacobiPreconditioner
    case = T.BY_ID["cg-bj3-f32-7x5-S5-x0random"]
    A, B, X0, M = _operands(case, T.reference(case, oracle)[0])
    for s in range(case.S):
        P = M.system(s)
        assert isinstance(P, BlockJacobiPreconditioner) and P.binv.data_ptr() == M.binv[s].data_ptr() and P.block_size == 3
        z = P(B[s])
        from _bj_mirror import block_apply
        assert _bits(z.cpu().numpy()) == _bits(block_apply(oracle, M.binv[s].cpu().numpy(), B[s].cpu().numpy(), np.float32))


# ------------------------------------------------------------------ routes
@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.id)
def test_loop_and_auto_routes_agree_with_the_kernel(hipk, oracle, case):
    from pytorch_sparse_solver.module_a import batch as batch_mod
    ops = _operands(case, T.reference(case, oracle)[0])
    kern = _solve(case, ops, "kernel")
    auto = _solve(case, ops, "auto")
    assert auto[2].path == (case.path if case.S >= batch_mod.BJ_BATCH_MIN_SYSTEMS else "loop")
    _assert_same(case, auto, kern)
    loop = _solve(case, ops, "loop")
    assert loop[2].path == "loop" and loop[2].launches == 0 and "blockjacobi" in loop[2].method
    _assert_same(case, loop, kern)


def test_auto_switches_exactly_at_bj_batch_min_systems(hipk, oracle, monkeypatch):
    from pytorch_sparse_solver.module_a import batch as batch_mod
    case = T.BY_ID["bicgstab-bj4-f64-7x5-S5-x0random"]
    ops = _operands(case, T.reference(case, oracle)[0])
    _, ref = _reference(case, oracle, ops[3])
    monkeypatch.setattr(batch_mod, "BATCH_MIN_SYSTEMS", 1000)        # the other solves' constant has no say
    for least, path in ((5, case.path), (6, "loop")):
        monkeypatch.setattr(batch_mod, "BJ_BATCH_MIN_SYSTEMS", least)
        X, info, st = _solve(case, ops, "auto")
        assert st.path == path
        _assert_oracle(case, ref, X, info, st)


def test_gmres_batch_takes_the_loop_and_has_no_kernel_form(hipk, oracle):
    from pytorch_sparse_solver.module_a import get_last_stats, gmres, gmres_batch
    case = T.BY_ID["bicgstab-bj4-f64-7x5-S5-x0random"]
    A, B, X0, M = _operands(case, T.reference(case, oracle)[0])
    for route in ("loop", "auto"):
        X, info = gmres_batch(A, B, X0, tol=1e-8, restart=10, M=M, route=route)
        assert get_last_stats().path == "loop"
        for s in range(case.S):
            x, i = gmres(A.system(s), B[s].clone(), X0[s].clone(), tol=1e-8, restart=10, M=M.system(s))
            assert torch.equal(X[s], x) and int(info[s]) == int(i) == 0
    with pytest.raises(ValueError, match="the GMRES batch kernel has no block-Jacobi form"):
        gmres_batch(A, B, X0, M=M, route="kernel")


def test_outside_the_envelope_auto_loops_and_kernel_raises(hipk, oracle):
    from pytorch_sparse_solver.module_a import BatchedBlockJacobiPreconditioner, BatchedCSR, cg_batch, get_last_stats
    data = BC.build(next(c for c in BC.CASES if not c.kernel and c.grid))       # n = 4097
    A = BatchedCSR(torch.from_numpy(data["crow"]).to(DEV), torch.from_numpy(data["col"]).to(DEV), torch.from_numpy(data["vals"]).to(DEV))
    B = torch.from_numpy(data["B"]).to(DEV)
    M = BatchedBlockJacobiPreconditioner(A, block_size=4)
    with pytest.raises(ValueError, match="at most 4096 rows"):
        cg_batch(A, B, M=M, route="kernel", maxiter=3)
    cg_batch(A, B, M=M, route="auto", maxiter=3)
    assert get_last_stats().path == "loop"


# ------------------------------------------------------------------ the reference's own block-Jacobi runs
@pytest.mark.parametrize("solver,name,tag,rtol", [("cg", "bj_varpoisson_nx32_bs4", "cg", 1e-8), ("bicgstab", "bj_convdiff_29x31_bs3", "bicgstab", 1e-5)])
def test_a_batch_built_on_a_golden_fixture(hipk, oracle, solver, name, tag, rtol):
    """System 0 is the fixture, systems 1 .. 3 seeded perturbations of its diagonal (SPD stays SPD)."""
    d = load_case(name)
    bs = int(d["binv"].shape[1])
    n = int(d["n"])
    rows = np.repeat(np.arange(n), np.diff(d["crow"]))
    diag = d["col"] == rows
    rng = np.random.default_rng(11)
    vals = np.stack([d["val"]] * 4)
    for s in range(1, 4):
        vals[s, diag] *= 1.0 + 0.1 * s * rng.random(int(diag.sum()))
    B = np.stack([d["b"]] + [rng.standard_normal(n) for _ in range(3)])
    data = {"crow": d["crow"].astype(np.int32), "col": d["col"].astype(np.int32), "vals": np.ascontiguousarray(vals), "B": B, "X0": None,
            "n": n, "nnz": int(d["col"].size)}
    case = T.Case(id=f"golden-{name}", solver=solver, dtype="f64", bs=bs, S=4)
    ops = _operands(case, data)
    ref = T.oracle_run(case, data, oracle, ops[3].binv.cpu().numpy())
    kern = _solve(case, ops, "kernel")
    assert kern[2].path == case.path
    _assert_oracle(case, ref, *kern)
    assert len({r.iterations for r in ref}) >= 2
    x_ref = d[tag + "_x"]
    assert int(kern[1][0]) == 0 and np.linalg.norm(kern[0][0].cpu().numpy() - x_ref) <= rtol * np.linalg.norm(x_ref)
    for route in ("loop", "auto"):
        _assert_same(case, _solve(case, ops, route), kern)


def test_values_updated_in_place_and_a_new_preconditioner_reach_every_route(hipk, oracle, monkeypatch):
    """nnz = 151 (odd): the kernel route works on a padded copy of `values`, which must follow an in-place update."""
    from pytorch_sparse_solver.module_a import BatchedBlockJacobiPreconditioner
    from pytorch_sparse_solver.module_a import batch as batch_mod
    case = T.BY_ID["cg-bj4-f64-7x5-S4-x0none"]
    data = T.reference(case, oracle)[0]
    assert data["nnz"] % 2 == 1
    A, B, X0, M = _operands(case, data)
    _, ref = _reference(case, oracle, M)
    _assert_oracle(case, ref, *_solve(case, (A, B, X0, M), "kernel"))
    new = dict(data, vals=np.ascontiguousarray(data["vals"][::-1] * 1.5))      # other matrices in every slot
    A.values.copy_(torch.from_numpy(new["vals"]).to(DEV))
    M2 = BatchedBlockJacobiPreconditioner(A, block_size=case.bs)
    assert not torch.equal(M2.binv, M.binv)
    ref2 = T.oracle_run(case, new, oracle, M2.binv.cpu().numpy())
    assert [r.iterations for r in ref2] != [r.iterations for r in ref]
    monkeypatch.setattr(batch_mod, "BJ_BATCH_MIN_SYSTEMS", 2)
    for route, path in (("kernel", case.path), ("loop", "loop"), ("auto", case.path)):
        X, info, st = _solve(case, (A, B, X0, M2), route)
        assert st.path == path
        _assert_oracle(case, ref2, X, info, st)


# ------------------------------------------------------------------ launch budgets: the resume path
@pytest.mark.parametrize("budget", [7, 1])
@pytest.mark.parametrize("cid", T.BUDGET_IDS)
def test_bits_do_not_depend_on_the_launch_budget(hipk, oracle, monkeypatch, cid, budget):
    case = T.BY_ID[cid]
    ops = _operands(case, T.reference(case, oracle)[0])
    _, ref = _reference(case, oracle, ops[3])
    monkeypatch.setenv("HIPK_BATCH_LAUNCH_ITS", str(budget))
    X, info, st = _solve(case, ops, "kernel")
    most = max(r.iterations for r in ref)
    assert most > budget, "the case must need more than one launch"
    assert st.launches > 1 and st.launches >= -(-most // budget), (st.launches, most)
    _assert_oracle(case, ref, X, info, st)


# ------------------------------------------------------------------ the C entry points: memory contract
class _Abi:
    """One block-Jacobi batch solve at the C level between guards: vals, B, X with leading dimensions larger than their rows (pads
    hold a pattern), binv with ldbinv = its blocks + 5 elements (so the blocks of systems 1 .. start at odd element offsets: no
    16-byte alignment to lean on), `work` exactly hipk_bj_batch_work_bytes."""

    def __init__(self, hipk, case, data, binv, extra=(8, 4, 12)):
        self.hipk, self.case, self.data = hipk, case, data
        self.dt = torch.float64 if case.dtype == "f64" else torch.float32
        es = 8 if case.dtype == "f64" else 4
        self.S, self.n, self.nnz, self.bs = case.S, data["n"], data["nnz"], case.bs
        per = 16 // es
        up = lambda v, e: (v + e * per + per - 1) // per * per
        self.ldv, self.ldb, self.ldx = up(self.nnz, extra[0]), up(self.n, extra[1]), up(self.n, extra[2])
        self.blocks = binv.shape[1] * self.bs * self.bs
        self.ldbinv = self.blocks + 5
        g = guard_bytes_for(max(self.n, self.nnz, self.ldbinv), es)
        self.method = case.solver
        self.wb = hipk.bj_batch_work_bytes(self.n, self.nnz, self.S, self.dt, self.method, self.bs)
        mk = lambda ld: Arena(DEV, self.S * ld * es, 16, g)
        self.a_vals, self.a_b, self.a_x, self.a_binv = mk(self.ldv), mk(self.ldb), mk(self.ldx), mk(self.ldbinv)
        self.crow = Arena(DEV, (self.n + 1) * 4, 16, g)
        self.col = Arena(DEV, max(self.nnz, 1) * 4, 16, g)
        self.crow.put(data["crow"])
        self.col.put(data["col"])
        self.x_start = self._padded(data["X0"] if data["X0"] is not None else np.zeros_like(data["B"]), self.ldx, 3)
        self.a_vals.put(self._padded(data["vals"], self.ldv, 1))
        self.a_b.put(self._padded(data["B"], self.ldb, 2))
        self.a_binv.put(self._padded(binv.reshape(self.S, -1), self.ldbinv, 4))

    def _padded(self, rows, ld, seed):
        """(S, ld) with the rows in front and a seeded pattern (NaNs among it) in the pads."""
        rows = np.asarray(rows)
        out = np.random.default_rng(seed).standard_normal((rows.shape[0], ld)).astype(rows.dtype) * 1e30
        out[:, ld - 1] = np.nan
        out[:, :rows.shape[1]] = rows
        return out

    def guarded(self):
        return {"vals": self.a_vals, "B": self.a_b, "X": self.a_x, "crow": self.crow, "col": self.col, "binv": self.a_binv}

    def readonly(self):
        return {"vals": self.a_vals, "B": self.a_b, "crow": self.crow, "col": self.col, "binv": self.a_binv}

    def call(self, work_ptr, work_bytes, stream=None, n=None, bs=None, binv="own", ldbinv=None):
        hipk = self.hipk
        prm = hipk.Params()
        kw = self.case.solve_kwargs
        prm.tol, prm.atol = float(kw["tol"]), float(kw.get("atol", 0.0))
        prm.maxiter = -1 if kw.get("maxiter") is None else int(kw["maxiter"])
        prm.gpu_tolerances = 1
        st = (hipk.Stats * self.S)()
        self.a_x.put(self.x_start)
        fn = getattr(hipk.lib(), f"hipk_{self.method}_solve_batch_bj")
        rc = fn(self.n if n is None else n, self.nnz, self.crow.data_ptr(), self.col.data_ptr(), self.a_vals.data_ptr(), self.ldv,
                self.a_binv.data_ptr() if binv == "own" else binv, self.ldbinv if ldbinv is None else ldbinv, self.bs if bs is None else bs,
                self.S, self.a_b.data_ptr(), self.ldb, self.a_x.data_ptr(), self.ldx, hipk._dtype_code(self.dt), work_ptr, work_bytes,
                ctypes.byref(prm), st, hipk._stream(torch.device(DEV)) if stream is None else stream)
        torch.cuda.synchronize()
        return rc, st

    def x_rows(self):
        return self.a_x.view(self.dt, self.S * self.ldx).view(self.S, self.ldx).cpu().numpy()

    def result(self, st):
        X = self.x_rows()
        return {"x": _bits(X[:, :self.n]), "x pads": _bits(X[:, self.n:]),
                "stats": bytes(b"".join(bytes(memoryview(s))[:64] for s in st))}     # everything before solve_ms


def _abi(hipk, oracle, cid):
    case = T.BY_ID[cid]
    data, binv, ref = T.reference(case, oracle)
    return case, data, ref, _Abi(hipk, case, data, binv)


ABI_IDS = ["cg-bj4-f64-7x5-S4-x0none", "cg-bj3-f32-257x1-S4-x0none", "bicgstab-bj3-f64-257x1-S4-x0none", "bicgstab-bj4-f32-16x16-S5-x0none-b0",
           "cg-bj3-f64-rag31n2049-dup_shuf", "bicgstab-bj2-f64-bd-10"]


@pytest.mark.parametrize("cid", ABI_IDS)
def test_abi_workspace_states_guards_and_pads(hipk, oracle, cid):
    case, data, ref, abi = _abi(hipk, oracle, cid)
    assert abi.wb % 256 == 0 and abi.ldv > abi.nnz and abi.ldbinv > abi.blocks
    work = Arena(DEV, abi.wb, 256, guard_bytes_for(abi.n, 8))
    x_pads0 = _bits(abi.x_start[:, abi.n:])

    def run(i):
        rc, st = abi.call(work.data_ptr(), abi.wb)
        assert rc == 0, hipk.lib().hipk_last_error().decode()
        assert hipk.last_solve_path() == case.path and hipk.lib().hipk_last_batch_launches() == 1
        res = abi.result(st)
        assert res["x pads"] == x_pads0, "pad elements of X were written"
        return res

    res = run_states(work, abi.guarded(), abi.readonly(), run, label=cid)[0]
    X = np.frombuffer(res["x"], dtype=data["B"].dtype).reshape(case.S, abi.n)
    for s, r in enumerate(ref):
        assert _bits(X[s]) == _bits(r.x.astype(X.dtype)), (cid, s)


def test_abi_one_workspace_shared_with_a_plain_batch_solve_and_a_side_stream(hipk, oracle):
    from test_gpu_batch import _Abi as _PlainAbi
    mine = [_abi(hipk, oracle, i) for i in ("bicgstab-bj4-f64-7x5-S5-x0random", "cg-bj32-f32-11x7-S4-x0none")]
    pc = BC.BY_ID["cg-f64-17x15-S5-x0exact"]
    pdata, pref = BC.reference(pc, oracle)
    plain = _PlainAbi(hipk, pc, pdata, None)
    wb = max([a[3].wb for a in mine] + [plain.wb])
    work = Arena(DEV, wb, 256, guard_bytes_for(2049, 8)).fill(0xA5)
    side = torch.cuda.Stream()
    for rnd in range(2):
        for case, data, ref, abi in mine:
            for a in abi.readonly().values():
                a.snapshot()
            if rnd == 1:
                torch.cuda.synchronize()
                rc, st = abi.call(work.data_ptr(), abi.wb, stream=side.cuda_stream)
            else:
                rc, st = abi.call(work.data_ptr(), abi.wb)
            assert rc == 0, hipk.lib().hipk_last_error().decode()
            check_memory(dict(abi.guarded(), work=work), abi.readonly(), f"{case.id} round {rnd}")
            X = abi.x_rows()
            for s, r in enumerate(ref):
                assert _bits(X[s, :abi.n]) == _bits(r.x.astype(X.dtype)) and st[s].iterations == r.iterations, (case.id, rnd, s)
        rc, st = plain.call(work.data_ptr(), plain.wb)
        assert rc == 0 and hipk.last_solve_path() == pc.path
        X = plain.x_rows()
        for s, r in enumerate(pref):
            assert _bits(X[s, :plain.n]) == _bits(r.x) and st[s].iterations == r.iterations, (pc.id, rnd, s)


def test_abi_error_codes_write_nothing(hipk, oracle):
    case, data, ref, abi = _abi(hipk, oracle, "cg-bj4-f64-7x5-S4-x0none")
    work = Arena(DEV, abi.wb, 256, guard_bytes_for(abi.n, 8)).fill(0x3C)
    work.snapshot()
    for a in abi.readonly().values():
        a.snapshot()

    def untouched(when, rc, want):
        assert rc == want, (when, rc, hipk.lib().hipk_last_error().decode())
        check_memory(dict(abi.guarded(), work=work), dict(abi.readonly(), work=work), when)
        assert _bits(abi.x_rows()) == _bits(abi.x_start), f"{when}: X was written"

    ARG, UNSUPPORTED, WORKSPACE = -1, -4, -5
    untouched("block_size 0", abi.call(work.data_ptr(), abi.wb, bs=0)[0], UNSUPPORTED)
    untouched("block_size 33", abi.call(work.data_ptr(), abi.wb, bs=33)[0], UNSUPPORTED)
    untouched("n = 4097", abi.call(work.data_ptr(), 1 << 40, n=4097)[0], UNSUPPORTED)
    untouched("null binv", abi.call(work.data_ptr(), abi.wb, binv=None)[0], ARG)
    untouched("short ldbinv", abi.call(work.data_ptr(), abi.wb, ldbinv=abi.blocks - 1)[0], ARG)
    untouched("work one byte short", abi.call(work.data_ptr(), abi.wb - 1)[0], WORKSPACE)
    rc, st = abi.call(work.data_ptr(), abi.wb, ldbinv=abi.blocks + 5)
    assert rc == 0 and st[0].iterations == ref[0].iterations
    # a 33-entry row: dense 33 x 33 pattern
    n = 33
    crow, col = BC._dense_pattern(n)
    vals = (np.eye(n) * 40.0 + 0.5)[None].repeat(2, 0).reshape(2, -1)
    d33 = {"crow": crow, "col": col, "vals": vals, "B": np.ones((2, n)), "X0": None, "n": n, "nnz": n * n}
    c33 = T.Case(id="dense33", solver="bicgstab", dtype="f64", bs=4, S=2)
    abi33 = _Abi(hipk, c33, d33, T.identity_binv(2, n, 4, np.float64))
    work33 = Arena(DEV, abi33.wb, 256, guard_bytes_for(n * n, 8))
    for a in abi33.readonly().values():
        a.snapshot()
    work33.fill(0x3C).snapshot()
    rc, _ = abi33.call(work33.data_ptr(), abi33.wb)
    assert rc == UNSUPPORTED and "32 stored entries" in hipk.lib().hipk_last_error().decode(), rc
    check_memory(dict(abi33.guarded(), work=work33), dict(abi33.readonly(), work=work33), "33-entry row")
    assert _bits(abi33.x_rows()) == _bits(abi33.x_start)


# ------------------------------------------------------------------ the existing batch solves are untouched by the new M
def test_plain_and_jacobi_batch_solves_keep_their_kernels_next_to_a_block_solve(hipk, oracle):
    pc = BC.BY_ID["cg-jac-f64-16x16-S4-x0none"]
    pdata, pref = BC.reference(pc, oracle)
    from test_gpu_batch import _assert_oracle as plain_assert, _operands as plain_operands, _reference as plain_reference, _solve as plain_solve
    case = T.BY_ID["cg-bj8-f64-16x16-S5-x0none-b0"]
    _solve(case, _operands(case, T.reference(case, oracle)[0]), "kernel")
    assert hipk.last_solve_path() == case.path
    pops = plain_operands(pc, pdata)
    X, info, st = plain_solve(pc, pops, "kernel")
    assert st.path == pc.path == "hipk_cg_batch_kernel<double,true>"
    plain_assert(pc, plain_reference(pc, oracle, pops[3]), X, info, st)
