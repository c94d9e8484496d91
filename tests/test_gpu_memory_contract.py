"""The memory contract of include/hipk.h beyond the two solve tables (which run every case through tests/_solve_runner.py):

1. hipk_cheb_apply with its two work vectors, z and r in guarded arenas (tests/_arena.py) of exactly 2 * ((n + 3) & ~3) and n
   elements, in the four workspace states, against tests/_cheb_mirror.py;
2. one workspace reused by twelve solves of different solvers, loop kinds and sizes, back to back and never refilled: each solve is
   given only its own *_work_bytes prefix, leaves the bytes beyond it alone and gives the bits it gives alone;
3. one solve per kind of loop on a stream that is not the default one: the bits, path, form and stats of the default-stream run.

The cases of 2 and 3 are rows of the two tables, by id."""
import numpy as np
import pytest
import torch

import _cheb_cases as C
import test_gpu_mid_oracle as TM
import test_gpu_solver_forms as TF
from _arena import FILLS, Arena, check_memory, guard_bytes_for, run_states
from _cheb_mirror import mirror
from _form_cases import FIXED_B
from _solve_runner import DEV, Operands, build_case, run_solve_in, work_bytes
from test_gpu_coded import make_handle

pytestmark = pytest.mark.gpu

FORM_ROWS = {c[0]: c for c in TF.CASES}
MID_ROWS = {c[0]: (c[0], c[0].split("-")[0]) + c[1:] + (TM.form_of(c[-1]),) for c in TM.CASES}   # (+ solver, form)


# ---------------------------------------------------------------------------------------------- 1. hipk_cheb_apply
FIVE_POINT = [(0, -1), (-1, 0), (0, 0), (1, 0), (0, 1)]


def _cheb_matrix(n):
    if n == 17 * 13:
        return C.grid_stencil(17, 13, FIVE_POINT, 4.5) + (4.5,)
    return C.band(n, C.SMALL_OFFSETS)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("n", [1, 255, 2049, 17 * 13])
def test_cheb_apply_in_arenas(hipk, oracle, monkeypatch, n, dtype):
    crow, col, val, diag = _cheb_matrix(n)
    val = val.astype(dtype)
    dinv, r = C.apply_inputs(n, diag, dtype)
    tdt = torch.from_numpy(r).dtype
    item = r.itemsize
    g = guard_bytes_for(n, item)
    za, ra, da = (Arena(DEV, n * item, 16, g) for _ in range(3))
    rd, dd = ra.put(r), da.put(dinv)
    zd = za.view(tdt, n)
    work = Arena(DEV, 2 * ((n + 3) & ~3) * item, 16, g)
    h = make_handle(hipk, crow, col, val, n, dtype=tdt)
    try:
        for degree in (1, 2, 5):
            M, coef = C.apply_coefficients(degree, dinv)
            ref = mirror(oracle, crow, col, val, M, r, dtype=dtype)
            for fused in ("1", "0"):
                monkeypatch.setenv("HIPK_CHEB_FUSED", fused)

                def run(i):
                    za.fill(0xFF)
                    out = hipk.cheb_apply(h, degree, dd, coef, rd, work=work.payload, out=zd)
                    assert out.data_ptr() == zd.data_ptr()
                    return {"z": za.payload.cpu().numpy().tobytes()}
                label = f"hipk_cheb_apply n={n} degree={degree} fused={fused}"
                res = run_states(work, {"z": za, "r": ra, "dinv": da}, {"r": ra, "dinv": da}, run, FILLS, label=label)
                assert res[0]["z"] == ref.tobytes(), label + f" [{hipk.CsrHandle.last_spmv_kernel()}]: not the mirror's bits"
    finally:
        h.close()


# ---------------------------------------------------------------------------------------------- table rows as prepared cases
def _prepare(hipk, row, monkeypatch):
    """(solver, handle, Operands, kw, env, path, form, host arrays) of a table row, built by the table tests' own builder."""
    cid, solver, key, dtn, kw, env, x0kind, path, form = row
    T = TF if cid in FORM_ROWS else TM
    dt = np.float64 if dtn == "f64" else np.float32
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        M, h, b, x0, dinv = build_case(hipk, T._matrix, cid, solver, key, dt, x0kind, FIXED_B)
    finally:
        for k in env:
            monkeypatch.delenv(k)
    n = M.shape[0]
    return dict(cid=cid, solver=solver, h=h, ops=Operands(b, x0, dinv), kw=kw, env=env, path=path, form=form, n=n, dt=dt,
                host=(M, b, x0, dinv))


def _solve(hipk, case, monkeypatch, work_tensor):
    for k, v in case["env"].items():
        monkeypatch.setenv(k, v)
    try:
        return run_solve_in(hipk, case["cid"], case["solver"], case["h"], case["ops"], case["kw"], work_tensor)
    finally:
        for k in case["env"]:
            monkeypatch.delenv(k)


def _alone(hipk, case, monkeypatch):
    """The case in a workspace arena of its own (zero-filled), as its table test's first run: (x bytes, stat bits, path, form)."""
    wb = work_bytes(hipk, case["solver"], case["n"], case["dt"], case["kw"])
    work = Arena(DEV, wb, 256, case["ops"].guard).fill(0x00)
    got = _solve(hipk, case, monkeypatch, work.payload)
    check_memory({"work": work}, {}, case["cid"] + " alone")
    assert got[2] == case["path"] and (case["form"] is None or got[3] == case["form"]), (case["cid"], got[2], got[3])
    return got, wb


# ---------------------------------------------------------------------------------------------- 2. one workspace, many solves
# consecutive solves differ in solver and in loop kind
REUSE = [
    "gmres-w5-non5-f64",              # a GMRES mid loop
    "cg-lds-g1-f64",                  # a CG LDS loop on one XCD
    "bicgstab-w5-non5-f64",           # a BiCGStab mid loop
    "cg2-row32-f64",                  # two-launch CG
    "gmres-big-r64-c1r-f32",          # GMRES, restart above 31
    "pcg-w7-sym7-f64",                # a PCG mid loop
    "bicgstab-spread-far-c32-f64",    # a BiCGStab LDS loop spread over the chip
    "cg-chunks513-f64",               # three-launch CG with the x update deferred (513 chunks: the fourth vector)
    "gmres-lds-not-resident1-f64",    # a hand-back under HIPK_TEST_LDS_NOT_RESIDENT
    "pbicgstab-w9-lap9-f32",          # a Jacobi BiCGStab mid loop, fp32
    "gmres-cycle-small-f64",          # the small GMRES cycle kernel
    "pcg-lds-g1r-f32",                # a Jacobi PCG LDS loop, fp32
]
ORACLE_AGAIN_MAX_N = 20_000   # the oracle runs again where it is cheap; every row is pinned to it by its own table test


def test_one_workspace_reused_across_solvers_and_sizes(hipk, oracle, monkeypatch):
    cases = [_prepare(hipk, FORM_ROWS.get(cid) or MID_ROWS[cid], monkeypatch) for cid in REUSE]
    alone = [_alone(hipk, c, monkeypatch) for c in cases]
    assert cases[7]["n"] > 512 * 2048 and cases[7]["path"] == "launch sequence"
    for c, (got, _) in zip(cases, alone):
        if c["n"] <= ORACLE_AGAIN_MAX_N and not c["kw"].get("callback"):
            M, b, x0, dinv = c["host"]
            fn = getattr(oracle, TF.ORACLE[c["solver"]] + ("32" if c["dt"] == np.float32 else ""))
            okw = dict(x0=x0, tol=c["kw"]["tol"], atol=0.0, maxiter=c["kw"]["maxiter"])
            if c["solver"] in ("gmres", "pgmres"):
                okw.update({k: v for k, v in c["kw"].items() if k in ("restart", "solve_method")}, gpu_tolerances=True)
            ref = fn(*((M.indptr, M.indices, M.data) + ((dinv,) if dinv is not None else ()) + (b,)), **okw)
            assert got[0] == ref.x.astype(c["dt"]).tobytes(), c["cid"]
    biggest = max(wb for _, wb in alone)
    shared = Arena(DEV, biggest, 256, max(c["ops"].guard for c in cases))   # as created: whatever the sentinel stream put there
    for rnd in range(2):      # the second round meets what every OTHER solver left
        for c, (want, wb) in zip(cases, alone):
            beyond = shared.payload[wb:].clone()
            got = _solve(hipk, c, monkeypatch, shared.payload[:wb])
            where = f"{c['cid']} (round {rnd + 1}, {wb} of {biggest} bytes)"
            assert got[2:] == want[2:], (where, got[2:], want[2:])
            assert got[1] == want[1], where + ": stats depend on what the workspace held"
            assert got[0] == want[0], where + ": x depends on what the workspace held"
            assert torch.equal(shared.payload[wb:], beyond), where + ": wrote beyond its work_bytes"
            check_memory({"work": shared}, {}, where)


# ---------------------------------------------------------------------------------------------- 3. not the default stream
# one row per kind of loop (hipk_last_solve_path family / launch-sequence form), the smallest matrix of the tables for each
STREAM = [
    "cg-lds-n35-f64", "bicgstab-lds-n35-f64", "gmres-lds-n35-f64", "gmres-cycle-small-f32",
    "cg-small-row13-f64", "pcg-seq-row13-f64", "bicgstab-small-row13-f64", "gmres-small-row33-f64", "gmres-big-r32-n35-f64",
    "cg-general-row13-c9-f64", "cg2-c33-mid0-f64", "cg-lds-not-resident1-f64",
    "cg-chunks9-f64", "bicgstab-chunks9-f64", "gmres-chunks33-f64", "pbicgstab-callback-small-f64",
]


@pytest.mark.parametrize("cid", STREAM)
def test_solve_on_a_stream_that_is_not_the_default(hipk, monkeypatch, cid):
    case = _prepare(hipk, FORM_ROWS.get(cid) or MID_ROWS[cid], monkeypatch)   # handle and operands: the default stream
    torch.cuda.synchronize()
    want, wb = _alone(hipk, case, monkeypatch)
    work = Arena(DEV, wb, 256, case["ops"].guard).fill(0xFF)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        assert hipk._stream(torch.device(DEV)) == s.cuda_stream != torch.cuda.default_stream().cuda_stream
        got = _solve(hipk, case, monkeypatch, work.payload)
    s.synchronize()
    assert got[2:] == want[2:], (cid, got[2:], want[2:])
    assert got[1] == want[1] and got[0] == want[0], cid + ": not the default-stream run's bits"
    check_memory(dict(case["ops"].guarded, work=work), {}, cid + " on a side stream")
