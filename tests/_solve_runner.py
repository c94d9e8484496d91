"""The shared runner of the solve tables (tests/test_gpu_solver_forms.py, tests/test_gpu_mid_oracle.py) and of the workspace
reuse and stream tests: one whole solve with every operand in guarded memory (tests/_arena.py).

  * `work` lies in a 256-aligned arena of exactly the library's *_work_bytes; x, b and dinv in 16-aligned arenas of exactly n
    elements;
  * the solve runs once per workspace state (0x00, 0xFF, 0x5A, no refill), every time from the same x0;
  * after every run: hipk_last_solve_path / hipk_last_solve_form equal the expected literals, all guards are intact, b and dinv
    are byte-identical to their snapshots;
  * runs 2 .. 4 equal run 1 in x (as bytes: NaN patterns count) and in the bit patterns of the returned stats.

Run 1 is what the caller compares with the oracle, so every run is pinned to it."""
import struct
import zlib

import numpy as np
import torch

from _arena import FILLS, Arena, check_memory, guard_bytes_for, run_states

DEV = "cuda:0"
PRE = ("pcg", "pbicgstab", "pgmres")
STAT_FIELDS = ("iterations", "matvecs", "info", "breakdown", "b_norm", "residual_norm", "x_norm", "threshold", "recurrence_rs")


def stat_bits(st):
    """The deterministic fields of a SolveStats as bit patterns (a NaN equals itself, -0.0 differs from 0.0)."""
    return struct.pack("<qqii5d", *(getattr(st, f) for f in STAT_FIELDS))


def work_bytes(hipk, solver, n, dt, kw):
    """The library's figure for this solve (dt: numpy dtype): what the wrappers pass as work_bytes (restart: their default is 20)."""
    L, code = hipk.lib(), hipk.HIPK_F64 if np.dtype(dt) == np.float64 else hipk.HIPK_F32
    if solver in ("gmres", "pgmres"):
        return int(L.hipk_gmres_work_bytes(n, int(kw.get("restart", 20)), code))
    return int(getattr(L, f"hipk_{solver}_work_bytes")(n, code))


def call_solve(hipk, solver, h, dd, bd, xd, kw, work):
    """The one hipk.solve* call of a table row, with the caller's workspace."""
    gkw = {k: v for k, v in kw.items() if k in ("restart", "solve_method")}
    common = dict(tol=kw["tol"], atol=0.0, maxiter=kw["maxiter"], work=work)
    if kw.get("callback") and solver == "pbicgstab":   # M is called in place on workspace vectors: views of the arena
        return hipk.solve_bicgstab_callable(h, lambda v: dd * v, bd, xd, **common)
    if kw.get("callback"):
        return hipk.solve_gmres_callable(h, lambda v: dd * v, bd, xd, **common, **gkw)
    if solver not in PRE:
        return hipk.solve(solver, h, bd, xd, **common, **gkw)
    if solver == "pgmres":
        return hipk.solve_pgmres(h, dd, bd, xd, **common, **gkw)
    return hipk.solve_pcg(h, dd, bd, xd, method={"pcg": "cg", "pbicgstab": "bicgstab"}[solver], **common)


def build_case(hipk, matrix, cid, solver, key, dt, x0kind, fixed_b=None):
    """The inputs of a table row, for both table tests and for every test that reruns a row by id: (M, handle, b, x0, dinv) as
    host arrays.  matrix: the table module's _matrix; the row's environment is set by the caller, before the handle exists.
    x0kind: None | "rand" | "exact" (b = A x0) | "consistent" (b = A x_true) | "fixture" (b = fixed_b[key]())."""
    M, A = matrix(key, dt)
    h = hipk.handle_for(A)
    n = M.shape[0]
    rng = np.random.default_rng(zlib.crc32(cid.encode()))
    x0 = rng.standard_normal(n).astype(dt) if x0kind in ("rand", "exact") else None
    if x0kind == "exact":         # the library's own product: the loop stops at iteration 0
        b = hipk.spmv(h, torch.from_numpy(x0).to(DEV)).cpu().numpy()
    elif x0kind == "consistent":  # (the LDC matrix is singular)
        b = (M.astype(np.float64) @ rng.standard_normal(n)).astype(dt)
    elif x0kind == "fixture":
        b = fixed_b[key]().astype(dt)
    else:
        b = rng.standard_normal(n).astype(dt)
    dinv = (1.0 / M.diagonal().astype(np.float64)).astype(dt) if solver in PRE else None
    return M, h, b, x0, dinv


class Operands:
    """x, b and (for the Jacobi forms) dinv of one case in 16-aligned arenas of exactly n elements."""

    def __init__(self, b, x0, dinv):
        n, dt = b.shape[0], b.dtype
        g = guard_bytes_for(n, dt.itemsize)
        self.n, self.dt, self.guard = n, dt, g
        self.x0 = torch.from_numpy(np.zeros(n, dtype=dt) if x0 is None else np.ascontiguousarray(x0, dtype=dt)).to(DEV)
        self.b_arena, self.x_arena = Arena(DEV, n * dt.itemsize, 16, g), Arena(DEV, n * dt.itemsize, 16, g)
        self.bd = self.b_arena.put(b)
        self.xd = self.x_arena.put(self.x0)
        self.guarded = {"x": self.x_arena, "b": self.b_arena}
        self.readonly = {"b": self.b_arena}
        self.dd = None
        if dinv is not None:
            self.d_arena = Arena(DEV, n * dt.itemsize, 16, g)
            self.dd = self.d_arena.put(dinv)
            self.guarded["dinv"] = self.readonly["dinv"] = self.d_arena

    def reset_x(self):
        self.xd.copy_(self.x0)

    def x_bytes(self):
        return self.x_arena.payload.cpu().numpy().tobytes()


def run_solve_case(hipk, cid, solver, h, b, x0, dinv, kw, path, form, fills=FILLS):
    """Run one table row in every workspace state of `fills`; returns (stats, x as numpy, device b) of the 0x00-fill run.
    form None: only required to be the same in every run (the mid table's rows that do not finish in a mid loop)."""
    ops = Operands(b, x0, dinv)
    wb = work_bytes(hipk, solver, ops.n, b.dtype, kw)
    work = Arena(DEV, wb, 256, ops.guard)
    first = {}

    def run(i):
        ops.reset_x()
        st = call_solve(hipk, solver, h, ops.dd, ops.bd, ops.xd, kw, work.payload)
        got_path, got_form = hipk.last_solve_path(), hipk.last_solve_form()
        if i == 0:
            first.update(st=st, form=got_form)
        assert got_path == path, (cid, f"run {i + 1}", got_path, got_form)
        assert got_form == (form if form is not None else first["form"]), (cid, f"run {i + 1}", got_form)
        return {"x": ops.x_bytes(), "stats": stat_bits(st)}

    res = run_states(work, ops.guarded, ops.readonly, run, fills, label=cid)
    x = np.frombuffer(res[0]["x"], dtype=b.dtype).copy()
    return first["st"], x, ops.bd


def run_solve_in(hipk, cid, solver, h, ops, kw, work_tensor):
    """One solve of a prepared case in a workspace the CALLER owns (a prefix of a shared arena, whatever it holds): returns
    (x bytes, stat bits, path, form) after checking the operands' guards and read-only operands."""
    for a in ops.readonly.values():
        a.snapshot()
    ops.reset_x()
    st = call_solve(hipk, solver, h, ops.dd, ops.bd, ops.xd, kw, work_tensor)
    path, form = hipk.last_solve_path(), hipk.last_solve_form()
    check_memory(ops.guarded, ops.readonly, cid)
    return ops.x_bytes(), stat_bits(st), path, form
