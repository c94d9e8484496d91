"""Neighbours in a batch must not notice: cg_batch, bicgstab_batch and gmres_batch solve eight systems on one pattern of 28 rows
(a 7 x 4 grid), one workgroup per system in ONE launch.  System 3 is then given values at 2^700 or 2^-300 (fp32 storage: 2^100,
2^-100) or a NaN in its right-hand side, and the batch is solved again: every other system must be, bit for bit, what it was in the
batch without the special system -- x, iterations, matvecs, info, breakdown and the norms.  That comparison is device against
device.  System 3 itself is held against its own oracle solve (NaNs in equal places: the sign and payload of a produced NaN are the
implementation's, as tests/test_gpu_gmres_batch.py has it) and must differ from what it was, so that the case is not vacuous."""
import numpy as np
import pytest
import torch

import _batch_cases as BC
import _gmres_batch_cases as GC
import test_gpu_batch as TB
import test_gpu_gmres_batch as TG

pytestmark = pytest.mark.gpu
WHO, S_ALL = 3, 8
KINDS = ("A-up", "A-down", "nan-b")
EXP = {"f64": (700, -300), "f32": (100, -100)}
NORMS = ("recurrence_rs", "residual_norm", "x_norm", "b_norm", "threshold")


def _case(solver, dtype, pre):
    if solver == "gmres":
        return GC.Case(id=f"special-gmres{'-jac' if pre else ''}-{dtype}", dtype=dtype, pre=pre, restart=5, method="batched", grid=(7, 4),
                       S=S_ALL, kwargs={"maxiter": 2})
    return BC.Case(id=f"special-{solver}{'-jac' if pre else ''}-{dtype}", solver=solver, dtype=dtype, pre=pre, grid=(7, 4), S=S_ALL,
                   kwargs={"maxiter": 12})


def _per_system(st, X, s):
    out = [np.ascontiguousarray(X[s]).tobytes(), (st.iterations[s], st.matvecs[s], st.info[s], st.breakdown[s])]
    for name in NORMS:
        if hasattr(st, name):
            out.append(np.float64(getattr(st, name)[s]).tobytes())
    return out


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("pre", [False, True], ids=["plain", "jacobi"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("solver", ["cg", "bicgstab", "gmres"])
def test_batch_neighbours_of_a_special_system(hipk, oracle, solver, dtype, pre, kind):
    case = _case(solver, dtype, pre)
    T, C = (TG, GC) if solver == "gmres" else (TB, BC)
    data = C.build(case)
    assert data["n"] == 28 and data["vals"].shape[0] == S_ALL
    ops = T._operands(case, data)
    X0, info0, st0 = T._solve(case, ops, "kernel")
    assert hipk.last_solve_path() == case.path and st0.launches == 1
    X0 = X0.cpu().numpy()
    base = [_per_system(st0, X0, s) for s in range(S_ALL)]

    poisoned = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in data.items()}
    if kind == "nan-b":
        poisoned["B"][WHO, 11] = np.nan
    else:
        e = EXP[dtype][0 if kind == "A-up" else 1]
        poisoned["vals"][WHO] = np.ldexp(poisoned["vals"][WHO], e).astype(poisoned["vals"].dtype)
    ops = T._operands(case, poisoned)
    print("batch special case", case.id, kind, flush=True)
    X1, info1, st1 = T._solve(case, ops, "kernel")
    assert hipk.last_solve_path() == case.path and st1.launches == 1
    X1 = X1.cpu().numpy()
    for s in range(S_ALL):
        got = _per_system(st1, X1, s)
        if s != WHO:
            assert got == base[s], f"{case.id} {kind}: system {s} noticed system {WHO}: {got[1]} was {base[s][1]}"
    assert _per_system(st1, X1, WHO) != base[WHO], "the special system solved as the ordinary one: the case is vacuous"
    # the special system against its own oracle solve, with the Jacobi vector the solve used
    dinv = ops[3].dinv.cpu().numpy() if pre else None
    with np.errstate(all="ignore"):
        ref = C.oracle_run(case, poisoned, oracle, dinv=dinv)[WHO]
    got = (st1.iterations[WHO], st1.matvecs[WHO], st1.info[WHO], st1.breakdown[WHO])
    print("  system", WHO, got, "| oracle", (ref.iterations, ref.matvecs, ref.info, ref.breakdown), flush=True)
    assert got == (ref.iterations, ref.matvecs, ref.info, ref.breakdown), (case.id, kind)
    assert TG._same(X1[WHO], ref.x.astype(X1.dtype)), (case.id, kind)
