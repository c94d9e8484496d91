"""Every form a single-device solve can finish in (hipk_last_solve_form, csrc/hipk_forms.h) against the CPU oracle, one case per
row of tests/_form_cases.py: the whole-solve LDS kernels on one XCD and spread over the chip, the small and general launch
sequences, the two-launch CG iteration on both sides of each of its guards, GMRES at restart 32 .. 255.  (The mid loops have
their own table, tests/test_gpu_mid_oracle.py.)  Each case asserts

  * which kind of loop finished the solve (hipk_last_solve_path) and which form of it (hipk_last_solve_form), both written
    literally in the table from reading the dispatch code: a loop whose eligibility test went dead cannot pass as another;
  * x, iterations, matvecs, info and breakdown bitwise equal to the oracle's (NaN patterns included), and b unchanged;
  * the returned stats against a long-double recomputation from the stored A, b and the returned x.

The callback-M cases of GMRES compare as test_gpu_pcg.py's callable-M test does (counts equal, x to 1e-9): their ||M(.)||^2 is
a chunked dot, the oracle's a tiled one."""
import zlib

import numpy as np
import pytest
import torch

from _form_cases import CASES, F64, FIXED_B, MATRICES
from _oracle_cases import _check_stats_long_double

DEV = "cuda:0"
ORACLE = {"cg": "cg", "pcg": "pcg_jacobi", "bicgstab": "bicgstab", "pbicgstab": "bicgstab_jacobi", "gmres": "gmres",
          "pgmres": "gmres_jacobi"}
_built = {}


def _matrix(key, dt):
    """(scipy CSR with the stored values, device CSR tensor) for matrix `key` in storage dtype dt (cached per process)."""
    if (key, dt) not in _built:
        if key not in _built:
            _built[key] = MATRICES[key]()
        M = _built[key].copy()
        M.data = M.data.astype(dt)
        A = torch.sparse_csr_tensor(torch.from_numpy(M.indptr.astype(np.int64)), torch.from_numpy(M.indices.astype(np.int64)),
                                    torch.from_numpy(M.data), size=M.shape).to(DEV)
        _built[(key, dt)] = (M, A)
    return _built[(key, dt)]


@pytest.mark.gpu
@pytest.mark.parametrize("cid, solver, key, dtn, kw, env, x0kind, path, form", CASES, ids=[c[0] for c in CASES])
def test_solver_form_vs_oracle(hipk, oracle, monkeypatch, cid, solver, key, dtn, kw, env, x0kind, path, form):
    dt = np.float64 if dtn == F64 else np.float32
    for k, v in env.items():     # before the handle exists
        monkeypatch.setenv(k, v)
    M, A = _matrix(key, dt)
    h = hipk.handle_for(A)
    n = M.shape[0]
    rng = np.random.default_rng(zlib.crc32(cid.encode()))
    x0 = rng.standard_normal(n).astype(dt) if x0kind in ("rand", "exact") else None
    if x0kind == "exact":       # b = A x0 (the library's own product): the loop stops at iteration 0
        b = hipk.spmv(h, torch.from_numpy(x0).to(DEV)).cpu().numpy()
    elif x0kind == "fixture":
        b = FIXED_B[key]().astype(dt)
    else:
        b = rng.standard_normal(n).astype(dt)
    pre = solver in ("pcg", "pbicgstab", "pgmres")
    callback = bool(kw.get("callback"))
    dinv = (1.0 / M.diagonal().astype(np.float64)).astype(dt) if pre else None
    bd = torch.from_numpy(b).to(DEV)
    xd = torch.zeros_like(bd) if x0 is None else torch.from_numpy(x0).to(DEV)
    dd = torch.from_numpy(dinv).to(DEV) if pre else None
    gkw = {k: v for k, v in kw.items() if k in ("restart", "solve_method")}
    print("solver form case", cid, flush=True)   # (-s: which case a hang is in)
    if callback and solver == "pbicgstab":
        st = hipk.solve_bicgstab_callable(h, lambda v: dd * v, bd, xd, tol=kw["tol"], atol=0.0, maxiter=kw["maxiter"])
    elif callback:
        st = hipk.solve_gmres_callable(h, lambda v: dd * v, bd, xd, tol=kw["tol"], atol=0.0, maxiter=kw["maxiter"], **gkw)
    elif not pre:
        st = hipk.solve(solver, h, bd, xd, tol=kw["tol"], atol=0.0, maxiter=kw["maxiter"], **gkw)
    elif solver == "pgmres":
        st = hipk.solve_pgmres(h, dd, bd, xd, tol=kw["tol"], atol=0.0, maxiter=kw["maxiter"], **gkw)
    else:
        st = hipk.solve_pcg(h, dd, bd, xd, tol=kw["tol"], atol=0.0, maxiter=kw["maxiter"], method={"pcg": "cg", "pbicgstab": "bicgstab"}[solver])
    got_path, got_form = hipk.last_solve_path(), hipk.last_solve_form()
    x = xd.cpu().numpy()
    assert got_path == path, (cid, got_path, got_form)
    assert got_form == form, (cid, got_form)
    assert np.array_equal(bd.cpu().numpy(), b), cid

    fn = getattr(oracle, ORACLE[solver] + ("32" if dt == np.float32 else ""))
    args = (M.indptr, M.indices, M.data) + ((dinv,) if pre else ()) + (b,)
    okw = dict(x0=x0, tol=kw["tol"], atol=0.0, maxiter=kw["maxiter"])
    if solver in ("gmres", "pgmres"):
        okw.update(gkw, gpu_tolerances=True)
    oracle.set_threads(16 if n >= 100_000 else 4 if n >= 10_000 else 1)   # (the bits do not depend on it; small systems lose time to threads)
    try:
        ref = fn(*args, **okw)
    finally:
        oracle.set_threads(1)   # (both the fp64 and the fp32 library)
    print("  iterations", st.iterations, "matvecs", st.matvecs, "info", st.info, "breakdown", st.breakdown, "| oracle", ref.iterations,
          ref.matvecs, ref.info, ref.breakdown, flush=True)
    if callback and solver == "pgmres":
        assert (st.iterations, st.matvecs, st.info) == (ref.iterations, ref.matvecs, ref.info), cid
        assert np.linalg.norm(x.astype(np.float64) - ref.x) <= 1e-9 * np.linalg.norm(ref.x), cid
    else:
        assert (st.iterations, st.matvecs, st.info, st.breakdown) == (ref.iterations, ref.matvecs, ref.info, ref.breakdown), \
            (cid, (st.iterations, st.matvecs, st.info, st.breakdown), (ref.iterations, ref.matvecs, ref.info, ref.breakdown))
        assert np.array_equal(x, ref.x, equal_nan=True), cid
    _check_stats_long_double(solver, dt, M, dinv, b, x, st, kw)
