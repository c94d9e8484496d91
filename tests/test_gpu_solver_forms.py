"""Every form a single-device solve can finish in (hipk_last_solve_form, csrc/hipk_forms.h) against the CPU oracle, one case per
row of tests/_form_cases.py: the whole-solve LDS kernels on one XCD and spread over the chip, the small and general launch
sequences, the two-launch CG iteration on both sides of each of its guards, GMRES at restart 32 .. 255.  (The mid loops have
their own table, tests/test_gpu_mid_oracle.py.)  Each case asserts

  * which kind of loop finished the solve (hipk_last_solve_path) and which form of it (hipk_last_solve_form), both written
    literally in the table from reading the dispatch code: a loop whose eligibility test went dead cannot pass as another;
  * x, iterations, matvecs, info and breakdown bitwise equal to the oracle's (NaN patterns included), and b unchanged;
  * the returned stats against a long-double recomputation from the stored A, b and the returned x.

The callback-M cases of GMRES compare as test_gpu_pcg.py's callable-M test does (counts equal, x to 1e-9): their ||M(.)||^2 is
a chunked dot, the oracle's a tiled one.

Every solve runs through tests/_solve_runner.py: the workspace in a guarded arena of exactly *_work_bytes, x, b and dinv in arenas
of exactly n elements, once per workspace state (0x00, 0xFF, 0x5A fill, no refill).  Path, form, guards and read-only operands are
asserted after every run; the 0x00 run feeds the assertions above, the others must equal it bit for bit.  The cases of
TWO_STATES keep the 0x00 and 0xFF runs only."""
import numpy as np
import pytest
import torch

from _arena import FILLS, FILLS_SHORT
from _form_cases import CASES, F64, FIXED_B, MATRICES
from _oracle_cases import _check_stats_long_double
from _solve_runner import build_case, run_solve_case

DEV = "cuda:0"
ORACLE = {"cg": "cg", "pcg": "pcg_jacobi", "bicgstab": "bicgstab", "pbicgstab": "bicgstab_jacobi", "gmres": "gmres",
          "pgmres": "gmres_jacobi"}
# cases whose GPU solve alone takes more than 0.5 s (0.64 and 0.60 s on one MI355X before this runner existed; the next one takes
# 0.47 s): they keep the 0x00 and 0xFF workspace states (at most 10 % of the table)
TWO_STATES = frozenset([
    "pgmres-big-r255-c1r-split-f32",
    "gmres-big-r255-c1r-f32",
])
assert TWO_STATES <= {c[0] for c in CASES} and 10 * len(TWO_STATES) <= len(CASES)
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
    M, h, b, x0, dinv = build_case(hipk, _matrix, cid, solver, key, dt, x0kind, FIXED_B)
    n = M.shape[0]
    pre = dinv is not None
    callback = bool(kw.get("callback"))
    print("solver form case", cid, flush=True)   # (-s: which case a hang is in)
    st, x, bd = run_solve_case(hipk, cid, solver, h, b, x0, dinv, kw, path, form, FILLS_SHORT if cid in TWO_STATES else FILLS)
    assert np.array_equal(bd.cpu().numpy(), b), cid

    fn = getattr(oracle, ORACLE[solver] + ("32" if dt == np.float32 else ""))
    args = (M.indptr, M.indices, M.data) + ((dinv,) if pre else ()) + (b,)
    okw = dict(x0=x0, tol=kw["tol"], atol=0.0, maxiter=kw["maxiter"])
    if solver in ("gmres", "pgmres"):
        okw.update({k: v for k, v in kw.items() if k in ("restart", "solve_method")}, gpu_tolerances=True)
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
