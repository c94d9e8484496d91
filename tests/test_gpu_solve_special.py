"""Every form a single-device solve can finish in, in every regime of tests/_special_cases.py: operands scaled by powers of two
up to overflow, underflow and subnormal products, and right-hand sides with a NaN, an infinity or a chunk of zeros.  These are the
branches tame inputs never take: each loop form's own copy of the stop test, of the breakdown tests and of the iteration-0 exits.

Rows: for every distinct form of tests/_form_cases.CASES and of the mid table (tests/test_gpu_mid_oracle.py) the first row that
reports it, with the row's own tol and switches, maxiter capped at 12 (GMRES: two cycles).  tests/test_special_cases.py shows
without a GPU that the oracle reaches the regime's branch on every (row, regime) run here.  Each case asserts

  * the path and form of the row: a power-of-two scale changes neither the pattern nor the number of distinct values, so the
    dispatch does not move (GMRES tests its start on the host: where no cycle runs it reports its launch sequence,
    _special_cases.gmres_idle_form);
  * x as bytes, iterations, matvecs, info, breakdown and the bit patterns of the returned stats equal to the oracle's (the
    callback-M rows of GMRES: counts equal, NaN and zero masks equal, finite x to 1e-9, as tests/test_gpu_solver_forms.py).
    Every NaN counts as ONE pattern (_canon): IEEE 754 leaves the sign and payload of a NaN an operation produces to the
    implementation, and gfx950 and the oracle's host differ there -- measured on the first run of this file: where A p overflows
    the device's x is 0x7FF8... and the oracle's 0xFFF8..., with a NaN in b it is the other way round (a negation of the NaN
    in forming b - A x).  The positions of the NaNs and every bit of every other value count;
  * in the exact-multiple regimes, x bitwise 2^k times the plain run of the same row on the same device with equal counts --
    a check that does not go through the oracle at all.

Every solve runs through tests/_solve_runner.py (guarded arenas of exactly the stated sizes) in two workspace states.  Every case
has a small finite maxiter; its id is printed before the solve (-s: which case a hang is in)."""
import numpy as np
import pytest
import torch

import _form_cases as FC
import _special_cases as S
import test_gpu_mid_oracle as MO
from _arena import FILLS_SHORT
from _solve_runner import STAT_FIELDS, build_case, run_solve_case, stat_bits

pytestmark = pytest.mark.gpu


def _canon(a):
    a = np.array(a, copy=True)
    a[np.isnan(a)] = np.nan
    return a


def _stats(st, skip=None):
    """stat_bits with every NaN as one pattern (skip: a field left out)."""
    class C:
        pass
    c = C()
    for f in STAT_FIELDS:
        v = getattr(st, f)
        setattr(c, f, 0.0 if f == skip else float("nan") if isinstance(v, float) and v != v else v)
    return stat_bits(c)


DEV = "cuda:0"
ROWS = S.form_rows(FC.CASES, MO.CASES)
PARAMS = [(row, reg, ea, eb) for row in ROWS for reg, ea, eb in S.row_regimes(row)]
_base, _plain = {}, {}


def _base_matrix(table, key, dt):
    if (table, key) not in _base:
        _base[(table, key)] = (FC.MATRICES if table == "form" else MO.MATRICES)[key]()
    M = _base[(table, key)].copy()
    M.data = M.data.astype(dt)
    return M


def _device_matrix(M0, vals):
    """matrix(key, dt) for build_case: M0's pattern with `vals`, and a fresh device tensor (so a fresh handle)."""
    def matrix(key, dt):
        M = M0.copy()
        M.data = vals
        A = torch.sparse_csr_tensor(torch.from_numpy(M.indptr.astype(np.int64)), torch.from_numpy(M.indices.astype(np.int64)),
                                    torch.from_numpy(M.data), size=M.shape).to(DEV)
        return M, A
    return matrix


def _run(hipk, row, M0, vals, b, x0, dinv, kw, path, form, tag):
    cid, solver, key, table, dtn, _, env, x0kind = row[:8]
    dt = M0.data.dtype
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        M, h, b_row, x0_row, _ = build_case(hipk, _device_matrix(M0, vals), cid, solver, key, dt, x0kind)
    print("solve special case", tag, flush=True)
    st, x, bd = run_solve_case(hipk, tag, solver, h, b, x0, dinv, kw, path, form, FILLS_SHORT)
    assert bd.cpu().numpy().tobytes() == b.tobytes(), tag
    return M, st, x, (b_row, x0_row)


@pytest.mark.parametrize("row, reg, ea, eb", PARAMS, ids=[f"{p[0][0]}/{p[1][0]}" for p in PARAMS])
def test_solve_form_in_regime(hipk, oracle, monkeypatch, row, reg, ea, eb):
    cid, solver, key, table, dtn, kw, env, x0kind, path, form = row
    dt = np.float64 if dtn == S.F64 else np.float32
    for k, v in env.items():     # before the handle exists
        monkeypatch.setenv(k, v)
    M0 = _base_matrix(table, key, dt)
    n = M0.shape[0]
    pre = solver in ("pcg", "pbicgstab", "pgmres")
    callback = bool(kw.get("callback"))
    b, x0 = S.row_vectors(cid, n, dt, x0kind)
    vals, bs, x0s, dinv = S.operands(M0, b, x0, pre, reg, ea, eb)
    kwr = S.regime_kw(solver, kw, reg)
    branch = reg[5][solver]
    tag = f"{cid}/{reg[0]}"
    want_path, want_form = path, form
    if solver in ("gmres", "pgmres") and branch == "it0":     # no cycle ran
        want_path, want_form = FC.LS, S.gmres_idle_form(n, kw, env)
    M, st, x, drawn = _run(hipk, row, M0, vals, bs, x0s, dinv, kwr, want_path, want_form, tag)
    assert np.array_equal(drawn[0], b) and (x0 is None) == (drawn[1] is None), tag      # the row's own b and x0, as build_case draws them

    ref = S.oracle_solve(oracle, solver, M, vals, dinv, bs, x0s, kwr)
    got = (st.iterations, st.matvecs, st.info, st.breakdown)
    want = (ref.iterations, ref.matvecs, ref.info, ref.breakdown)
    print("  iterations, matvecs, info, breakdown", got, "| oracle", want, "| nan", int(np.isnan(x).sum()), "zero", int((x == 0).sum()), flush=True)
    start = np.zeros(n, dt) if x0s is None else x0s
    if callback and solver == "pgmres":
        assert got[:3] == want[:3], (tag, got, want)
        assert np.array_equal(np.isnan(x), np.isnan(ref.x)) and np.array_equal(x == 0, ref.x == 0), tag
        fin = np.isfinite(ref.x)
        assert np.array_equal(np.isfinite(x), fin), tag
        if fin.any():
            k = eb - ea
            a, w = np.ldexp(x[fin].astype(np.float64), -k), np.ldexp(ref.x[fin].astype(np.float64), -k)
            assert np.linalg.norm(a - w) <= 1e-9 * np.linalg.norm(w), tag
    else:
        assert got == want, (tag, got, want)
        assert _canon(x).tobytes() == _canon(ref.x).tobytes(), (tag, int(np.sum(S._bits(_canon(x)) != S._bits(_canon(ref.x)))))
        shown = (tag, [(f, getattr(st, f), getattr(ref, f)) for f in ("b_norm", "residual_norm", "x_norm", "threshold", "recurrence_rs")])
        if callback:
            # BiCGStab with M through the callback: ||M (b - A x)||^2 is a chunked dot of the stored M(.) (hipk_launch_dot_parts in
            # finish()), the oracle's Jacobi form a tiled one fused into the SpMV.  Both sum the same n non-negative squares in
            # fp64, each within gamma_n = n 2^-53 of the exact sum, the square root halves that: |difference| <= n 2^-53 ||r||.
            # First run of this file: one ulp apart on pbicgstab-callback-small-f64/ap-overflow, equal on the other 19 cases.
            a, w = st.residual_norm, ref.residual_norm
            assert a == w or (a != a and w != w) or abs(a - w) <= n * 2.0 ** -53 * abs(w), shown
            assert _stats(st, skip="residual_norm") == _stats(ref, skip="residual_norm"), shown
        else:
            assert _stats(st) == _stats(ref), shown
        # the regime reached its branch on the DEVICE's numbers too (the plain run: the device's own, below)
        if branch not in S.NEEDS_PLAIN:
            assert S.BRANCHES[branch](st_result(st, x), None, start, kwr["maxiter"], eb - ea), (tag, branch)

    if branch in S.NEEDS_PLAIN:
        # x is 2^k times the plain run of the same row on the same device: no oracle in this comparison
        if cid not in _plain:
            d0 = (1.0 / M0.diagonal().astype(np.float64)).astype(dt) if pre else None
            _, pst, px, _ = _run(hipk, row, M0, M0.data, b, x0, d0, S.capped(solver, kw), path, form, f"{cid}/plain")
            _plain[cid] = (pst, px)
        pst, px = _plain[cid]
        k = eb - ea
        if callback and solver == "pgmres":
            # the same kernels and the same M(v) = dinv * v in the same order on data scaled by a power of two: an exact multiple,
            # device against device, although the oracle comparison of these rows is to 1e-9
            assert (st.iterations, st.matvecs) == (pst.iterations, pst.matvecs), tag
            assert np.isfinite(x).all() and S._same_bits(x, np.ldexp(px, k).astype(px.dtype)), tag
        else:
            assert S.BRANCHES[branch](st_result(st, x), st_result(pst, px), start, kwr["maxiter"], k), \
                (tag, branch, got, (pst.iterations, pst.matvecs, pst.info, pst.breakdown))


class st_result:
    """A device solve in the shape of an OracleResult, for the branch predicates."""

    def __init__(self, st, x):
        self.x, self.info, self.iterations, self.matvecs, self.breakdown = x, st.info, st.iterations, st.matvecs, st.breakdown


# ---------------------------------------------------------------------------------------------- the fused CG launch
FUSE_REGIMES = [S.regime(name, S.F64) for name in S.REGIME_NAMES[S.F64]]
_fuse_plain = {}


def _fused_solve(hipk, system, vals, b, kw):
    """One CG solve of the 1025 x 1024 Poisson system (513 chunks: the smallest the fused launch takes) with `vals` on a fresh
    handle; (x, stats, kernel note, form, path, fused directions, kept p)."""
    A = system[0]
    h = hipk.CsrHandle(A.crow_indices(), A.col_indices(), torch.from_numpy(vals).to(DEV), A.shape)
    try:
        bd = torch.from_numpy(b).to(DEV)
        x = torch.zeros_like(bd)
        st = hipk.solve("cg", h, bd, x, atol=0.0, **kw)
        return (x.cpu().numpy(), st, hipk.CsrHandle.last_spmv_kernel(), hipk.last_solve_form(), hipk.last_solve_path(),
                hipk.last_cg_fused_directions(), hipk.last_cg_fused_kept_p())
    finally:
        h.close()


@pytest.mark.parametrize("reg", FUSE_REGIMES, ids=[r[0] for r in FUSE_REGIMES])
def test_fused_cg_launch_in_regime(hipk, oracle, monkeypatch, reg):
    """The fused SpMV + update + direction launch (form "cg three-launch", 513 chunks) with the assertions of
    tests/test_gpu_cg_fuse_collectors.py: every iteration that ran took the fused launch's tail and kept p on chip."""
    import test_gpu_cg_fuse_update as fu
    for k in fu.SWITCHES + ("HIPK_CG_FUSE_DIRECTION", "HIPK_CG_FUSE_KEEP_P", "HIPK_TEST_CG_FUSE_DIR_GIVE_UP", "HIPK_TEST_CG_FUSE_GIVE_UP_WHO"):
        monkeypatch.delenv(k, raising=False)
    system = fu._poisson(1025, 1024)
    crow, col, val = system[1:]
    n = len(crow) - 1
    assert (n + 2047) // 2048 == 513
    b = np.random.default_rng(21).standard_normal(n)
    M = S_csr(crow, col, val)
    vals, bs, _, _ = S.operands(M, b, None, False, reg)
    kw = S.regime_kw("cg", dict(tol=1e-8, maxiter=S.MAXITER_CAP), reg)
    print("fused cg special case", reg[0], flush=True)
    x, st, note, form, path, fused, kept = _fused_solve(hipk, system, vals, bs, kw)
    oracle.set_threads(16)
    try:
        ref = oracle.cg(crow, col, vals, bs, tol=kw["tol"], atol=0.0, maxiter=kw["maxiter"])
    finally:
        oracle.set_threads(1)
    got, want = (st.iterations, st.matvecs, st.info, st.breakdown), (ref.iterations, ref.matvecs, ref.info, ref.breakdown)
    print("  ", got, "| oracle", want, "| note", note, "fused", fused, "kept", kept, flush=True)
    assert (form, path) == (fu.FORM, "launch sequence"), (form, path)
    assert got == want, (got, want)
    assert _canon(x).tobytes() == _canon(ref.x).tobytes(), int(np.sum(S._bits(_canon(x)) != S._bits(_canon(ref.x))))
    assert _stats(st) == _stats(ref)
    assert (fused, kept) == (ref.iterations, ref.iterations), (fused, kept, ref.iterations)
    if ref.iterations > 0:
        assert note == fu.FUSED5, note
    branch = reg[5]["cg"]
    if branch in S.NEEDS_PLAIN:
        if "plain" not in _fuse_plain:
            _fuse_plain["plain"] = _fused_solve(hipk, system, val, b, S.capped("cg", dict(tol=1e-8, maxiter=S.MAXITER_CAP)))
        p = _fuse_plain["plain"]
        assert p[5] == p[1].iterations and p[2] == fu.FUSED5
        assert S.BRANCHES[branch](st_result(st, x), st_result(p[1], p[0]), np.zeros(n), kw["maxiter"], reg[3] - reg[2]), reg[0]
    else:
        assert S.BRANCHES[branch](st_result(st, x), None, np.zeros(n), kw["maxiter"], reg[3] - reg[2]), reg[0]


def S_csr(crow, col, val):
    import scipy.sparse as sp
    n = len(crow) - 1
    return sp.csr_matrix((val, col, crow), shape=(n, n))
