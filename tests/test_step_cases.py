"""The step-API case table checked without a GPU (tests/_step_cases.py, run on the device by tests/test_gpu_step_api.py):
  * coverage: every cell of entry point x dtype x chunk_rows, every shape, g_red and special kind the table promises, with the
    entry-point list taken from pytorch_sparse_solver._hipk.SYMBOLS -- a step entry point added without cases fails here;
  * the mirror is right: chained into a loop it reproduces the oracle's whole solves bit for bit, also with the rows split over
    two and three "ranks" on chunk boundaries, and for fp64 it equals tests/dist_cpu_ops.py::OracleOps call for call;
  * the table discriminates: for every mutant of the mirror below (a kernel that is subtly wrong in one decision) at least one case
    gives another result than the true mirror -- the evidence that such a kernel cannot pass the device run."""
import numpy as np
import pytest
import torch

import _step_cases as sc
import _step_mirror as sm
from conftest import load_case
from dist_cpu_ops import OracleOps
from oracle import oracle as O


@pytest.fixture(scope="module", autouse=True)
def _built(oracle):
    return oracle


def step_entry_points():
    """hipk_cg_* / hipk_cgm_* of the symbol list that are neither whole solves nor size queries."""
    from pytorch_sparse_solver import _hipk
    return sorted(s[len("hipk_"):] for s in _hipk.SYMBOLS
                  if s.startswith(("hipk_cg_", "hipk_cgm_")) and "solve" not in s and not s.endswith("_bytes"))


def of(entry=None, dtype=None, ch=None, kind=None):
    return [c for c in sc.CASES if (entry is None or c.entry == entry) and (dtype is None or c.dtype == dtype)
            and (ch is None or c.ch == ch) and (kind is None or kind in c.kinds)]


# ------------------------------------------------------------------------------------------------------------ coverage
def test_every_step_entry_point_has_cases():
    assert step_entry_points() == sorted(sc.ARGS)
    assert sorted(sc.STARTS + sc.PER_ITERATION) == sorted(sc.ARGS)
    assert len({c.id for c in sc.CASES}) == len(sc.CASES)


def test_every_cell_and_shape_is_covered():
    for entry in step_entry_points():
        for dtype in sc.DTYPES:
            for ch, ns in sc.SHAPES.items():
                cell = of(entry, dtype, ch)
                assert {c.n for c in cell} >= set(ns), (entry, dtype, ch)
                assert {sm.local_chunks(c.n, ch) for c in cell} >= {1, 2, 3}, (entry, dtype, ch)
                assert of(entry, dtype, ch, "tail_loop") or ch == 2048
            assert of(entry, dtype, 4096, "tail_loop") and of(entry, dtype, 8192, "tail_loop")
            assert any(c.n == 2049 for c in of(entry, dtype, 4096))      # the first step of the tail loop
            for gk in sc.G_KINDS:
                assert of(entry, dtype, kind=gk), (entry, dtype, gk)
            ragged = {c.n % sm.vec_width(dtype) for c in of(entry, dtype, kind="ragged")}
            assert ragged == ({1, 2, 3} if dtype == np.float32 else {1}), (entry, dtype)
    assert sc.SHAPES[2048] == (1, 2, 3, 4, 5, 1023, 1024, 1025, 2047, 2048, 2049, 4097, 6143)
    assert sc.SHAPES[4096] == (2049, 3073, 4095, 4096, 4097, 8195)
    assert sc.SHAPES[8192] == (2049, 8191, 8192, 8193, 16387)
    for c in sc.CASES:
        assert sm.local_chunks(c.n, c.ch) <= c.g <= sm.MAX_PARTS, c.id


def test_every_special_kind_is_covered():
    for dtype in sc.DTYPES:
        for entry in sc.PER_ITERATION:
            for kind in ("parity0", "parity1", "noop_eq", "noop_gt", "nonfinite"):
                assert of(entry, dtype, kind=kind), (entry, dtype, kind)
        for entry in sc.DIRECTIONS:
            for kind in ("maxiter_hit", "maxiter_minus1", "rr_eq", "rr_ulp"):
                assert of(entry, dtype, kind=kind), (entry, dtype, kind)
        for entry in sc.STARTS:
            for kind in ("garbage_block", "maxiter0", "stopped_at_start", "eq_tol", "ulp_tol", "eq_atol", "ulp_atol"):
                assert of(entry, dtype, kind=kind), (entry, dtype, kind)
        for ch in sc.SHAPES:
            assert of("cg_direction", dtype, ch, "split") and of("cg_direction", dtype, ch, "x_null")


def test_the_special_cases_are_what_they_say():
    """The stop decisions the kinds promise, read from the true mirror's scalar block."""
    for c in sc.CASES:
        inp = sc.inputs(c)
        out = sc.expected(c, inp)
        stop = int(sm.stop_word(out["scal"])[0])
        k = c.kinds
        if c.entry in sc.PER_ITERATION:
            assert inp.scal[0] != inp.scal[1]
            assert int(sm.sig_word(inp.scal)[0]) == 0        # hipk_cg_direction dereferences a non-null host_sig
        if k & {"noop_eq", "noop_gt"}:
            assert not sc.same(c, out, sc.outputs(inp.vec, inp.part, inp.scal))
            assert (stop == c.it) == ("noop_eq" in k) and stop <= c.it
        if k & {"maxiter_hit", "rr_eq"}:
            assert stop == c.it + 1, c.id
        if k & {"maxiter_minus1", "rr_ulp"}:
            assert stop == sm.INT64_MAX, c.id
        if k & {"rr_eq", "rr_ulp"}:
            rr = O.reduce_parts(inp.part["part_rr"][:c.g])
            assert (rr == inp.scal[sm.ATOL2]) == ("rr_eq" in k) and np.nextafter(inp.scal[sm.ATOL2], np.inf) >= rr
        if k & {"maxiter0", "stopped_at_start", "eq_tol", "eq_atol"}:
            assert stop == 0, c.id
        if k & {"ulp_tol", "ulp_atol"}:
            assert stop == sm.INT64_MAX, c.id
        if k & {"eq_tol", "ulp_tol", "eq_atol", "ulp_atol"}:
            rr0, bs = O.reduce_parts(inp.part["part_rr"][:c.g]), O.reduce_parts(inp.part["part_bb"][:c.g])
            a2, a3 = sm.squared_f32(c.tol) * bs, sm.squared_f32(c.atol)
            assert (a2 > a3) == bool(k & {"eq_tol", "ulp_tol"})            # which of tol and atol decides
            assert rr0 == (max(a2, a3) if k & {"eq_tol", "eq_atol"} else np.nextafter(max(a2, a3), np.inf))
        if "garbage_block" in k:
            assert np.all(inp.scal.view(np.uint64) == sc.GARBAGE)
            assert out["scal"][sm.GAMMA1] == 0.0 and int(sm.sig_word(out["scal"])[0]) == 0
        if "nonfinite" in k:
            assert not all(np.all(np.isfinite(v)) for v in out.values())
        if c.g > sm.local_chunks(c.n, c.ch):
            for name, p in inp.part.items():
                if name not in sc.OUT_PARTS:
                    assert np.all(p != 0.0) or "nonfinite" in k


def test_split_form_of_the_mirror():
    """hipk_cg_xupdate then hipk_cg_direction(x = NULL) is one hipk_cg_direction."""
    for c in of(kind="split"):
        inp = sc.inputs(c)
        want = sc.expected(c, inp)
        vec = {k: v.copy() for k, v in inp.vec.items()}
        part, scal = inp.part, inp.scal.copy()
        sm.TRUE.cg_xupdate(c.n, c.ch, c.g, scal, c.it, part["part_pAp"], vec["p"], vec["x"])
        sm.TRUE.cg_direction(c.n, c.ch, c.g, scal, c.it, c.maxiter, part["part_pAp"], part["part_rr"], vec["r"], vec["p"], None)
        assert not sc.same(c, sc.outputs(vec, part, scal), want), c.id


# ------------------------------------------------------------------------------------------- the mirror against the oracle
def chained(M, crow, col, val, b, x0, T, cuts, dinv=None, tol=1e-5, atol=0.0, maxiter=None):
    """CG through the mirror's step functions: oracle SpMV with tiled-dot partials (as OracleOps.spmv), the rows split at `cuts`
    (chunk boundaries), every "rank" with its own scalar block, partial outputs all-gathered into the global arrays."""
    f32 = T == np.float32
    spmv, tiled = (O.spmv32, O.dot_tiled_parts_ch32) if f32 else (O.spmv, O.dot_tiled_parts_ch)
    n = b.size
    ch, G = O.chunk_geom(n)
    maxiter = 10 * n if maxiter is None else maxiter
    b, val = b.astype(T), val.astype(T)
    x = np.zeros(n, T) if x0 is None else x0.astype(T)
    edges = [0] + [c * ch for c in cuts] + [n]
    ranks = list(zip(edges[:-1], edges[1:]))
    assert all(lo < hi for lo, hi in ranks)

    def A(v, bsub=None):
        return np.concatenate([spmv(crow[lo:hi + 1] - crow[lo], col[crow[lo]:crow[hi]], val[crow[lo]:crow[hi]], v,
                                    bsub=None if bsub is None else bsub[lo:hi]) for lo, hi in ranks])

    def gathered(fn):
        parts = np.full(sm.MAX_PARTS, np.nan)          # slots past G are never read
        for lo, hi in ranks:
            q = fn(lo, hi)
            assert q.size == sm.local_chunks(hi - lo, ch)
            parts[lo // ch:lo // ch + q.size] = q
        assert not np.any(np.isnan(parts[:G]))
        return parts

    r = A(x, b)
    part_rr = gathered(lambda lo, hi: tiled(r[lo:hi], r[lo:hi], ch))
    part_bb = gathered(lambda lo, hi: sm.dot_parts(b[lo:hi], b[lo:hi], ch))
    p = np.full(n, np.nan, T)
    scals = [np.full(sm.SCAL_WORDS, np.nan) for _ in ranks]
    if dinv is not None:
        dinv = dinv.astype(T)
        z = dinv * r
        part_rz = gathered(lambda lo, hi: sm.dot_parts(r[lo:hi], z[lo:hi], ch))
        for s, (lo, hi) in zip(scals, ranks):
            M.cgm_start(hi - lo, ch, G, s, part_rz, part_rr, part_bb, z[lo:hi], p[lo:hi], tol, atol, maxiter)
    else:
        for s, (lo, hi) in zip(scals, ranks):
            M.cg_start(hi - lo, ch, G, s, part_rr, part_bb, r[lo:hi], p[lo:hi], tol, atol, maxiter)
    it = 0
    while it < sm.stop_word(scals[0])[0]:
        Ap = A(p)
        part_pAp = gathered(lambda lo, hi: tiled(p[lo:hi], Ap[lo:hi], ch))
        outs = []
        for s, (lo, hi) in zip(scals, ranks):
            outs.append(np.full(sm.MAX_PARTS, np.nan))
            M.cg_update(hi - lo, ch, G, s, it, part_pAp, Ap[lo:hi], r[lo:hi], outs[-1])
        todo = iter(outs)
        part_rr = gathered(lambda lo, hi: next(todo)[:sm.local_chunks(hi - lo, ch)])
        if dinv is not None:
            z = dinv * r
            part_rz = gathered(lambda lo, hi: sm.dot_parts(r[lo:hi], z[lo:hi], ch))
            for s, (lo, hi) in zip(scals, ranks):
                M.cgm_direction(hi - lo, ch, G, s, it, maxiter, part_pAp, part_rz, part_rr, z[lo:hi], p[lo:hi], x[lo:hi])
        else:
            for s, (lo, hi) in zip(scals, ranks):
                M.cg_direction(hi - lo, ch, G, s, it, maxiter, part_pAp, part_rr, r[lo:hi], p[lo:hi], x[lo:hi])
        it += 1
        assert all(np.array_equal(sc.bits(s), sc.bits(scals[0])) for s in scals)
    return x, it, int(sm.stop_word(scals[0])[0])


def _golden(name):
    d = load_case(name)
    crow, col, val = d["crow"], d["col"], d["val"]
    n = crow.size - 1
    rows = np.repeat(np.arange(n), np.diff(crow))
    dinv = 1.0 / val[col == rows]
    return crow, col, val, d["b"], (d["x0"] if "x0" in d.files else None), dinv


SOLVES = {("cg", np.float64): O.cg, ("cg", np.float32): O.cg32, ("pcg", np.float64): O.pcg_jacobi, ("pcg", np.float32): O.pcg_jacobi32}


def _against_oracle(crow, col, val, b, x0, dinv, solver, T, cuts, **kw):
    if solver == "pcg":
        ref = SOLVES[solver, T](crow, col, val, dinv, b, x0=x0, **kw)
        x, it, stop = chained(sm.TRUE, crow, col, val, b, x0, T, cuts, dinv=dinv, **kw)
    else:
        ref = SOLVES[solver, T](crow, col, val, b, x0=x0, **kw)
        x, it, stop = chained(sm.TRUE, crow, col, val, b, x0, T, cuts, **kw)
    assert ref.x.dtype == x.dtype == T
    assert (it, stop) == (ref.iterations, ref.iterations)
    assert np.array_equal(sc.bits(x), sc.bits(ref.x))
    return it


@pytest.mark.parametrize("T", sc.DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("solver", ["cg", "pcg"])
@pytest.mark.parametrize("name", ["poisson_nx32", "poisson_17x13", "pcg_varpoisson_nx32"])
def test_chained_mirror_is_the_oracle_solve(name, solver, T):
    crow, col, val, b, x0, dinv = _golden(name)
    assert _against_oracle(crow, col, val, b, x0, dinv, solver, T, (), tol=1e-5) > 5
    assert _against_oracle(crow, col, val, b, x0, dinv, solver, T, (), tol=1e-9, atol=1e-3, maxiter=7) == 7
    assert _against_oracle(crow, col, val, b, x0, dinv, solver, T, (), tol=1e-5, maxiter=0) == 0


@pytest.mark.parametrize("T", sc.DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("solver", ["cg", "pcg"])
@pytest.mark.parametrize("cuts", [(1,), (2,), (1, 2)], ids=["1+2", "2+1", "1+1+1"])
def test_chained_mirror_split_over_ranks(cuts, solver, T):
    """Three reduction chunks (96 x 64 Poisson, 6144 rows): g_red is the global count on every rank."""
    from pytorch_sparse_solver.utils import matrix_utils as mu
    A = mu.create_poisson_2d_csr(96, 64)
    crow, col, val = (t.numpy() for t in (A.crow_indices().to(torch.int32), A.col_indices().to(torch.int32), A.values()))
    rng = np.random.default_rng(96 * 64)
    b = rng.uniform(-1.0, 1.0, 6144)
    dinv = 1.0 / rng.uniform(3.0, 5.0, 6144)          # any positive diagonal M
    assert O.chunk_geom(6144) == (2048, 3)
    assert _against_oracle(crow, col, val, b, None, dinv, solver, T, cuts, tol=1e-4) > 20


def test_mirror_equals_oracle_ops_in_fp64():
    """tests/dist_cpu_ops.py::OracleOps is the fp64 test double the row-partitioned loops are verified with; it has the three
    entry points below (its python-float alpha cannot divide by zero, so the non-finite kind is left out)."""
    ops, seen = OracleOps(), set()
    for c in of(dtype=np.float64):
        if c.entry not in ("cg_start", "cg_update", "cg_direction") or c.x_null or "nonfinite" in c.kinds:
            continue
        inp = sc.inputs(c)
        want = sc.expected(c, inp)
        vec = {k: torch.from_numpy(v.copy()) for k, v in inp.vec.items()}
        part = {k: torch.from_numpy(v.copy()) for k, v in inp.part.items()}
        scal = torch.from_numpy(inp.scal.copy())
        getattr(ops, c.entry)(*sc.call_args(c, vec.__getitem__, part.__getitem__, scal))
        got = sc.outputs({k: v.numpy() for k, v in vec.items()}, {k: v.numpy() for k, v in part.items()}, scal.numpy())
        got["scal"], want["scal"] = got["scal"][:sm.HOST_SIG], want["scal"][:sm.HOST_SIG]   # OracleOps keeps no host_sig word
        assert not sc.same(c, got, want), c.id
        seen.add(c.entry)
    assert seen == {"cg_start", "cg_update", "cg_direction"}


# --------------------------------------------------------------------------------------------------------------- mutants
class OtherParity(sm.Mirror):
    def gamma(self, scal, it):
        return scal[(it + 1) & 1]


class LessThanAtStart(sm.Mirror):
    def stop_at_start(self, maxiter, rr0, atol2):
        return bool(maxiter <= 0 or rr0 < atol2)


class LessThanInDirection(sm.Mirror):
    def stop_next(self, it, maxiter, rr, atol2):
        return bool(it + 1 >= maxiter or rr < atol2)


class OneIterationMore(sm.Mirror):
    def stop_next(self, it, maxiter, rr, atol2):
        return bool(it + 1 > maxiter or rr <= atol2)


class LocalFold(sm.Mirror):
    def fold(self, part, g, n, ch):
        return np.float64(O.reduce_parts(part[:sm.local_chunks(n, ch)]))


class DoubleCoefficients(sm.Mirror):
    """alpha / beta kept in double: the product is formed in fp64 and rounded to T once (fp32 calls only)."""
    def coef(self, v, dtype):
        return np.float64(v)

    def mul(self, c, v):
        return (c * v.astype(np.float64)).astype(v.dtype)


class XReadsNewP(sm.Mirror):
    x_reads_new_p = True


class NoTailLoop(sm.Mirror):
    def touched(self, n, ch, dtype):
        return (np.arange(n) % ch) < sm.BASE_CHUNK


class NoRaggedTail(sm.Mirror):
    def touched(self, n, ch, dtype):
        return np.arange(n) < n - n % sm.vec_width(dtype)


class PartialPastTheLocalSlots(sm.Mirror):
    def write_parts(self, out, q):
        out[:q.size] = q
        if q.size < out.size:
            out[q.size] = 0.0


class HostSigLeft(sm.Mirror):
    def write_start_block(self, scal, gamma0, atol2, bs, stop):
        sig = int(sm.sig_word(scal)[0])
        super().write_start_block(scal, gamma0, atol2, bs, stop)
        sm.sig_word(scal)[0] = sig


class Gamma1Left(sm.Mirror):
    def write_start_block(self, scal, gamma0, atol2, bs, stop):
        g1 = scal[sm.GAMMA1]
        super().write_start_block(scal, gamma0, atol2, bs, stop)
        scal[sm.GAMMA1] = g1


# mutant: (the entry points it can show in, a kind whose cases must catch it)
MUTANTS = {
    OtherParity: (sc.PER_ITERATION, "parity1"),
    LessThanAtStart: (sc.STARTS, "eq_tol"),
    LessThanInDirection: (sc.DIRECTIONS, "rr_eq"),
    OneIterationMore: (sc.DIRECTIONS, "maxiter_hit"),
    LocalFold: (tuple(sc.ARGS), "g=2048"),
    DoubleCoefficients: (sc.PER_ITERATION, "tail_loop"),
    XReadsNewP: (sc.DIRECTIONS, "parity0"),
    NoTailLoop: (tuple(sc.ARGS), "tail_loop"),
    NoRaggedTail: (tuple(sc.ARGS), "ragged"),
    PartialPastTheLocalSlots: (("cg_update",), "g=local"),
    HostSigLeft: (sc.STARTS, "garbage_block"),
    Gamma1Left: (sc.STARTS, "garbage_block"),
}


@pytest.mark.parametrize("mutant", list(MUTANTS), ids=lambda m: m.__name__)
def test_the_table_tells_the_mutant_apart(mutant):
    entries, kind = MUTANTS[mutant]
    m = mutant()
    for entry in entries:
        for dtype in sc.DTYPES:
            if mutant is DoubleCoefficients and dtype == np.float64:
                continue
            caught = [c for c in of(entry, dtype) if sc.same(c, sc.expected(c, (inp := sc.inputs(c)), m), sc.expected(c, inp))]
            assert caught, (mutant.__name__, entry, dtype)
            assert any(kind in c.kinds for c in caught), (mutant.__name__, entry, dtype, kind)


def test_mutants_change_nothing_they_should_not():
    """The mutants are single decisions: DoubleCoefficients is the true mirror in fp64, LocalFold where g_red is the local count."""
    for c in of(dtype=np.float64):
        inp = sc.inputs(c)
        assert not sc.same(c, sc.expected(c, inp, DoubleCoefficients()), sc.expected(c, inp)), c.id
    for c in of(kind="g=local"):
        inp = sc.inputs(c)
        assert not sc.same(c, sc.expected(c, inp, LocalFold()), sc.expected(c, inp)), c.id
