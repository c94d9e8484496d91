"""The exported step API and the BLAS-1 entry points of include/hipk.h, call by call on the device: hipk_cg_start, hipk_cg_update,
hipk_cg_direction, hipk_cg_xupdate, hipk_cgm_start, hipk_cgm_direction over the case table of tests/_step_cases.py (one launch per
case, every output compared BITWISE with tests/_step_mirror.py: the operands, all 2048 slots of every partial array, the first 8
words of the scalar block), then hipk_dot_parts, hipk_reduce_parts, hipk_dot, hipk_axpy, hipk_xpby and hipk_gather against the
oracle / numpy, and the error paths, none of which reaches a launch.

Every device operand is a view into a larger buffer with 64 sentinel elements before and after it; the view starts 16-byte aligned
and ends with the operand's last element, and the sentinels are compared after every call: a store before the operand or past a
ragged tail shows without anything having to fault.  tests/test_step_cases.py shows without a GPU that the table covers every cell
and that a subtly wrong kernel gives other bits on at least one case."""
import numpy as np
import pytest
import torch

import _step_cases as sc
import _step_mirror as sm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
ERR_ARG, ERR_ALIGN, ERR_UNSUPPORTED = -1, -3, -4
SCALAR = 0.3718281828            # not representable in fp32


def sentinel(dtype):
    return np.dtype(dtype).type({8: -3.5e203, 4: -3.5e33}[np.dtype(dtype).itemsize]) if np.dtype(dtype).kind == "f" \
        else np.dtype(dtype).type(-0x5EED)


class Guarded:
    """A device operand between two guards of 64 sentinel elements."""
    def __init__(self, host):
        host = np.ascontiguousarray(host)
        self.n, self.dtype = host.size, host.dtype
        full = np.full(self.n + 2 * GUARD, sentinel(host.dtype), dtype=host.dtype)
        full[GUARD:GUARD + self.n] = host
        self.buf = torch.from_numpy(full).to(DEV)
        self.view = self.buf[GUARD:GUARD + self.n]
        self.ptr = self.buf.data_ptr() + GUARD * host.itemsize
        assert self.ptr % 16 == 0 and (self.n == 0 or self.view.data_ptr() == self.ptr)

    def read(self):
        """The operand after a call; the guards must be what they were."""
        full = self.buf.cpu().numpy()
        g = np.concatenate([full[:GUARD], full[GUARD + self.n:]])
        assert np.array_equal(sc.bits(g), sc.bits(np.full(2 * GUARD, sentinel(self.dtype), dtype=self.dtype))), "guard overwritten"
        return full[GUARD:GUARD + self.n].copy()


def stream(hipk):
    return hipk._stream(torch.device(DEV))


def code(hipk, dtype):
    return hipk.HIPK_F64 if np.dtype(dtype) == np.float64 else hipk.HIPK_F32


# ------------------------------------------------------------------------------------------------------ the step API
def device_args(hipk, case, entry, vec, part, scal, x_null):
    out = []
    for tok in sc.ARGS[entry]:
        if tok[0] == "@":
            out.append(None if (tok == "@x" and x_null) else vec[tok[1:]].ptr)
        elif tok[0] == "#":
            out.append(part[tok[1:]].ptr)
        else:
            out.append({"n": case.n, "ch": case.ch, "g": case.g, "it": case.it, "maxiter": case.maxiter, "tol": case.tol,
                        "atol": case.atol, "scal": scal.ptr, "dt": code(hipk, case.dtype), "stream": stream(hipk)}[tok])
    return out


@pytest.mark.parametrize("case", sc.CASES, ids=lambda c: c.id)
def test_step_call_is_the_mirror(hipk, oracle, case):
    L = hipk.lib()
    assert int(L.hipk_cg_scal_bytes()) == 8 * sc.SCAL_ALLOC
    inp = sc.inputs(case)
    want = sc.expected(case, inp)
    vec = {k: Guarded(v) for k, v in inp.vec.items()}
    part = {k: Guarded(v) for k, v in inp.part.items()}
    scal = Guarded(inp.scal)
    if case.split:
        # x += alpha p on its own, then the direction step without x: the x, p and block of the one call
        xargs = device_args(hipk, case, "cg_xupdate", vec, part, scal, False)
        hipk._check(L.hipk_cg_xupdate(*xargs), "hipk_cg_xupdate")
    args = device_args(hipk, case, case.entry, vec, part, scal, case.x_null or case.split)
    hipk._check(getattr(L, "hipk_" + case.entry)(*args), "hipk_" + case.entry)
    block = scal.read()
    if case.entry in sc.STARTS:
        # read on the host before any further call could see the block: hipk_cg_direction dereferences a non-null host_sig
        assert block[sm.GAMMA1] == 0.0 and int(sm.sig_word(block)[0]) == 0, "start left gamma[1] / host_sig as found"
    got = sc.outputs({k: v.read() for k, v in vec.items()}, {k: v.read() for k, v in part.items()}, block)
    assert np.array_equal(sc.bits(block[sm.SCAL_WORDS:]), sc.bits(inp.scal[sm.SCAL_WORDS:])), "words past the first 8 changed"
    bad = sc.same(case, got, want)
    for k in bad:
        d = np.flatnonzero(sc.bits(got[k]) != sc.bits(want[k]))
        print(f"{case.id} {k}: {d.size} differ, first at {d[0]}: got {got[k][d[0]]!r}, mirror {want[k][d[0]]!r}")
    assert not bad


def _dummy(hipk, entry, dtype, n=8):
    """Arguments of a call that must be refused before any launch (n_local = 8, one chunk)."""
    case = sc._case(entry, dtype, 2048, n, "g=local+5", it=2)
    inp = sc.inputs(case)
    vec = {k: Guarded(v) for k, v in inp.vec.items()}
    part = {k: Guarded(v) for k, v in inp.part.items()}
    scal = Guarded(inp.scal)
    keep = (inp, vec, part, scal)
    return case, device_args(hipk, case, entry, vec, part, scal, False), keep


def _refused(hipk, entry, args, status, text, keep):
    L = hipk.lib()
    assert getattr(L, "hipk_" + entry)(*args) == status, (entry, text)
    assert text in L.hipk_last_error().decode(), (entry, text, L.hipk_last_error())
    inp, vec, part, scal = keep           # nothing ran: every operand and guard is what it was
    for host, dev in [(inp.vec[k], vec[k]) for k in vec] + [(inp.part[k], part[k]) for k in part] + [(inp.scal, scal)]:
        assert np.array_equal(sc.bits(dev.read()), sc.bits(host))


@pytest.mark.parametrize("dtype", sc.DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("entry", list(sc.ARGS))
def test_step_entry_point_refuses_bad_arguments(hipk, entry, dtype):
    toks = sc.ARGS[entry]
    case, good, keep = _dummy(hipk, entry, dtype)

    def with_(**kw):
        a = list(good)
        for k, v in kw.items():
            a[toks.index(k)] = v
        return a

    _refused(hipk, entry, with_(n=0), ERR_ARG, "n_local must be positive", keep)
    for ch in (1024, 3072):
        _refused(hipk, entry, with_(ch=ch), ERR_ARG, "chunk_rows", keep)
    for g in (0, 2049):
        _refused(hipk, entry, with_(g=g), ERR_ARG, "g_red out of range", keep)
    _refused(hipk, entry, with_(n=2 * 2048 + 1, g=2), ERR_ARG, "more local chunks than g_red", keep)
    _refused(hipk, entry, with_(dt=7), ERR_UNSUPPORTED, "dtype", keep)
    for i, tok in enumerate(toks):
        if tok == "scal" or tok[0] in "@#":
            if (entry, tok) == ("cg_direction", "@x"):
                continue                      # x == NULL is the p-only form (the x_null cases of the table)
            a = list(good)
            a[i] = None
            _refused(hipk, entry, a, ERR_ARG, "null argument", keep)
        if tok[0] == "@":                     # a vector one element past a 16-byte boundary
            a = list(good)
            a[i] = good[i] + np.dtype(dtype).itemsize
            _refused(hipk, entry, a, ERR_ALIGN, "must be 16-byte aligned", keep)


def test_blas1_entry_points_refuse_bad_arguments(hipk):
    L = hipk.lib()
    x = Guarded(np.ones(8))
    part = Guarded(np.zeros(sm.MAX_PARTS))
    out = Guarded(np.zeros(1))
    assert L.hipk_reduce_parts(part.ptr, 2049, out.ptr, stream(hipk)) == ERR_ARG
    assert "bad argument" in L.hipk_last_error().decode()
    assert L.hipk_dot_parts(2048 * 2048 + 1, 2048, x.ptr, x.ptr, hipk.HIPK_F64, part.ptr, stream(hipk)) == ERR_ARG
    assert "too many chunks" in L.hipk_last_error().decode()
    assert L.hipk_dot_parts(8, 2048, x.ptr + 8, x.ptr, hipk.HIPK_F64, part.ptr, stream(hipk)) == ERR_ALIGN
    assert out.read()[0] == 0.0 and not part.read().any() and np.all(x.read() == 1.0)


# --------------------------------------------------------------------------------------------------------- BLAS-1
DOT_SHAPES = dict(sc.SHAPES)
DOT_SHAPES[2048 * 16] = (2049, 32767, 32768, 32769, 65539)


@pytest.mark.parametrize("dtype", sc.DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("ch", list(DOT_SHAPES))
def test_dot_parts_with_an_explicit_chunk_size(hipk, oracle, ch, dtype):
    L = hipk.lib()
    for n in DOT_SHAPES[ch]:
        rng = np.random.default_rng(n + ch)
        a, b = rng.standard_normal(n).astype(dtype), rng.standard_normal(n).astype(dtype)
        x, y = Guarded(a), Guarded(b)
        part = Guarded(np.full(sm.MAX_PARTS, sc.SENTINEL_PART))
        hipk._check(L.hipk_dot_parts(n, ch, x.ptr, y.ptr, code(hipk, dtype), part.ptr, stream(hipk)), "hipk_dot_parts")
        want = np.full(sm.MAX_PARTS, sc.SENTINEL_PART)
        q = sm.dot_parts(a, b, ch)
        assert q.size == sm.local_chunks(n, ch)
        want[:q.size] = q                                   # the slots beyond the local chunks are untouched
        assert np.array_equal(sc.bits(part.read()), sc.bits(want)), (n, ch)
        assert np.array_equal(sc.bits(x.read()), sc.bits(a)) and np.array_equal(sc.bits(y.read()), sc.bits(b))


@pytest.mark.parametrize("g", [0, 1, 2, 255, 256, 257, 2047, 2048])
def test_reduce_parts_fold_order(hipk, oracle, g):
    """Parts over 30 orders of magnitude with mixed signs: another order of the fold gives other bits.  The slots past g hold NaN."""
    L = hipk.lib()
    rng = np.random.default_rng(1000 + g)
    parts = rng.uniform(0.5, 1.5, sm.MAX_PARTS) * 10.0 ** rng.uniform(-15, 15, sm.MAX_PARTS) * rng.choice([-1.0, 1.0], sm.MAX_PARTS)
    parts[g:] = np.nan
    p, out = Guarded(parts), Guarded(np.full(1, sc.SENTINEL_PART))
    hipk._check(L.hipk_reduce_parts(p.ptr, g, out.ptr, stream(hipk)), "hipk_reduce_parts")
    want = oracle.reduce_parts(parts[:g])
    assert sc.bits(out.read())[0] == sc.bits(np.array([want]))[0]
    assert np.array_equal(sc.bits(p.read()), sc.bits(parts))


@pytest.mark.parametrize("n", [1, 2, 3, 5, 1023, 2049, 100_003])
def test_dot_fp32(hipk, oracle, n):
    L = hipk.lib()
    rng = np.random.default_rng(n)
    a, b = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    x, y, out = Guarded(a), Guarded(b), Guarded(np.full(1, sc.SENTINEL_PART))
    scratch = hipk.scratch(torch.device(DEV))
    hipk._check(L.hipk_dot(n, x.ptr, y.ptr, hipk.HIPK_F32, out.ptr, scratch.data_ptr(), stream(hipk)), "hipk_dot")
    assert sc.bits(out.read())[0] == sc.bits(np.array([oracle.dot32(a, b)]))[0]
    assert np.array_equal(sc.bits(x.read()), sc.bits(a)) and np.array_equal(sc.bits(y.read()), sc.bits(b))


@pytest.mark.parametrize("dtype", sc.DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("n", [1, 2, 3, 5, 2047, 2049, 10_001, 4_194_304 + 3])       # the last: chunks of 4096 and their tail
def test_axpy_xpby(hipk, n, dtype):
    """y + T(a) * x and x + T(a) * y in numpy of dtype T: the scalar is rounded to T first, then multiply, round, add, round."""
    L = hipk.lib()
    assert int(L.hipk_chunk_size(n)) == (4096 if n > 4_194_304 else 2048)
    rng = np.random.default_rng(n)
    xh, yh = rng.standard_normal(n).astype(dtype), rng.standard_normal(n).astype(dtype)
    a = np.dtype(dtype).type(SCALAR)
    assert (float(a) != SCALAR) == (dtype == np.float32)
    x, y = Guarded(xh), Guarded(yh)
    hipk._check(L.hipk_axpy(n, SCALAR, x.ptr, y.ptr, code(hipk, dtype), stream(hipk)), "hipk_axpy")
    want = yh + a * xh
    assert want.dtype == dtype and np.array_equal(sc.bits(y.read()), sc.bits(want))
    y = Guarded(yh)
    hipk._check(L.hipk_xpby(n, x.ptr, SCALAR, y.ptr, code(hipk, dtype), stream(hipk)), "hipk_xpby")
    want = xh + a * yh
    assert want.dtype == dtype and np.array_equal(sc.bits(y.read()), sc.bits(want))
    assert np.array_equal(sc.bits(x.read()), sc.bits(xh))


@pytest.mark.parametrize("dtype", sc.DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("m", [0, 1, 255, 256, 257, 2048 * 256 + 1])                   # the last: the second grid-stride round
def test_gather(hipk, m, dtype):
    L = hipk.lib()
    rng = np.random.default_rng(m)
    n_src = 4099
    src = rng.standard_normal(n_src).astype(dtype)
    idx = rng.integers(0, n_src, size=max(m, 1)).astype(np.int32)       # unsorted, repeated
    idx[0] = n_src - 1
    if m > 1:
        idx[-1], idx[m // 2] = 0, idx[0]
    s, i = Guarded(src), Guarded(idx)
    before = np.full(max(m, 1), sentinel(dtype), dtype=dtype)
    d = Guarded(before)
    hipk._check(L.hipk_gather(m, i.ptr, s.ptr, d.ptr, code(hipk, dtype), stream(hipk)), "hipk_gather")
    want = before.copy()
    want[:m] = src[idx[:m]]
    assert np.array_equal(sc.bits(d.read()), sc.bits(want))
    assert np.array_equal(sc.bits(s.read()), sc.bits(src)) and np.array_equal(i.read(), idx)


# --------------------------------------------------------------------------------------------------------- special values
SPECIAL_N = (1, 2049, 70_001)
SPECIAL_KINDS = ("+inf", "-inf", "both-inf", "nan", "negzero", "subnormal")


def _special(kind, n, dtype, seed):
    """(a, b) of n standard-normal entries with the kind's special entries: one infinity, two of opposite sign (inf - inf in a sum),
    one NaN, every entry of a a negative zero (the sign of a zero sum), or both vectors scaled until products are subnormal or 0."""
    rng = np.random.default_rng(seed)
    a, b = rng.standard_normal(n).astype(dtype), rng.standard_normal(n).astype(dtype)
    k = n // 2
    if kind in ("+inf", "-inf"):
        a[k] = np.inf if kind == "+inf" else -np.inf
    elif kind == "both-inf":
        a[k], a[0], b[k], b[0] = np.inf, -np.inf, 1.0, 1.0          # n = 1: the second assignment wins, one -inf
    elif kind == "nan":
        b[n - 1] = np.nan
    elif kind == "negzero":
        a[:] = -0.0
    else:
        e = -530 if dtype == np.float64 else -70                      # products near 2^-1060 / 2^-140: subnormal, or rounded to 0
        a, b = np.ldexp(a, e).astype(dtype), np.ldexp(b, e).astype(dtype)
        a[k] = -0.0
    return a, b


def _canon_bits(a):
    """sc.bits with every NaN as one pattern: the sign and payload of a NaN an operation produces are the implementation's."""
    a = np.array(a, copy=True)
    a[np.isnan(a)] = np.nan
    return sc.bits(a)


@pytest.mark.parametrize("dtype", sc.DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("n", SPECIAL_N)
def test_dot_on_special_values(hipk, oracle, n, dtype):
    L = hipk.lib()
    scratch = hipk.scratch(torch.device(DEV))
    for kind in SPECIAL_KINDS:
        a, b = _special(kind, n, dtype, n)
        x, y, out = Guarded(a), Guarded(b), Guarded(np.full(1, sc.SENTINEL_PART))
        hipk._check(L.hipk_dot(n, x.ptr, y.ptr, code(hipk, dtype), out.ptr, scratch.data_ptr(), stream(hipk)), "hipk_dot")
        want = oracle.dot(a, b) if dtype == np.float64 else oracle.dot32(a, b)
        got = out.read()
        assert _canon_bits(got)[0] == _canon_bits(np.array([want]))[0], (kind, n, got[0], want)
        assert np.array_equal(sc.bits(x.read()), sc.bits(a)) and np.array_equal(sc.bits(y.read()), sc.bits(b))


@pytest.mark.parametrize("dtype", sc.DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("n", SPECIAL_N)
def test_dot_parts_on_special_values(hipk, oracle, n, dtype):
    """A special entry reaches the partial of its own chunk only."""
    L = hipk.lib()
    ch = 2048
    for kind in SPECIAL_KINDS:
        a, b = _special(kind, n, dtype, n + 1)
        x, y = Guarded(a), Guarded(b)
        part = Guarded(np.full(sm.MAX_PARTS, sc.SENTINEL_PART))
        hipk._check(L.hipk_dot_parts(n, ch, x.ptr, y.ptr, code(hipk, dtype), part.ptr, stream(hipk)), "hipk_dot_parts")
        q = oracle.dot_parts_ch(a, b, ch) if dtype == np.float64 else oracle.dot_parts_ch32(a, b, ch)
        got = part.read()
        assert np.array_equal(_canon_bits(got[:q.size]), _canon_bits(q)), (kind, n)
        assert np.array_equal(sc.bits(got[q.size:]), sc.bits(np.full(sm.MAX_PARTS - q.size, sc.SENTINEL_PART)))
        if kind in ("+inf", "-inf", "both-inf", "nan"):
            special = np.unique(np.flatnonzero(~np.isfinite(a) | ~np.isfinite(b)) // ch)
            assert np.array_equal(np.flatnonzero(~np.isfinite(got[:q.size])), special), (kind, n)


@pytest.mark.parametrize("dtype", sc.DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("n", SPECIAL_N)
def test_axpy_xpby_on_special_values(hipk, n, dtype):
    L = hipk.lib()
    a = np.dtype(dtype).type(SCALAR)
    for kind in SPECIAL_KINDS:
        xh, yh = _special(kind, n, dtype, n + 2)
        x, y = Guarded(xh), Guarded(yh)
        hipk._check(L.hipk_axpy(n, SCALAR, x.ptr, y.ptr, code(hipk, dtype), stream(hipk)), "hipk_axpy")
        with np.errstate(all="ignore"):
            want = yh + a * xh
        assert np.array_equal(_canon_bits(y.read()), _canon_bits(want)), (kind, n)
        y = Guarded(yh)
        hipk._check(L.hipk_xpby(n, x.ptr, SCALAR, y.ptr, code(hipk, dtype), stream(hipk)), "hipk_xpby")
        with np.errstate(all="ignore"):
            want = xh + a * yh
        assert np.array_equal(_canon_bits(y.read()), _canon_bits(want)), (kind, n)
        assert np.array_equal(sc.bits(x.read()), sc.bits(xh))


@pytest.mark.parametrize("dtype", sc.DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("n", SPECIAL_N)
def test_gather_on_special_values(hipk, n, dtype):
    """A copy: every bit arrives, the sign and payload of a NaN included."""
    L = hipk.lib()
    for kind in SPECIAL_KINDS:
        src, _ = _special(kind, n, dtype, n + 3)
        if kind == "nan":
            src[0] = np.array([-np.nan], dtype=dtype)[0]
            src[n // 2] = np.nan
        idx = np.random.default_rng(n).integers(0, n, size=n).astype(np.int32)
        idx[0], idx[-1] = n // 2, 0
        s, i = Guarded(src), Guarded(idx)
        d = Guarded(np.full(n, sentinel(dtype), dtype=dtype))
        hipk._check(L.hipk_gather(n, i.ptr, s.ptr, d.ptr, code(hipk, dtype), stream(hipk)), "hipk_gather")
        assert np.array_equal(sc.bits(d.read()), sc.bits(src[idx])), (kind, n)
        assert np.array_equal(sc.bits(s.read()), sc.bits(src))
