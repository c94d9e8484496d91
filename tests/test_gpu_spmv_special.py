"""Every in-process SpMV case of tests/_spmv_cases.py on non-finite and on tiny, signed operands.  The sliced-ELL kernels pad rows,
tiles and lane groups, and what keeps the padding out of a sum is an argument in a comment each time ("acc + (0.0 * 0.0)", "kept out
of the sum by a select", "surplus lanes re-read the group's first entry", "padding lanes read x[min(row, n_rows - 1)]"): a padding lane
that multiplies instead of selecting gives the right bits on every finite x and turns ONE infinity in x into NaNs in rows that never
reference it.  Per case, every step and every mode, the kernel note asserted as tests/test_gpu_spmv_instantiations.py does:

  1. baseline: y and the chunk partials of the fused dots from the table's x, w, b -- the oracle's bits;
  2. poison (the 2.2 M-row matrices: columns n - 1 and the uniform tile's, +inf and NaN, for the time budget): x[c] = +inf, -inf,
     NaN for c = 0, n - 1, the middle of a full interior tile (served from a uniform-tile word where the
     case has them), the first column of a tile (referenced by the last rows of the tile before it) and the last column of the last
     full tile.  y and the partials are the oracle's bits; and, without the oracle, y[r] is non-finite exactly for the rows that
     store an entry in column c (poison() of tests/_special_cases.py, from the host CSR arrays), a partial exactly where its chunk
     holds such a row (with w = x: or row c), and everything else has the baseline's bits;
  3. small and signed: x at 2^-1040 (fp32: 2^-140) with a few -0.0 entries, the matrix values at the same scale through
     CsrHandle.update_values -- the handle keeps its path and form -- and both: subnormal products, and the signs of zero sums.

"Bits" means every bit of every value that is not a NaN, and the positions of the NaNs (_ibits).  The `also_plain` cases repeat all of
it on the plain CSR kernels.  Comparisons run on the device; a mismatch is fetched and named."""
import numpy as np
import pytest
import torch

import _special_cases as S
import _spmv_cases as C
from _arena import Arena, guard_bytes_for
from _spmv_inst_worker import References

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VALUES = (("+inf", np.inf), ("-inf", -np.inf), ("nan", np.nan))
SMALL = {C.DOUBLE: -1040, C.FLOAT: -140}
_held = {}


def _ibits(t):
    """The bit patterns of t, every NaN as ONE pattern: IEEE 754 leaves the sign and payload of a NaN that an operation produces
    to the implementation, and the two differ (inf - inf is 0x7FF8... on gfx950 and 0xFFF8... on x86; b - A x negates a NaN of x
    on one and not on the other).  Where the NaNs are, and every bit of every other value -- zeros' signs, infinities' -- counts."""
    t = t.masked_fill(torch.isnan(t), float("nan"))
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _to(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class _Refs:
    """The oracle's outputs of one References on the device: y[resid], part0[(resid, w is x)], part1[resid]."""

    def __init__(self, ref):
        self.x, self.w, self.b = _to(ref.x), _to(ref.w), _to(ref.b)
        self.y = {k: _to(v) for k, v in ref.y.items()}
        self.part0 = {k: _to(v) for k, v in ref.part0.items()}
        self.part1 = {k: _to(v) for k, v in ref.part1.items()}


_last_arrays = {}


def _arrays(name):
    """C.matrix(name), kept for the next storage type of the same matrix (the cases run matrix by matrix)."""
    if name not in _last_arrays:
        _last_arrays.clear()
        _last_arrays[name] = C.matrix(name)
    return _last_arrays[name]


class _Matrix:
    """One (matrix, storage type) of the table: the CSR arrays, the baseline, one poisoned reference per (column, value), and the
    small-and-signed references -- each computed once by the oracle and kept on the device."""

    def __init__(self, hipk, oracle, name, dtype):
        self.name, self.dtype = name, dtype
        self.f = np.float64 if dtype == C.DOUBLE else np.float32
        self.arrays = _arrays(name)
        self.crow, self.col, val = self.arrays
        self.n = len(self.crow) - 1
        self.ch = int(hipk.lib().hipk_chunk_size(self.n))
        self.G = int(hipk.lib().hipk_chunk_count(self.n))
        x, w, b = C.vectors(name, dtype)
        self.base = _Refs(References(oracle, name, dtype, self.ch, arrays=self.arrays, vectors=(x, w, b)))
        self.dcrow, self.dcol, self.dval = _to(self.crow), _to(self.col), _to(val.astype(self.f))
        full = self.n // S.TILE
        ut = full // 2
        # the uniform tile: every one of its 256 rows stores the same column offsets (an interior tile of a band), which is what
        # the uniform-tile words encode; the cases whose note says UNI / wide serve it from such a word
        lens = np.diff(self.crow[ut * S.TILE:(ut + 1) * S.TILE + 1])
        assert (lens == lens[0]).all()
        e0 = int(self.crow[ut * S.TILE])
        offs = self.col[e0:e0 + S.TILE * int(lens[0])].reshape(S.TILE, -1) - np.arange(ut * S.TILE, (ut + 1) * S.TILE)[:, None]
        assert (offs == offs[0]).all(), "the tile chosen as uniform is not"
        self.poisoned = []
        vals_of = dict(VALUES)
        for c, vnames in S.spmv_poisons(self.n, ut):
            rows, _, chunks = S.poison(self.crow, self.col, [c], chunk=self.ch)
            assert rows.size >= 1 and c in rows          # every matrix of the table stores its diagonal
            rmask = torch.zeros(self.n, dtype=torch.bool, device=DEV)
            rmask[_to(rows)] = True
            cmask = torch.zeros(self.G, dtype=torch.bool, device=DEV)
            cmask[_to(chunks)] = True
            for vname in vnames:
                v = vals_of[vname]
                xp = x.copy()
                xp[c] = v
                refs = _Refs(References(oracle, name, dtype, self.ch, arrays=self.arrays, vectors=(xp, w, b)))
                self.poisoned.append((f"x[{c}] = {vname}", refs, rmask, cmask))
        # small and signed: 2^e x with a few negative zeros; the values at 2^e
        e = SMALL[dtype]
        xs = S.scaled(x, e)
        xz = x.copy()
        for a in (xs, xz):
            a[[0, 1, self.n // 2, self.n - 1]] = -0.0
        vs = S.scaled(val.astype(self.f), e)
        self.small_vals = _to(vs)
        spmv = oracle.spmv if dtype == C.DOUBLE else oracle.spmv32
        oracle.set_threads(16)
        try:
            self.small = [("x at 2^%d" % e, False, _to(xs), {r: _to(spmv(self.crow, self.col, val.astype(self.f), xs, bsub=b if r else None)) for r in (False, True)}),
                          ("A at 2^%d" % e, True, _to(xz), {r: _to(spmv(self.crow, self.col, vs, xz, bsub=b if r else None)) for r in (False, True)}),
                          ("A and x at 2^%d" % e, True, _to(xs), {r: _to(spmv(self.crow, self.col, vs, xs, bsub=b if r else None)) for r in (False, True)})]
        finally:
            oracle.set_threads(1)
        item = np.dtype(self.f).itemsize
        self.y_arena = Arena(DEV, self.n * item, 16, guard_bytes_for(self.n, item))


def _matrix(hipk, oracle, name, dtype):
    key = (name, dtype)
    if key not in _held:
        _held.clear()                      # one at a time: sixteen references of 2.2 M rows each
        _held[key] = _Matrix(hipk, oracle, name, dtype)
    return _held[key]


def _launch(hipk, h, m, x, w, b, mode):
    L = hipk.lib()
    y = m.y_arena.view(x.dtype, m.n)
    y.fill_(float("nan"))
    p0 = torch.full((m.G,), float("nan"), dtype=torch.float64, device=DEV)
    p1 = torch.full((m.G,), float("nan"), dtype=torch.float64, device=DEV)
    hipk._check(L.hipk_spmv_ex(h._h, x.data_ptr(), y.data_ptr(), mode, w.data_ptr(), b.data_ptr(), p0.data_ptr(), p1.data_ptr(),
                               None, 0, torch.cuda.current_stream().cuda_stream), "hipk_spmv_ex")
    return hipk.CsrHandle.last_spmv_kernel(), y, p0, p1


def _where(got, want, unit):
    bad = torch.nonzero(_ibits(got) != _ibits(want)).flatten()
    first = bad[:6].cpu().tolist()
    return (f"{bad.numel()} of {got.numel()} differ; first {first}" + (f" (tiles {[i // unit for i in first]})" if unit else "") +
            f", last {int(bad[-1])}; got {got[bad[:3]].cpu().tolist()} want {want[bad[:3]].cpu().tolist()}")


def _run_all(hipk, h, m, case, want_note, failures, tag0, plain=False):
    """Steps 1 and 2 on handle h with its current switches: every run of the case, baseline first."""
    base = {}
    for mode, wx in case["runs"]:
        resid = bool(mode & 4)
        for what, refs, rmask, cmask in [("baseline", m.base, None, None)] + m.poisoned:
            tag = f"{tag0} mode {mode}" + (" w=x" if wx else "") + f", {what}"
            x = refs.x
            note, y, p0, p1 = _launch(hipk, h, m, x, x if wx else refs.w, refs.b, mode)
            if not (note.startswith("hipk_spmv_kernel<") if plain else note == want_note[mode]):
                failures.append(f"{tag}: kernel {note}, expected {'hipk_spmv_kernel<...>' if plain else want_note[mode]}")
            outs = [("y", y, refs.y[resid], rmask, S.TILE)]
            if mode & 1:
                outs.append(("part0", p0, refs.part0[(resid, wx)], cmask, 0))
            if mode & 2:
                outs.append(("part1", p1, refs.part1[resid], cmask, 0))
            for oname, got, want, mask, unit in outs:
                if not torch.equal(_ibits(got), _ibits(want)):
                    failures.append(f"{tag} [{note}] {oname} against the oracle: {_where(got, want, unit)}")
                if mask is None:
                    base[(mode, wx, oname)] = got.clone()
                    if not bool(torch.isfinite(got).all()):
                        failures.append(f"{tag} [{note}] {oname}: a non-finite baseline")
                    continue
                # without the oracle: non-finite exactly where the pattern says, the baseline's bits elsewhere
                if oname == "part0" and wx:
                    c = int(what.split("[")[1].split("]")[0])
                    mask = mask.clone()
                    mask[c // m.ch] = True
                bad = ~torch.isfinite(got)
                if not torch.equal(bad, mask):
                    extra, missing = torch.nonzero(bad & ~mask).flatten(), torch.nonzero(mask & ~bad).flatten()
                    failures.append(f"{tag} [{note}] {oname}: non-finite where the pattern does not reference the column: "
                                    f"{extra.numel()} (first {extra[:8].cpu().tolist()}); finite where it does: {missing.numel()} "
                                    f"(first {missing[:8].cpu().tolist()}); expected {int(mask.sum())}")
                b0 = base[(mode, wx, oname)]
                if not torch.equal(_ibits(got).masked_fill(mask, 0), _ibits(b0).masked_fill(mask, 0)):
                    failures.append(f"{tag} [{note}] {oname}: rows outside the poisoned set lost the baseline's bits")


def _guards(m, failures, tag0):
    """The guards of y's arena after a set of launches (tests/test_gpu_spmv_instantiations.py checks them launch by launch)."""
    if not m.y_arena.guards_intact():
        failures.append(f"{tag0}: a write outside y[0..n): {m.y_arena.touched()}")


def _run_small(hipk, h, m, case, want_note, failures, tag0, path, plain=False):
    """Step 3: tiny x, tiny values through update_values, both; then the table's values again."""
    try:
        current = "table"
        for what, scaled_vals, xs, ys in m.small:
            if scaled_vals and current != "small":
                h.update_values(m.small_vals)
                current = "small"
                kind = hipk.CsrHandle.last_update_kind()
                if kind == 3 or h.path() != path:
                    failures.append(f"{tag0} {what}: update_values changed the form (kind {kind}, path {h.path()}, was {path})")
            for mode, wx in case["runs"]:
                tag = f"{tag0} mode {mode}" + (" w=x" if wx else "") + f", {what}"
                note, y, _, _ = _launch(hipk, h, m, xs, xs if wx else m.base.w, m.base.b, mode)
                if not (note.startswith("hipk_spmv_kernel<") if plain else note == want_note[mode]):
                    failures.append(f"{tag}: kernel {note}, expected {'hipk_spmv_kernel<...>' if plain else want_note[mode]}")
                want = ys[bool(mode & 4)]
                if not torch.equal(_ibits(y), _ibits(want)):
                    failures.append(f"{tag} [{note}] y against the oracle: {_where(y, want, S.TILE)}")
    finally:
        h.update_values(m.dval)
    kind = hipk.CsrHandle.last_update_kind()
    if kind == 3 or h.path() != path:
        failures.append(f"{tag0}: update_values back to the table's values changed the form (kind {kind}, path {h.path()}, was {path})")


IN_PROCESS = sorted(S.spmv_rows(C.CASES), key=lambda n: (C.CASES[n]["matrix"], C.CASES[n]["dtype"], n))


@pytest.mark.parametrize("name", IN_PROCESS)
def test_spmv_case_on_special_operands(hipk, oracle, monkeypatch, name):
    case = C.CASES[name]
    m = _matrix(hipk, oracle, case["matrix"], case["dtype"])
    assert int(hipk.lib().hipk_chunk_size(m.n)) == m.ch

    def setenv(k, v):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)

    for k, v in case["env"].items():
        setenv(k, v)
    print("spmv special case", name, flush=True)
    failures = []
    h = hipk.CsrHandle(m.dcrow, m.dcol, m.dval, (m.n, m.n))     # after the switches: the handle caches its kernel choice
    try:
        if case["plain_only"]:
            h.set_path(plain_only=True)
        path = h.path()
        for si, (delta, want) in enumerate(case["steps"]):
            for k, v in delta.items():
                setenv(k, v)
            _run_all(hipk, h, m, case, want, failures, f"{name} step {si}")
            _run_small(hipk, h, m, case, want, failures, f"{name} step {si}", path)
            _guards(m, failures, f"{name} step {si}")
        if case["also_plain"]:
            h.set_path(plain_only=True)
            _run_all(hipk, h, m, case, None, failures, f"{name} plain CSR kernels", plain=True)
            _run_small(hipk, h, m, case, None, failures, f"{name} plain CSR kernels", h.path(), plain=True)
            _guards(m, failures, f"{name} plain CSR kernels")
    finally:
        h.close()
    for t, t0 in ((m.base.x, C.vectors(case["matrix"], case["dtype"])[0]),):
        assert np.array_equal(t.cpu().numpy(), t0), f"{name}: x changed"
    assert not failures, "\n".join(failures[:40]) + (f"\n... {len(failures)} failures" if len(failures) > 40 else "")


# ---------------------------------------------------------------------------------------------- the Chebyshev epilogue instantiations
CHEB_CASES = [("band3", np.float64), ("band5", np.float64), ("band7", np.float64), ("band5", np.float32)]
CHEB_DEGREES = (1, 3)      # the init step alone, and the repeated step: a poisoned entry spreads by one stencil reach per degree


@pytest.mark.parametrize("name, dtype", CHEB_CASES, ids=[f"{n}-{'f64' if d == np.float64 else 'f32'}" for n, d in CHEB_CASES])
def test_cheb_epilogue_on_a_poisoned_vector(hipk, oracle, monkeypatch, name, dtype):
    """hipk_cheb_apply with one non-finite entry in r, through every instantiation that carries the epilogue (tests/_cheb_cases.py:
    hipk_spmv_sell_wide_kernel<4 | 5 | 8, 28, 0 | 1>, hipk_spmv_cheb_kernel<double, 1280 | 2048>, <float, 2048>), the note asserted,
    at the ragged n = 2 200 077 that the chunk walk needs.  Degree 1 with +inf in the last row (the ragged tile), degree 3 with a
    NaN in the middle of a uniform interior tile: z has the mirror's bits (tests/_cheb_mirror.py), and, without the mirror, z is
    non-finite exactly in the rows that poison() reaches in `degree` applications from the poisoned row; every other row has the
    bits of the same call on the finite r.  (The finite apply is pinned to the mirror by tests/test_gpu_chebyshev_kernels.py.)"""
    import _cheb_cases as CC
    from _cheb_mirror import mirror
    from test_gpu_coded import make_handle
    case = CC.BANDS[name]
    n = CC.N_BIG
    crow, col, val, diag = CC.band(n, case["offsets"])
    val = val.astype(dtype)
    dinv, r = CC.apply_inputs(n, diag, dtype)
    dd = _to(dinv)
    variants = {1: (n - 1, np.inf), 3: ((n // S.TILE // 2) * S.TILE + S.TILE // 2, np.nan)}
    coef, refs, masks, rds = {}, {}, {}, {}
    oracle.set_threads(16)
    try:
        for m, (c, v) in variants.items():
            M, coef[m] = CC.apply_coefficients(m, dinv)
            rp = r.copy()
            rp[c] = v
            refs[m] = _to(mirror(oracle, crow, col, val, M, rp, dtype=dtype))
            rows = np.array([c])
            for _ in range(m):
                rows = S.poison(crow, col, rows)[0]
            masks[m] = torch.zeros(n, dtype=torch.bool, device=DEV)
            masks[m][_to(rows)] = True
            assert rows.size > 1 and c in rows
            rds[m] = _to(rp)
    finally:
        oracle.set_threads(1)
    r0 = _to(r)
    failures = []

    def run(tag, h, note):
        monkeypatch.setenv("HIPK_CHEB_FUSED", "1")
        for m in CHEB_DEGREES:
            zb = hipk.cheb_apply(h, m, dd, coef[m], r0).clone()
            z = hipk.cheb_apply(h, m, dd, coef[m], rds[m])
            got = hipk.CsrHandle.last_spmv_kernel()
            t = f"{name} {tag} degree {m} [{got}]"
            if got != note:
                failures.append(f"{t}: expected {note}")
            if not bool(torch.isfinite(zb).all()):
                failures.append(f"{t}: a non-finite baseline")
            if not torch.equal(_ibits(z), _ibits(refs[m])):
                failures.append(f"{t} against the mirror: {_where(z, refs[m], S.TILE)}")
            bad = ~torch.isfinite(z)
            if not torch.equal(bad, masks[m]):
                extra, missing = torch.nonzero(bad & ~masks[m]).flatten(), torch.nonzero(masks[m] & ~bad).flatten()
                failures.append(f"{t}: non-finite outside the reach of the poisoned row: {extra.numel()} (first {extra[:8].cpu().tolist()}); "
                                f"finite inside it: {missing.numel()} (first {missing[:8].cpu().tolist()}); expected {int(masks[m].sum())}")
            if not torch.equal(_ibits(z).masked_fill(masks[m], 0), _ibits(zb).masked_fill(masks[m], 0)):
                failures.append(f"{t}: rows outside the reach lost the bits of the finite apply")

    print("cheb special case", name, dtype.__name__, flush=True)
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    if dtype == np.float64:
        for strided in (0, 1):
            monkeypatch.setenv("HIPK_SPMV_SELL_STRIDED", str(strided))
            h = make_handle(hipk, crow, col, val, n)
            assert h.path() == "coded"
            run(f"strided={strided}", h, case["wide"][strided])
            h.close()
        monkeypatch.delenv("HIPK_SPMV_SELL_STRIDED")
    h = make_handle(hipk, crow, col, val, n, dtype=tdt)
    h.set_path(plain_only=True)
    run("plain", h, case["plain"] if dtype == np.float64 else "hipk_spmv_cheb_kernel<float,2048>")
    h.close()
    assert not failures, "\n".join(failures)
