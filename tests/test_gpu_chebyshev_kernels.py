"""Every SpMV kernel instantiation that carries the Chebyshev epilogue (tests/test_chebyshev_kernel_resources.py: CHEB), run and
compared bit for bit with the numpy mirror (tests/_cheb_mirror.py), the instantiation asserted from the kernel note:

1. hipk_cheb_apply stand-alone at n = 2 200 077 (a last tile of 13 rows, a ragged last chunk) on banded matrices of 3 to 9
   entries per row -- hipk_spmv_sell_wide_kernel<4 | 5 | 8, 28, 0 | 1>, hipk_spmv_cheb_kernel<double, 1280 | 2048> and
   <float, 2048> --, dinv varying per row, scale != 1, degrees 1, 3 and 32; the wide kernel's masked tiles (HIPK_SPMV_MASKED=1)
   on grids of 2.2 M to 4 M rows whose line ends make such tiles, their presence read from the handle's byte count; the same
   apply at n = 70 001 and at sizes below a handful of tiles (hipk_cheb_init_kernel / hipk_cheb_step_kernel, n not a multiple
   of the 16-byte vector: bits only, whichever kernel runs);
2. ChebyshevPreconditioner at the sizes the README quotes (N = 4 M, 16 M, 64 M: chunk sizes 2048, 8192, 32768);
3. whole cg / bicgstab / gmres solves in which an epilogue kernel runs: bitwise equal to the same solve with SpMV +
   hipk_cheb_step_kernel and to the same solve with the recurrence written in torch operations around hipk.spmv.

The case table is tests/_cheb_cases.py; tests/test_chebyshev_cases.py checks it without a GPU.  Every comparison is bitwise."""
import numpy as np
import pytest
import torch

import _cheb_cases as C
from _cheb_mirror import mirror
from test_gpu_coded import make_handle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _bits(a):
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def _differs(z, ref):
    """None if z has the mirror's bits, else where it does not: count, first rows, their 256-row tiles."""
    bad = np.flatnonzero(_bits(z) != _bits(ref))
    if bad.size == 0:
        return None
    n = ref.size
    return (f"{bad.size} of {n} rows differ; first rows {bad[:8].tolist()} (tiles {(bad[:8] // 256).tolist()} of {(n + 255) // 256}, "
            f"the last tile has {n - (n - 1) // 256 * 256} rows), last row {int(bad[-1])}; z {z[bad[:3]].tolist()} mirror {ref[bad[:3]].tolist()}")


class _Apply:
    """One matrix's inputs on the host and the device, its mirrors per degree, and the check of one hipk_cheb_apply call."""

    def __init__(self, hipk, oracle, crow, col, val, diag, dtype=np.float64, degrees=C.DEGREES):
        self.hipk, self.n, self.dtype = hipk, len(crow) - 1, dtype
        self.dinv, self.r = C.apply_inputs(self.n, diag, dtype)
        self.coef, self.ref = {}, {}
        oracle.set_threads(16)
        try:
            for m in degrees:
                M, self.coef[m] = C.apply_coefficients(m, self.dinv)
                self.ref[m] = mirror(oracle, crow, col, val, M, self.r, dtype=dtype)
        finally:
            oracle.set_threads(1)
        self.rd, self.dd = torch.from_numpy(self.r).to(DEV), torch.from_numpy(self.dinv).to(DEV)
        self.r0, self.d0 = self.rd.clone(), self.dd.clone()
        self.failures = []

    def run(self, cid, h, degree, monkeypatch, fused, note=None, note_end=None):
        monkeypatch.setenv("HIPK_CHEB_FUSED", fused)
        cid = f"{cid} degree={degree} fused={fused}"
        print(cid, flush=True)
        z = self.hipk.cheb_apply(h, degree, self.dd, self.coef[degree], self.rd)
        got = self.hipk.CsrHandle.last_spmv_kernel()
        z = z.cpu().numpy()
        if note is not None and got != note:
            self.failures.append(f"{cid}: kernel {got}, expected {note}")
        if note_end is not None and not got.endswith(note_end):
            self.failures.append(f"{cid}: kernel {got}, expected ... {note_end}")
        if not (torch.equal(self.rd, self.r0) and torch.equal(self.dd, self.d0)):
            self.failures.append(f"{cid}: r or dinv changed")
        d = _differs(z, self.ref[degree])
        if d is not None:
            self.failures.append(f"{cid} [{got}]: {d}")

    def done(self):
        assert not self.failures, "\n".join(self.failures)


# ---------------------------------------------------------------------------------------------- 1. the apply, every instantiation
@pytest.mark.parametrize("name", sorted(C.BANDS))
def test_apply_every_instantiation_ragged(hipk, oracle, monkeypatch, name):
    case = C.BANDS[name]
    crow, col, val, diag = C.band(C.N_BIG, case["offsets"])
    ap = _Apply(hipk, oracle, crow, col, val, diag)
    if case["wide"] is not None:
        # the switch is set before the handle exists, a handle per setting: the handle caches its kernel choice
        for strided in (0, 1):
            monkeypatch.setenv("HIPK_SPMV_SELL_STRIDED", str(strided))
            h = make_handle(hipk, crow, col, val, C.N_BIG)
            assert h.path() == "coded"
            for degree in C.DEGREES:
                ap.run(f"{name} strided={strided}", h, degree, monkeypatch, "1", note=case["wide"][strided])
                ap.run(f"{name} strided={strided}", h, degree, monkeypatch, "0", note=C.two_launches(case["wide"][strided]))
            h.close()
        monkeypatch.delenv("HIPK_SPMV_SELL_STRIDED")
    h = make_handle(hipk, crow, col, val, C.N_BIG)
    assert h.path() == "coded"
    if case["wide"] is None:
        # tile widths 6 and 9: not the two-rows-per-lane kernel, and the one-row-per-lane coded kernels have no epilogue
        for degree in C.DEGREES:
            for fused in ("1", "0"):
                ap.run(f"{name} default path", h, degree, monkeypatch, fused, note_end=C.STEP64)
                assert "sell_wide" not in hipk.CsrHandle.last_spmv_kernel()
    h.set_path(plain_only=True)
    for degree in C.DEGREES:
        ap.run(f"{name} plain", h, degree, monkeypatch, "1", note=case["plain"])
        ap.run(f"{name} plain", h, degree, monkeypatch, "0", note=C.two_launches(case["plain"]))
    h.close()
    ap.done()


@pytest.mark.parametrize("name", sorted(C.GRIDS))
def test_apply_masked_tiles(hipk, oracle, monkeypatch, name):
    """HIPK_SPMV_MASKED=1 on grids whose line ends lie inside the matrix: the tiles that hold a line end go through the
    two-rows-per-lane path with a per-row presence mask (row_mask) -- tile widths 4, 5 and 8 (d loaded late), both walks.  That the
    handle really built masked tiles is read from its byte count: a masked tile streams one word and 256 mask bytes in place of its
    `width` code planes of 256 bytes, and the number of such tiles is the one tests/_cheb_cases.py: dispatch_keys computes."""
    nx, ny, steps, diag, notes, width = C.GRIDS[name]
    n = nx * ny
    crow, col, val, _ = C.grid(name)
    masked = C.dispatch_keys(crow, col, val)["masked"]
    assert masked > 0
    ap = _Apply(hipk, oracle, crow, col, val, diag)
    monkeypatch.setenv("HIPK_SPMV_MASKED", "0")
    h = make_handle(hipk, crow, col, val, n)
    plain_bytes = h.format_bytes()
    h.close()
    monkeypatch.setenv("HIPK_SPMV_MASKED", "1")
    for strided in (0, 1):
        monkeypatch.setenv("HIPK_SPMV_SELL_STRIDED", str(strided))
        h = make_handle(hipk, crow, col, val, n)
        assert h.path() == "coded"
        print(f"{name}: {masked} masked tiles expected, format bytes {plain_bytes} -> {h.format_bytes()}", flush=True)
        if plain_bytes - h.format_bytes() != masked * 256 * (width - 1):
            ap.failures.append(f"{name} strided={strided}: format bytes {plain_bytes} -> {h.format_bytes()}, expected a drop of "
                               f"{masked} masked tiles x 256 x {width - 1}")
        for degree in C.DEGREES:
            ap.run(f"{name} masked=1 strided={strided}", h, degree, monkeypatch, "1", note=notes[strided])
            ap.run(f"{name} masked=1 strided={strided}", h, degree, monkeypatch, "0", note=C.two_launches(notes[strided]))
        h.close()
    ap.done()


def test_apply_fp32_plain_ragged(hipk, oracle, monkeypatch):
    crow, col, val, diag = C.band(C.N_BIG, C.BANDS["band5"]["offsets"])
    ap = _Apply(hipk, oracle, crow, col, val.astype(np.float32), diag, dtype=np.float32)
    h = make_handle(hipk, crow, col, val, C.N_BIG, dtype=torch.float32)
    h.set_path(plain_only=True)
    for degree in C.DEGREES:
        ap.run("band5 f32 plain", h, degree, monkeypatch, "1", note="hipk_spmv_cheb_kernel<float,2048>")
        ap.run("band5 f32 plain", h, degree, monkeypatch, "0", note="hipk_spmv_kernel<float,2048,true>" + C.STEP32)
    h.close()
    ap.done()


def test_apply_grouped_walk_at_a_small_size(hipk, oracle, monkeypatch):
    n = C.SMALL_N_WIDE
    crow, col, val, diag = C.band(n, C.SMALL_OFFSETS)
    ap = _Apply(hipk, oracle, crow, col, val, diag)
    monkeypatch.setenv("HIPK_SPMV_SELL_STRIDED", "1")
    h = make_handle(hipk, crow, col, val, n)
    assert h.path() == "coded"
    for degree in C.DEGREES:
        ap.run(f"n={n} strided=1", h, degree, monkeypatch, "1", note=C.SMALL_WIDE)
        ap.run(f"n={n} strided=1", h, degree, monkeypatch, "0", note=C.two_launches(C.SMALL_WIDE))
    h.close()
    ap.done()


@pytest.mark.parametrize("n", C.SMALL_NS)
def test_apply_sizes_below_a_few_tiles(hipk, oracle, monkeypatch, n):
    """No or exactly half of the tiles uniform: whichever form the library takes, the call succeeds and the bits are the
    mirror's (hipk_cheb_init_kernel / hipk_cheb_step_kernel and the (n + 3) & ~3 work layout at n = 1, 2, 3, 5, ...)."""
    crow, col, val, diag = C.band(n, C.SMALL_OFFSETS)
    ap = _Apply(hipk, oracle, crow, col, val, diag)
    for strided in ("0", "1"):
        monkeypatch.setenv("HIPK_SPMV_SELL_STRIDED", strided)
        h = make_handle(hipk, crow, col, val, n)
        for degree in C.DEGREES:
            for fused in ("1", "0"):
                ap.run(f"n={n} strided={strided}", h, degree, monkeypatch, fused)
        h.close()
    ap.done()


# ---------------------------------------------------------------------------------------------- 2. the README's sizes
@pytest.mark.parametrize("nx", sorted(C.POISSON_SIZES))
def test_preconditioner_at_the_quoted_sizes(hipk, oracle, monkeypatch, nx):
    """N = 4 M (chunks of 2048 rows, the last ragged), 16 M (chunks of 8192: the grouped walk by default) against the mirror;
    N = 64 M (chunks of 32768): one launch per step against SpMV + hipk_cheb_step_kernel on the device -- both forms are tied to
    the mirror at the sizes below, a 64 M-row CPU mirror is not run."""
    from pytorch_sparse_solver.module_a import ChebyshevPreconditioner
    from pytorch_sparse_solver.utils.matrix_utils import create_poisson_2d_csr
    one = C.POISSON_SIZES[nx]
    two = C.two_launches(one)
    A = create_poisson_2d_csr(nx, nx, device=DEV)
    n = nx * nx
    M = ChebyshevPreconditioner(A, degree=3)
    r = torch.randn(n, dtype=torch.float64, device=DEV, generator=torch.Generator(device=DEV).manual_seed(nx))
    r0 = r.clone()
    try:
        out = {}
        for fused, note in (("1", one), ("0", two)):
            monkeypatch.setenv("HIPK_CHEB_FUSED", fused)
            print(f"poisson {nx} x {nx} fused={fused}", flush=True)
            out[fused] = M(r)
            got = hipk.CsrHandle.last_spmv_kernel()
            assert got == note, got
            assert torch.equal(r, r0)
        assert torch.equal(out["1"].view(torch.int64), out["0"].view(torch.int64))
        assert (M.applies, M.spmvs) == (2, 6)
        if nx <= 4000:
            crow, col, val = (t.cpu().numpy() for t in (A.crow_indices(), A.col_indices(), A.values()))
            oracle.set_threads(16)
            try:
                ref = mirror(oracle, crow, col, val, M, r.cpu().numpy())
            finally:
                oracle.set_threads(1)
            d = _differs(out["1"].cpu().numpy(), ref)
            assert d is None, d
    finally:
        del M, A
        hipk.clear_cache()


# ---------------------------------------------------------------------------------------------- 3. whole solves
def _torch_recurrence(hipk, A, M):
    """The documented recurrence as a plain callable: hipk.spmv on a handle of its own, separate torch element-wise operations
    (every step rounds on its own), coefficients rounded to the working dtype once."""
    dt = A.values().dtype
    h = hipk.CsrHandle(A.crow_indices(), A.col_indices(), A.values(), A.shape)
    c = lambda x: torch.tensor(x, dtype=dt, device=DEV)
    c0, c1, c2, scale = c(M.c0), [c(x) for x in M.c1], [c(x) for x in M.c2], c(M.scale)
    dinv = M.dinv.to(device=DEV, dtype=dt).clone()

    def apply(v):
        v = v.contiguous()
        d = c0 * (dinv * v)
        z = d
        for k in range(M.degree):
            res = dinv * (v - hipk.spmv(h, z))
            d = (c1[k] * d) + (c2[k] * res)
            z = z + d
        if M.scale != 1.0:
            z = scale * z
        return z
    apply.handle = h
    return apply


@pytest.mark.parametrize("cid", sorted(C.SOLVES))
def test_solves_in_which_the_epilogue_runs(hipk, monkeypatch, cid):
    from pytorch_sparse_solver.module_a import ChebyshevPreconditioner, bicgstab, cg, get_last_stats, gmres
    matrix, dtype, solver, degree, kw, plain, note = C.SOLVES[cid]
    A = C.solve_matrix(matrix)
    A = torch.sparse_csr_tensor(A.crow_indices(), A.col_indices(), A.values().to(dtype), size=A.shape).to(DEV)
    n = A.shape[0]
    g = torch.Generator().manual_seed(n)
    b = torch.randn(n, dtype=torch.float64, generator=g).to(dtype).to(DEV)
    x0 = (0.1 * torch.randn(n, dtype=torch.float64, generator=g)).to(dtype).to(DEV)
    solve = {"cg": cg, "bicgstab": bicgstab, "gmres": gmres}[solver]
    step = C.STEP64 if dtype == torch.float64 else C.STEP32
    h = hipk.handle_for(A)
    h.set_path(plain_only=plain)
    own = None
    try:
        res = {}
        for form in ("a", "b", "c"):
            monkeypatch.setenv("HIPK_CHEB_FUSED", "0" if form == "b" else "1")
            M = ChebyshevPreconditioner(A, degree=degree)
            print(f"{cid} ({form})", flush=True)
            if form == "c":
                own = _torch_recurrence(hipk, A, M)
                x, info = solve(A, b, x0=x0, M=own, **kw)
            else:
                # a solve's own last SpMV is its residual product: the step kernel is read from one apply before the solve
                M(b)
                got = hipk.CsrHandle.last_spmv_kernel()
                if form == "a":
                    assert got == note, got
                else:
                    assert got.endswith(step) and ",28," not in got and "cheb_kernel" not in got, got
                x, info = solve(A, b, x0=x0, M=M, **kw)
            st = get_last_stats()
            assert "callable_M" in st.method and st.iterations > 1, (st.method, st.iterations)
            if form != "c":
                assert M.applies > 2 and M.spmvs == degree * M.applies
            res[form] = (x.clone(), info, st.iterations, st.matvecs, st.breakdown)
            print(f"{cid} ({form}): info {info}, {st.iterations} iterations, {st.matvecs} matvecs, breakdown {st.breakdown}", flush=True)
        for form in ("b", "c"):
            assert res[form][1:] == res["a"][1:], (form, res[form][1:], res["a"][1:])
            d = _differs(res[form][0].cpu().numpy(), res["a"][0].cpu().numpy())
            assert d is None, f"({form}) against (a): {d}"
        assert bool(torch.isfinite(res["a"][0]).all())
    finally:
        h.set_path(plain_only=False)
        if own is not None:
            own.handle.close()
        hipk.clear_cache()
