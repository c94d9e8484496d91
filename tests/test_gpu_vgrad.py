"""hipk_csr_grad_values and hipk_batch_grad_values (csrc/hipk_vgrad.hip) on the GPU, fp64 and fp32, bit for bit against the scalar loop
of tests/_vgrad_mirror.py.  In every case g lies between seeded guards (tests/_arena.py) and is prefilled with 0x00, 0xFF and 0x5A:
the three runs must agree, so every element below nnz is written and nothing else is."""
import ctypes

import numpy as np
import pytest
import torch

import _order_cases as OC
import _vgrad_mirror as VM
from _arena import Arena, guard_bytes_for

pytestmark = pytest.mark.gpu

DT = {"f64": (torch.float64, np.float64, np.uint64, 8), "f32": (torch.float32, np.float32, np.uint32, 4)}
FILLS = (0x00, 0xFF, 0x5A)
DEV = "cuda:0"
HIPK_ERR_ARG, HIPK_ERR_ALIGN, HIPK_ERR_UNSUPPORTED = -1, -3, -4
LOOP_MAX = 50_000        # entries up to which the mirror is the scalar loop; beyond, its row-sliced form (pinned to the loop on CPU)


# ------------------------------------------------------------------------------------------------ patterns
def _from_lens(lens, cols_of, n_cols):
    lens = np.asarray(lens, dtype=np.int64)
    crow = np.concatenate([[0], np.cumsum(lens)])
    col = np.concatenate([np.asarray(cols_of(r, int(l)), dtype=np.int64) for r, l in enumerate(lens) if l] or [np.zeros(0, np.int64)])
    assert len(col) == crow[-1] and (len(col) == 0 or (col.min() >= 0 and col.max() < n_cols))
    return len(lens), n_cols, crow, col


def tridiag(n, empty=()):
    def cols(r, l):
        return [c for c in (r - 1, r, r + 1) if 0 <= c < n]
    lens = [0 if r in empty else len(cols(r, 0)) for r in range(n)]
    return _from_lens(lens, cols, n)


def stencil(dims, offsets):
    """The stencil with `offsets` (tuples) on a grid of `dims`, rows in ascending column order."""
    dims = tuple(dims)
    idx = np.arange(int(np.prod(dims))).reshape(dims)
    rows, cols = [], []
    for off in offsets:
        src = tuple(slice(max(0, -o), d - max(0, o)) for o, d in zip(off, dims))
        dst = tuple(slice(max(0, o), d - max(0, -o)) for o, d in zip(off, dims))
        rows.append(idx[src].reshape(-1))
        cols.append(idx[dst].reshape(-1))
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    order = np.lexsort((cols, rows))
    n = idx.size
    return n, n, np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]), cols[order]


def grid5(nx, ny):
    return stencil((ny, nx), [(0, 0), (0, 1), (0, -1), (1, 0), (-1, 0)])


def transformed(case, name):
    n, m, crow, col = case
    crow2, col2, _ = OC.TRANSFORMS[name](crow, col, np.zeros(len(col)), seed=2)
    return n, m, crow2, col2


def long_row():
    rng = np.random.default_rng(600)
    return _from_lens([5000 if r == 300 else 1 for r in range(600)], lambda r, l: rng.integers(0, 600, l) if l > 1 else [r], 600)


def seeded_lens(n, hi, n_cols, seed):
    rng = np.random.default_rng(seed)
    return _from_lens(rng.integers(0, hi + 1, n), lambda r, l: rng.integers(0, n_cols, l), n_cols)


SINGLE = {
    "n1_one_entry": lambda: (1, 1, np.array([0, 1]), np.array([0])),
    "n1_three_entries_in_column_0": lambda: (1, 1, np.array([0, 3]), np.array([0, 0, 0])),
    "tridiag255": lambda: tridiag(255), "tridiag256": lambda: tridiag(256), "tridiag257": lambda: tridiag(257),
    "first_row_empty": lambda: tridiag(300, empty=(0,)), "last_row_empty": lambda: tridiag(300, empty=(299,)),
    "300_empty_rows_over_a_whole_tile": lambda: tridiag(900, empty=range(200, 500)),
    "alternating_empty_rows": lambda: tridiag(601, empty=range(1, 601, 2)),
    "n600_one_row_of_5000": long_row,
    "dense40": lambda: _from_lens([40] * 40, lambda r, l: np.arange(40), 40),
    "poisson17x13": lambda: grid5(17, 13),
    "poisson17x13_reversed": lambda: transformed(grid5(17, 13), "rev"),
    "poisson17x13_shuffled": lambda: transformed(grid5(17, 13), "shuf"),
    "poisson17x13_duplicates": lambda: transformed(grid5(17, 13), "dup_shuf"),
    "convdiff64x64": lambda: grid5(64, 64),
    "seven_point_12x12x12": lambda: stencil((12, 12, 12), [(0, 0, 0), (0, 0, 1), (0, 0, -1), (0, 1, 0), (0, -1, 0), (1, 0, 0), (-1, 0, 0)]),
    "rectangular300x500": lambda: seeded_lens(300, 6, 500, 35),
    "n70001_row_lengths_0_to_40": lambda: seeded_lens(70001, 40, 70001, 71),
    "poisson1000x1000": lambda: grid5(1000, 1000),
}


def _mirror(crow, col, lam, x, ndt):
    f = VM.grad_values if len(col) <= LOOP_MAX else VM.grad_values_rows
    return f(crow, col, lam, x, ndt)


def _same(got, want, bits, nan=False):
    assert got.shape == want.shape and got.dtype == want.dtype
    if nan:
        assert np.array_equal(np.isnan(got), np.isnan(want))
        ok = ~np.isnan(want)
        return np.array_equal(got[ok].view(bits), want[ok].view(bits))
    return np.array_equal(got.view(bits), want.view(bits))


def _operands(n_rows, n_cols, ndt, seed):
    rng = np.random.default_rng([seed, n_rows, n_cols])
    return rng.standard_normal(n_rows).astype(ndt), rng.standard_normal(n_cols).astype(ndt)


def _run_handle(hipk, case, dt, idx=torch.int32, lam=None, x=None, stream=None, nan=False):
    tdt, ndt, bits, es = DT[dt]
    n_rows, n_cols, crow, col = case
    nnz = len(col)
    L = hipk.lib()
    if lam is None:
        lam, x = _operands(n_rows, n_cols, ndt, 1)
    vals = torch.from_numpy(np.random.default_rng(nnz).standard_normal(nnz).astype(ndt)).to(DEV)
    h = hipk.CsrHandle(torch.as_tensor(crow, dtype=idx, device=DEV), torch.as_tensor(col, dtype=idx, device=DEV), vals, (n_rows, n_cols))
    lam_t, x_t = torch.from_numpy(lam).to(DEV), torch.from_numpy(x).to(DEV)
    lam_0, x_0 = lam_t.clone(), x_t.clone()
    g = Arena(DEV, nnz * es, 16, guard_bytes_for(nnz, es))
    outs = []
    st = torch.cuda.current_stream(DEV) if stream is None else stream
    torch.cuda.synchronize()             # the operands above were made on the default stream
    with torch.cuda.stream(st):
        for fill in FILLS:
            g.fill(fill)
            rc = L.hipk_csr_grad_values(h.ptr, lam_t.data_ptr(), x_t.data_ptr(), g.data_ptr(), st.cuda_stream)
            assert rc == 0, L.hipk_last_error()
            assert L.hipk_last_grad_values_launches() == 1
            st.synchronize()
            assert g.guards_intact(), f"0x{fill:02X} prefill: a write outside g {g.touched()}"
            outs.append(g.view(tdt, nnz).cpu().numpy().copy())
    assert torch.equal(lam_t.view(torch.uint8), lam_0.view(torch.uint8)) and torch.equal(x_t.view(torch.uint8), x_0.view(torch.uint8))
    for o in outs[1:]:
        assert np.array_equal(o.view(bits), outs[0].view(bits)), "the result depends on what g held: an element is not written"
    assert _same(outs[0], _mirror(crow, col, lam, x, ndt), bits, nan=nan), "differs from the mirror"
    h.close()


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("name", sorted(SINGLE))
def test_handle_entry_is_the_mirror(hipk, name, dt):
    _run_handle(hipk, SINGLE[name](), dt)


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_int64_index_handle(hipk, dt):
    _run_handle(hipk, grid5(17, 13), dt, idx=torch.int64)


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_signed_zeros_infinities_and_nans(hipk, dt):
    ndt = DT[dt][1]
    case = grid5(17, 13)
    lam, x = _operands(221, 221, ndt, 2)
    lam[[0, 5, 50, 51]] = [0.0, -0.0, np.inf, -np.inf]
    x[[1, 6, 60, 61, 100]] = [-0.0, 0.0, -np.inf, np.inf, 1.0]
    _run_handle(hipk, case, dt, lam=lam.copy(), x=x.copy())                      # +-0 and +-inf: bitwise (no 0 * inf pair is adjacent)
    lam[120], x[130], x[51] = np.nan, np.nan, 0.0                                # NaN operands, and inf * 0 at the diagonal of row 51
    _run_handle(hipk, case, dt, lam=lam, x=x, nan=True)


def test_side_stream(hipk):
    _run_handle(hipk, grid5(64, 64), "f64", stream=torch.cuda.Stream(DEV))


# ------------------------------------------------------------------------------------------------ the batch entry
def _run_batch(hipk, case, S, dt, pad=(0, 0, 0)):
    """pad: extra 16-byte groups on ldl, ldx, ldg beyond the shortest aligned leading dimension."""
    tdt, ndt, bits, es = DT[dt]
    n, _, crow, col = case
    nnz = len(col)
    per = 16 // es
    up = lambda v: (v + per - 1) // per * per
    ldl, ldx, ldg = up(n) + pad[0] * per, up(n) + pad[1] * per, up(nnz) + pad[2] * per
    rng = np.random.default_rng([S, n, nnz])
    Lb, Xb = rng.standard_normal((S, ldl)).astype(ndt), rng.standard_normal((S, ldx)).astype(ndt)     # the padding is seeded too
    L = hipk.lib()
    crow_t, col_t = torch.as_tensor(crow, dtype=torch.int32, device=DEV), torch.as_tensor(col, dtype=torch.int32, device=DEV)
    lam_t, x_t = torch.from_numpy(Lb).to(DEV), torch.from_numpy(Xb).to(DEV)
    lam_0, x_0 = lam_t.clone(), x_t.clone()
    g = Arena(DEV, S * ldg * es, 16, guard_bytes_for(ldg, es))
    st = torch.cuda.current_stream(DEV)
    outs = []
    for fill in FILLS:
        g.fill(fill)
        rc = L.hipk_batch_grad_values(n, nnz, crow_t.data_ptr(), col_t.data_ptr(), S, lam_t.data_ptr(), ldl, x_t.data_ptr(), ldx,
                                      g.data_ptr(), ldg, hipk._dtype_code(tdt), st.cuda_stream)
        assert rc == 0, L.hipk_last_error()
        assert L.hipk_last_grad_values_launches() == 1
        st.synchronize()
        assert g.guards_intact(), f"0x{fill:02X} prefill: a write outside g {g.touched()}"
        full = g.view(tdt, S * ldg).cpu().numpy().copy().reshape(S, ldg)
        tail = np.ascontiguousarray(full[:, nnz:]).view(np.uint8)
        assert np.all(tail == fill), "an element of a g row at or beyond nnz was written"
        outs.append(np.ascontiguousarray(full[:, :nnz]))
    assert torch.equal(lam_t.view(torch.uint8), lam_0.view(torch.uint8)) and torch.equal(x_t.view(torch.uint8), x_0.view(torch.uint8))
    for o in outs[1:]:
        assert np.array_equal(o.view(bits), outs[0].view(bits)), "the result depends on what g held: an element is not written"
    want = VM.batch_grad_values(crow, col, Lb[:, :n], Xb[:, :n], ndt, fast=S * nnz > LOOP_MAX)
    assert _same(outs[0], want, bits), "differs from the mirror"


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("S", [1, 3, 17, 1030, 2500])
def test_batch_entry_on_the_7x5_grid(hipk, S, dt):
    """fp32: nnz = 151 is odd.  S = 1030 runs slices of 2 systems, S = 2500 slices of 3 with a last slice of one."""
    case = grid5(7, 5)
    assert len(case[3]) == 151
    _run_batch(hipk, case, S, dt)


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_batch_entry_beyond_the_solve_envelope(hipk, dt):
    _run_batch(hipk, tridiag(4097), 5, dt)
    _run_batch(hipk, long_row(), 3, dt)                      # a row of 5000 entries: the batch solves' 32-entry limit does not apply


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_batch_entry_with_padded_leading_dimensions(hipk, dt):
    _run_batch(hipk, transformed(grid5(17, 13), "dup_shuf"), 9, dt, pad=(1, 2, 3))
    _run_batch(hipk, tridiag(300, empty=(0, 299)), 20, dt, pad=(2, 1, 1))


# ------------------------------------------------------------------------------------------------ no launch, errors
def test_nnz_zero_and_batch_zero_take_no_launch(hipk):
    L = hipk.lib()
    _run_handle(hipk, grid5(7, 5), "f64")                                        # leaves the launch count at 1
    crow = torch.zeros(6, dtype=torch.int32, device=DEV)
    lam, x = torch.ones(5, dtype=torch.float64, device=DEV), torch.ones(5, dtype=torch.float64, device=DEV)
    g = Arena(DEV, 64, 16, 4096).fill(0x5A).snapshot()
    st = torch.cuda.current_stream(DEV).cuda_stream
    assert L.hipk_batch_grad_values(5, 0, crow.data_ptr(), None, 1, lam.data_ptr(), 5, x.data_ptr(), 5, g.data_ptr(), 0, 1, st) == 0
    assert L.hipk_last_grad_values_launches() == 0
    _run_handle(hipk, grid5(7, 5), "f64")
    assert L.hipk_batch_grad_values(5, 8, crow.data_ptr(), crow.data_ptr(), 0, lam.data_ptr(), 5, x.data_ptr(), 5, g.data_ptr(), 8, 1, st) == 0
    assert L.hipk_last_grad_values_launches() == 0
    torch.cuda.synchronize()
    assert g.unchanged() and g.guards_intact()


def test_every_error_code_leaves_g_untouched(hipk):
    L = hipk.lib()
    n, _, crow, col = grid5(7, 5)
    nnz = len(col)
    crow_t, col_t = torch.as_tensor(crow, dtype=torch.int32, device=DEV), torch.as_tensor(col, dtype=torch.int32, device=DEV)
    buf = torch.ones(4 * 40 + 2, dtype=torch.float64, device=DEV)
    lam, x = buf[:160], buf.clone()[:160]
    g = Arena(DEV, 4 * 152 * 8, 16, 4096).fill(0x5A).snapshot()
    st = torch.cuda.current_stream(DEV).cuda_stream
    P = lambda t: t.data_ptr()
    ok = dict(n=n, nnz=nnz, crow=P(crow_t), col=P(col_t), batch=4, lam=P(lam), ldl=40, x=P(x), ldx=40, g=g.data_ptr(), ldg=152, dtype=1)

    def call(**kw):
        a = dict(ok, **kw)
        rc = L.hipk_batch_grad_values(a["n"], a["nnz"], a["crow"], a["col"], a["batch"], a["lam"], a["ldl"], a["x"], a["ldx"], a["g"], a["ldg"],
                                      a["dtype"], st)
        assert L.hipk_last_grad_values_launches() == 0 or rc == 0
        return rc

    for kw in (dict(crow=None), dict(col=None), dict(lam=None), dict(x=None), dict(g=None), dict(n=-1), dict(nnz=-1), dict(batch=-1),
               dict(ldl=n - 1), dict(ldx=n - 1), dict(ldg=nnz - 1), dict(lam=g.data_ptr()), dict(x=g.data_ptr())):
        assert call(**kw) == HIPK_ERR_ARG, kw
    for kw in (dict(g=g.data_ptr() + 8), dict(lam=P(lam) + 8), dict(x=P(x) + 8), dict(col=P(col_t) + 4), dict(crow=P(crow_t) + 4),
               dict(ldl=37), dict(ldx=39), dict(ldg=151)):
        assert call(**kw) == HIPK_ERR_ALIGN, kw
    for code in (2, -1, 7):
        assert call(dtype=code) == HIPK_ERR_UNSUPPORTED, code
    torch.cuda.synchronize()
    assert g.unchanged() and g.guards_intact(), "an error return of the batch entry wrote to g"
    # the handle entry
    vals = torch.ones(nnz, dtype=torch.float64, device=DEV)
    h = hipk.CsrHandle(crow_t, col_t, vals, (n, n))
    hcall = lambda hp, l, xx, gg: L.hipk_csr_grad_values(hp, l, xx, gg, st)
    assert hcall(None, P(lam), P(x), g.data_ptr()) == HIPK_ERR_ARG
    assert hcall(h.ptr, None, P(x), g.data_ptr()) == HIPK_ERR_ARG
    assert hcall(h.ptr, P(lam), None, g.data_ptr()) == HIPK_ERR_ARG
    assert hcall(h.ptr, P(lam), P(x), None) == HIPK_ERR_ARG
    assert hcall(h.ptr, g.data_ptr(), P(x), g.data_ptr()) == HIPK_ERR_ARG
    assert hcall(h.ptr, P(lam), g.data_ptr(), g.data_ptr()) == HIPK_ERR_ARG
    assert hcall(h.ptr, P(lam) + 8, P(x), g.data_ptr()) == HIPK_ERR_ALIGN
    assert hcall(h.ptr, P(lam), P(x) + 8, g.data_ptr()) == HIPK_ERR_ALIGN
    assert hcall(h.ptr, P(lam), P(x), g.data_ptr() + 8) == HIPK_ERR_ALIGN
    assert L.hipk_last_grad_values_launches() == 0
    torch.cuda.synchronize()
    assert g.unchanged() and g.guards_intact(), "an error return of the handle entry wrote to g"
    h.close()
    # last, what is NOT an error: one system needs no alignment of its leading dimensions (and this call does write g)
    assert call(batch=1, ldl=37, ldx=39, ldg=151) == 0
    assert L.hipk_last_grad_values_launches() == 1
    torch.cuda.synchronize()
    assert not g.unchanged() and g.guards_intact()


# ------------------------------------------------------------------------------------------------ the binding
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_binding_takes_misaligned_and_strided_views(hipk, dt):
    tdt, ndt, bits, es = DT[dt]
    n, _, crow, col = grid5(7, 5)
    nnz = len(col)
    rng = np.random.default_rng(77)
    crow_t, col_t = torch.as_tensor(crow, dtype=torch.int32, device=DEV), torch.as_tensor(col, dtype=torch.int32, device=DEV)
    h = hipk.CsrHandle(crow_t, col_t, torch.ones(nnz, dtype=tdt, device=DEV), (n, n))
    lam, x = rng.standard_normal(n + 1), rng.standard_normal(2 * n)
    lam_v, x_v = torch.from_numpy(lam).to(DEV)[1:], torch.from_numpy(x).to(DEV)[::2]          # fp64 operands: cast to the handle's dtype
    want = VM.grad_values(crow, col, lam[1:], x[::2], ndt)
    got = hipk.csr_grad_values(h, lam_v, x_v)
    assert _same(got.cpu().numpy(), want, bits)
    st = hipk.last_grad_stats()
    assert (st.route, st.launches, st.nnz, st.batch) == ("kernel", 1, nnz, 1)
    out = torch.zeros(nnz + 1, dtype=tdt, device=DEV)[1:]
    assert hipk.csr_grad_values(h, lam_v, x_v, out=out) is out and _same(out.cpu().numpy(), want, bits)
    S = 3
    Lb, Xb = rng.standard_normal((S, n)).astype(ndt), rng.standard_normal((S, n)).astype(ndt)         # n = 35: rows start misaligned
    G = hipk.batch_grad_values(n, nnz, crow_t, col_t, torch.from_numpy(Lb).to(DEV), torch.from_numpy(Xb).to(DEV))
    assert tuple(G.shape) == (S, nnz) and _same(G.cpu().numpy(), VM.batch_grad_values(crow, col, Lb, Xb, ndt), bits)
    st = hipk.last_grad_stats()
    assert (st.route, st.launches, st.nnz, st.batch) == ("kernel", 1, nnz, S)
    out = torch.zeros((S, nnz), dtype=tdt, device=DEV)
    assert hipk.batch_grad_values(n, nnz, crow_t, col_t, torch.from_numpy(Lb).to(DEV), torch.from_numpy(Xb).to(DEV), out=out) is out
    assert _same(out.cpu().numpy(), VM.batch_grad_values(crow, col, Lb, Xb, ndt), bits)
    h.close()
