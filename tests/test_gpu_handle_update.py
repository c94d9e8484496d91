"""hipk_csr_update_values / CsrHandle.update_values / refresh_matrix: new values on the pattern of an existing handle.

The reference of every comparison is a FRESH CsrHandle on the same index arrays and the new values (and the oracle's SpMV for the
transpose): path, format bytes, the kernel note of every hipk_spmv_ex mode (the mode list of tests/test_gpu_spmv_instantiations.py),
y and the fused-dot partials bit for bit, and for solves x, the statistics, hipk_last_solve_path and hipk_last_solve_form.  The kind
of every update (hipk_last_csr_update_kind: 1 values only, 2 re-encoded in place, 3 form changed) is asserted literally, so an
update that silently rebuilt everything cannot pass."""
import numpy as np
import pytest
import torch

import _order_cases as OC
import _spmv_cases as C
from _arena import Arena, guard_bytes_for
from test_gpu_coded import banded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float64, torch.float32]
IDS = ["fp64", "fp32"]


# ------------------------------------------------------------------------------------------------------------ helpers
def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _vectors(n, dtype, seed=1):
    g = torch.Generator().manual_seed(seed + n)
    return tuple(torch.randn(n, dtype=torch.float64, generator=g).to(dtype).to(DEV) for _ in range(3))


def _all_modes(hipk, h, x, w, b):
    """[(mode, note, y, <w, y> partials, <y, y> partials)] of every hipk_spmv_ex mode, as bytes."""
    L = hipk.lib()
    n, G = h.n, int(L.hipk_chunk_count(h.n))
    out = []
    for mode, _wx in C.RUNS:
        y = torch.full((n,), float("nan"), dtype=h.dtype, device=DEV)
        p0 = torch.full((G,), float("nan"), dtype=torch.float64, device=DEV)
        p1 = torch.full((G,), float("nan"), dtype=torch.float64, device=DEV)
        with h._lock:
            hipk._check(L.hipk_spmv_ex(h._h, x.data_ptr(), y.data_ptr(), mode, w.data_ptr(), b.data_ptr(), p0.data_ptr(), p1.data_ptr(),
                                       None, 0, torch.cuda.current_stream().cuda_stream), "hipk_spmv_ex")
        out.append((mode, hipk.CsrHandle.last_spmv_kernel(), y.cpu().numpy().tobytes(),
                    p0.cpu().numpy().tobytes() if mode & 1 else b"", p1.cpu().numpy().tobytes() if mode & 2 else b""))
    return out


def _is_fresh(hipk, h, crow, col, val, path=None, vectors=None, plain_only=False):
    """`h` (updated to `val`) against a fresh handle on the same arrays: path, format bytes, notes and bits of every mode."""
    n = h.n
    x, w, b = vectors if vectors is not None else _vectors(h.shape[1] if h.shape[1] != n else n, h.dtype)
    fresh = hipk.CsrHandle(crow, col, val.clone(), h.shape)
    try:
        if plain_only:
            fresh.set_path(plain_only=True)
        assert h.path() == fresh.path() and (path is None or h.path() == path), (h.path(), fresh.path(), path)
        assert h.format_bytes() == fresh.format_bytes(), (h.format_bytes(), fresh.format_bytes())
        assert h.device_bytes() == fresh.device_bytes()
        got, want = _all_modes(hipk, h, x, w, b), _all_modes(hipk, fresh, x, w, b)
        for g, f in zip(got, want):
            assert g[1] == f[1], f"mode {g[0]}: kernel {g[1]}, the fresh handle's {f[1]}"
            assert g[2] == f[2], f"mode {g[0]} [{g[1]}]: y differs from the fresh handle's"
            assert g[3] == f[3] and g[4] == f[4], f"mode {g[0]} [{g[1]}]: fused-dot partials differ from the fresh handle's"
        return got[0][1]
    finally:
        fresh.close()


def _update(hipk, h, val, kind):
    assert h.update_values(val) is h
    assert hipk.CsrHandle.last_update_kind() == kind, (hipk.CsrHandle.last_update_kind(), kind)


def _grid(nx, ny, kind, dtype, seed=0, idx=torch.int64):
    """(crow, col, values) on the device of the 5-point Poisson ("c") or variable-diffusion ("v", a coefficient field per seed) matrix."""
    from pytorch_sparse_solver.utils.matrix_utils import create_poisson_2d_csr, create_variable_diffusion_2d_csr
    A = create_poisson_2d_csr(nx, ny) if kind == "c" else create_variable_diffusion_2d_csr(nx, ny, contrast=2.0, seed=seed)
    return A.crow_indices().to(idx).to(DEV), A.col_indices().to(idx).to(DEV), A.values().to(dtype).to(DEV)


def _random_pattern(n, per_row, seed):
    """A matrix with `per_row` random columns per row (diagonal included): hundreds of distinct offsets, so neither coded form."""
    rng = np.random.default_rng(seed)
    cols = np.sort(np.concatenate([rng.integers(0, n, (n, per_row - 1)), np.arange(n)[:, None]], axis=1), axis=1)
    crow = np.arange(n + 1, dtype=np.int64) * per_row
    return crow, cols.reshape(-1).astype(np.int64), rng.standard_normal(n * per_row)


# ------------------------------------------------------------------------------------------------------------ 1. the form is kept
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("grid", [(100, 100), (70, 73)], ids=["100x100", "70x73"])
def test_poisson_times_two_is_reencoded_in_place(hipk, grid, dtype):
    """n = 10 000 > 8192: the sample pass runs; 70 x 73 = 5110: a ragged last tile.  int64 indices at creation on the first grid."""
    crow, col, val = _grid(*grid, "c", dtype, idx=torch.int64 if grid == (100, 100) else torch.int32)
    h = hipk.CsrHandle(crow, col, val, (crow.numel() - 1,) * 2)
    assert h.path() == "coded"
    _update(hipk, h, val * 2, 2)
    _is_fresh(hipk, h, crow, col, val * 2, path="coded")
    h.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_layout_csr_is_reencoded_in_place(hipk, monkeypatch, dtype):
    monkeypatch.setenv(C.LAYOUT, "csr")
    crow, col, val = _grid(70, 73, "c", dtype)
    h = hipk.CsrHandle(crow, col, val, (5110, 5110))
    _update(hipk, h, val * 2, 2)
    note = _is_fresh(hipk, h, crow, col, val * 2, path="coded")
    assert note.startswith("hipk_spmv_coded_kernel<"), note
    h.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("grid", [(100, 100), (70, 73)], ids=["100x100", "70x73"])
def test_a_new_coefficient_field_rewrites_the_value_planes_only(hipk, grid, dtype):
    crow, col, val = _grid(*grid, "v", dtype, seed=1)
    new = _grid(*grid, "v", dtype, seed=2)[2]
    assert not torch.equal(val, new)
    h = hipk.CsrHandle(crow, col, val, (crow.numel() - 1,) * 2)
    assert h.path() == "offset_coded"
    _update(hipk, h, new, 1)
    _is_fresh(hipk, h, crow, col, new, path="offset_coded")
    h.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_plain_matrix_stays_plain(hipk, dtype):
    crow, col, val = _random_pattern(3001, 6, seed=4)
    crow, col, val = _dev(crow), _dev(col), _dev(val, dtype)
    h = hipk.CsrHandle(crow, col, val, (3001, 3001))
    assert h.path() == "tile_fast"
    _update(hipk, h, val * 3 + 1, 1)
    _is_fresh(hipk, h, crow, col, val * 3 + 1, path="tile_fast")
    h.close()


@pytest.mark.parametrize("width,dtype", [(32, torch.float64), (31, torch.float64), (32, torch.float32)], ids=["fp64_w32", "fp64_w31", "fp32_w32"])
def test_dense_tiles_at_the_lds_bound_of_the_staged_rewrite(hipk, width, dtype):
    """A band of `width` offsets with per-entry values, n = 1030 (four full tiles and a ragged one): offset-coded, rows of up to 32
    entries.  fp64, 32 wide: an interior tile holds 256 x 32 = 8192 values = 64 KB, with the slack of the aligned start more than
    the staged form may take, so the update runs hipk_csr_revalue_rows_kernel; 31 wide: 7936 values, 63 504 bytes with the slack,
    the staged form just below its bound; fp32, 32 wide: 32 784 bytes, staged.  Then the OTHER form is run on the same handle
    through hipk_csr_revalue_probe (where it may run) after an in-place change of the borrowed values, so each form's planes are
    held against a fresh handle."""
    n = 1030
    offsets = list(range(-16, 16)) if width == 32 else list(range(-15, 16))
    rng = np.random.default_rng(width)
    crow, col, val = banded(n, offsets, lambda r, k: rng.standard_normal(len(r)))
    assert int(np.diff(crow).max()) == width and int((crow[512] - crow[256])) == 256 * width
    crow, col, first = _dev(crow), _dev(col), _dev(val, dtype)
    new = _dev(rng.standard_normal(len(val)), dtype)
    h = hipk.CsrHandle(crow, col, first, (n, n))
    assert h.path() == "offset_coded"
    _update(hipk, h, new, 1)
    _is_fresh(hipk, h, crow, col, new, path="offset_coded")
    L, stream = hipk.lib(), torch.cuda.current_stream().cuda_stream
    staged_fits = (256 * width + 16 // new.element_size()) * new.element_size() <= 65536   # the tile's values + one 16-byte group
    for form in (1, 2) if staged_fits else (1,):
        new.mul_(-1.5)                                             # the planes still hold the values before this
        with h._lock:
            hipk._check(L.hipk_csr_revalue_probe(h._h, form, stream), "hipk_csr_revalue_probe")
        _is_fresh(hipk, h, crow, col, new, path="offset_coded")
    h.close()


# ------------------------------------------------------------------------------------------------------------ 2. the form changes
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_constant_to_variable_coefficients_and_back(hipk, dtype):
    crow, col, const = _grid(100, 100, "c", dtype)
    var = _grid(100, 100, "v", dtype, seed=3)[2]
    h = hipk.CsrHandle(crow, col, const, (10_000, 10_000))
    for val, path in ((var, "offset_coded"), (const, "coded"), (var, "offset_coded")):
        _update(hipk, h, val, 3)
        _is_fresh(hipk, h, crow, col, val, path=path)
    h.close()


def test_the_sample_passes_and_the_full_pass_decides(hipk):
    """The leading 4096 rows carry few pairs, so the sample lets the attempt go on; the rows beyond decide -- once against the pair
    dictionary (per-entry values there), once for it (a few more pairs there)."""
    crow, col, const = _grid(100, 100, "c", torch.float64)
    var = _grid(100, 100, "v", torch.float64, seed=3)[2]
    cut = int(crow[4096])
    mixed = torch.cat([const[:cut], var[cut:]])
    few = const.clone()
    few[cut:] *= (1 + torch.arange(const.numel() - cut, device=DEV) % 7).to(torch.float64)
    h = hipk.CsrHandle(crow, col, var, (10_000, 10_000))
    assert h.path() == "offset_coded"
    _update(hipk, h, mixed, 1)
    _is_fresh(hipk, h, crow, col, mixed, path="offset_coded")
    _update(hipk, h, few, 3)
    _is_fresh(hipk, h, crow, col, few, path="coded")
    h.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_uniform_tile_words_come_go_and_come_back(hipk, dtype):
    """A constant band: all tiles but the first and last are uniform.  With a value per (offset, row mod 3) the matrix still has
    15 pairs, but no tile whose rows agree: the words are dropped, format_bytes says so, and they come back."""
    crow, col, val = banded(10_000, [-40, -1, 0, 1, 40], lambda r, k: (k + 1.0) / 7.0 - 0.9)
    rows = np.repeat(np.arange(10_000), np.diff(crow))
    crow, col, uni, mixed = _dev(crow), _dev(col), _dev(val, dtype), _dev(val * (1 + rows % 3), dtype)
    h = hipk.CsrHandle(crow, col, uni, (10_000, 10_000))
    with_words = h.format_bytes()
    for val, same in ((mixed, False), (uni, True), (mixed, False)):
        _update(hipk, h, val, 2)
        _is_fresh(hipk, h, crow, col, val, path="coded")
        assert (h.format_bytes() == with_words) == same
    h.close()


# ------------------------------------------------------------------------------------------------------------ 3. edges
def _edge(name):
    """(crow, col, first values, new values, shape) as numpy, fp64."""
    rng = np.random.default_rng(len(name))
    if name == "n1":
        return np.array([0, 1]), np.array([0]), np.array([2.0]), np.array([-3.5]), 1
    if name == "n257":
        crow, col, val = banded(257, [-1, 0, 1], lambda r, k: np.asarray([-1.0, 2.0, -1.0])[k])
        return crow, col, val, val * 0.5, 257
    if name == "odd_nnz":
        crow, col, val = banded(300, [-1, 0, 1], lambda r, k: np.asarray([-1.0, 2.0, -1.0])[k])      # nnz = 898; drop the last entry: 897
        crow = crow.copy()
        crow[-1] -= 1
        return crow, col[:-1], val[:-1], rng.standard_normal(len(val) - 1), 300
    if name == "empty_row":
        crow, col, val = banded(600, [-1, 0, 1], lambda r, k: np.asarray([-1.0, 2.0, -1.0])[k])
        keep = np.repeat(np.arange(600), np.diff(crow)) != 300
        lens = np.diff(crow)
        lens[300] = 0
        return np.concatenate([[0], np.cumsum(lens)]), col[keep], val[keep], val[keep] * 3.0, 600
    if name in ("row32", "row33"):                                 # 33 entries: no coded attempt at all
        w = 32 if name == "row32" else 33
        crow, col, val = banded(700, [-1, 0, 1], lambda r, k: np.asarray([-1.0, 2.0, -1.0])[k])
        lens = np.diff(crow)
        at = int(crow[350])
        extra = np.arange(400, 400 + w - lens[350])
        col = np.concatenate([col[:at], extra, col[at:]])
        val = np.concatenate([val[:at], np.full(len(extra), 0.25), val[at:]])
        lens[350] = w
        return np.concatenate([[0], np.cumsum(lens)]), col, val, val * -2.0, 700
    crow, col, val = (a.cpu().numpy() for a in _grid(20, 23, "c", torch.float64))
    crow, col, val = OC.TRANSFORMS["shuf" if name == "unsorted" else "dup"](crow, col, val, seed=2)
    return crow, col, val, val * 1.5, 460


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", ["n1", "n257", "odd_nnz", "empty_row", "row32", "row33", "unsorted", "duplicate"])
def test_edges(hipk, name, dtype):
    crow, col, first, new, n = _edge(name)
    crow, col, first, new = _dev(crow.astype(np.int64)), _dev(col.astype(np.int64)), _dev(first, dtype), _dev(new, dtype)
    h = hipk.CsrHandle(crow, col, first, (n, n))
    before = h.path()
    h.update_values(new)
    kind = hipk.CsrHandle.last_update_kind()
    _is_fresh(hipk, h, crow, col, new)
    if name == "row33":
        assert kind == 1 and h.path() == before == "tile"
        assert int(hipk.lib().hipk_last_csr_update_syncs()) == 0
    elif name != "odd_nnz":                                        # (odd_nnz goes from three pairs to per-entry values)
        assert h.path() == before and kind in (1, 2)
    h.update_values(first)                                         # and back
    _is_fresh(hipk, h, crow, col, first)
    h.close()


def test_a_misaligned_view_and_the_same_pointer_after_an_in_place_change(hipk):
    crow, col, val = _grid(70, 73, "v", torch.float64, seed=1)
    new = _grid(70, 73, "v", torch.float64, seed=5)[2]
    nnz = val.numel()
    buf = torch.empty(nnz + 2, dtype=torch.float64, device=DEV)
    view = buf[1:nnz + 1]
    view.copy_(new)
    assert view.data_ptr() % 16 == 8
    h = hipk.CsrHandle(crow, col, val, (5110, 5110))
    _update(hipk, h, view, 1)
    assert h.val.data_ptr() != view.data_ptr() and h.val.data_ptr() % 16 == 0       # a copy, as in the constructor
    _is_fresh(hipk, h, crow, col, new, path="offset_coded")
    held = h.val
    held.mul_(0.5)                                                 # the tensor the handle borrows, changed in place
    _update(hipk, h, held, 1)
    assert h.val is held
    _is_fresh(hipk, h, crow, col, new * 0.5, path="offset_coded")
    h.close()


# ------------------------------------------------------------------------------------------------------------ 4. per SpMV family
def _family(case):
    """What distinguishes the kernels a case selects: the kernel's name, the loop kernel's CHUNKED and VALS arguments, the grouped walk,
    and whether the plain kernels were forced."""
    note = case["steps"][0][1][0]
    name, _, args = note.partition("<")
    args = args.split(">")[0].split(",")
    key = (name, "/groups" in note, case["plain_only"])
    return key + ((args[2], args[3]) if name == "hipk_spmv_sell_loop_kernel" else ())


def _families():
    """Per family of tests/_spmv_cases.py the smallest in-process case that selects it (rows, then name): derived from the table, so
    it follows the table."""
    best = {}
    for name, case in C.CASES.items():
        if case["fresh"] is None:
            rank = (C.MATRICES[case["matrix"]][0], name)
            fam = _family(case)
            if fam not in best or rank < best[fam][0]:
                best[fam] = (rank, name)
    return sorted(name for _, name in best.values())


FAMILIES = _families()


@pytest.mark.parametrize("name", FAMILIES)
def test_every_spmv_family_after_an_update(hipk, monkeypatch, name):
    case = C.CASES[name]
    for k, v in case["env"].items():
        monkeypatch.setenv(k, v)
    dtype = torch.float64 if case["dtype"] == C.DOUBLE else torch.float32
    crow, col, val = C.matrix(case["matrix"])
    n = len(crow) - 1
    other = np.random.default_rng(3).standard_normal(len(val))
    crow, col, val, other = _dev(crow), _dev(col), _dev(val, dtype), _dev(other, dtype)
    h = hipk.CsrHandle(crow, col, other, (n, n))
    if case["plain_only"]:
        h.set_path(plain_only=True)                                # hipk_csr_set_path's mode is kept by an update
    h.update_values(val)
    vec = tuple(_dev(v) for v in C.vectors(case["matrix"], case["dtype"]))
    _is_fresh(hipk, h, crow, col, val, vectors=vec, plain_only=case["plain_only"])
    want = case["steps"][0][1]
    got = {mode: note for mode, note, *_ in _all_modes(hipk, h, *vec)}
    assert got == {m: want[m] for m, _ in C.RUNS}, got
    h.close()


# ------------------------------------------------------------------------------------------------------------ 5. solves
def _solve(hipk, h, method, b, **kw):
    x = torch.zeros_like(b)
    st = hipk.solve(method, h, b, x, **{"tol": 1e-8, "atol": 0.0, "maxiter": None, **kw})
    return (x.cpu().numpy().tobytes(), st.iterations, st.matvecs, st.info, st.residual_norm, st.recurrence_rs, hipk.last_solve_path(),
            hipk.last_solve_form(), hipk.last_cg_fused_directions())


@pytest.mark.parametrize("method,nx,kw", [("cg", 35, {}), ("cg", 200, {}), ("bicgstab", 200, {}), ("gmres", 200, {"restart": 5, "maxiter": 40})],
                         ids=["cg35_lds", "cg200_mid", "bicgstab200", "gmres200_r5"])
def test_solves_on_an_updated_handle_are_the_fresh_handles(hipk, method, nx, kw):
    crow, col, const = _grid(nx, nx, "c", torch.float64)
    var = _grid(nx, nx, "v", torch.float64, seed=2)[2]
    n = nx * nx
    b = _vectors(n, torch.float64)[0]
    h = hipk.CsrHandle(crow, col, const, (n, n))
    _solve(hipk, h, method, b, **kw)                               # the window plan of the one-launch loop is made here, and kept
    for val in (var, const * 2):
        h.update_values(val)
        got = _solve(hipk, h, method, b, **kw)
        fresh = hipk.CsrHandle(crow, col, val.clone(), (n, n))
        want = _solve(hipk, fresh, method, b, **kw)
        fresh.close()
        print(method, nx, got[1:], flush=True)
        assert got == want, (got[1:], want[1:])
    if nx == 35:
        assert "hipk_cg_solve_lds_kernel" in got[6], got[6]
    if (method, nx) == ("cg", 200):
        assert got[6].startswith("hipk_cg_mid_kernel<"), got[6]
    h.close()


def test_the_fused_cg_launch_engages_after_an_update_to_constant_coefficients_and_not_after_the_reverse(hipk):
    nx = 1025
    crow, col, const = _grid(nx, nx, "c", torch.float64)
    var = _grid(nx, nx, "v", torch.float64, seed=2)[2]
    n = nx * nx
    b = torch.ones(n, dtype=torch.float64, device=DEV)
    kw = {"maxiter": 4, "tol": 0.0}
    h = hipk.CsrHandle(crow, col, var, (n, n))
    for val, kind, fused in ((const, 3, True), (var, 3, False)):
        _update(hipk, h, val, kind)
        got = _solve(hipk, h, "cg", b, **kw)
        fresh = hipk.CsrHandle(crow, col, val.clone(), (n, n))
        want = _solve(hipk, fresh, "cg", b, **kw)
        fresh.close()
        assert got == want, (got[1:], want[1:])
        assert (got[8] > 0) == fused, got[1:]
    h.close()


# ------------------------------------------------------------------------------------------------------------ 6. memory
@pytest.mark.parametrize("kind", ["c", "v"], ids=["pair_coded", "offset_coded"])
def test_an_update_writes_handle_owned_memory_only(hipk, kind):
    crow, col, val = _grid(70, 73, kind, torch.float64, seed=1)
    new = val * 2 if kind == "c" else _grid(70, 73, "v", torch.float64, seed=2)[2]
    n, nnz = 5110, val.numel()
    g = guard_bytes_for(n, 8)
    va, ba, xa = Arena(DEV, nnz * 8, 16, g), Arena(DEV, n * 8, 16, g), Arena(DEV, n * 8, 16, g)
    v, b, x = va.put(new), ba.put(_vectors(n, torch.float64)[0]), xa.view(torch.float64, n)
    x.zero_()
    va.snapshot()
    ba.snapshot()
    h = hipk.CsrHandle(crow, col, val, (n, n))
    _update(hipk, h, v, 2 if kind == "c" else 1)
    torch.cuda.synchronize()
    assert va.unchanged() and all(a.guards_intact() for a in (va, ba, xa)), [a.touched() for a in (va, ba, xa)]
    st = hipk.solve("cg", h, b, x, tol=1e-8, atol=0.0, maxiter=None)
    assert st.info == 0
    assert va.unchanged() and ba.unchanged() and all(a.guards_intact() for a in (va, ba, xa)), [a.touched() for a in (va, ba, xa)]
    fresh = hipk.CsrHandle(crow, col, new.clone(), (n, n))
    xf = torch.zeros(n, dtype=torch.float64, device=DEV)
    hipk.solve("cg", fresh, b.clone(), xf, tol=1e-8, atol=0.0, maxiter=None)
    assert torch.equal(x, xf)
    fresh.close()
    h.close()


# ------------------------------------------------------------------------------------------------------------ 7. errors
def test_error_codes_leave_the_handle_as_it_was(hipk):
    L = hipk.lib()
    crow, col, val = _grid(70, 73, "c", torch.float64)
    new = val * 2
    h = hipk.CsrHandle(crow, col, val, (5110, 5110))
    vec = _vectors(5110, torch.float64)
    before = _all_modes(hipk, h, *vec)
    stream = torch.cuda.current_stream().cuda_stream
    assert L.hipk_csr_update_values(h._h, None, stream) == -1 and b"null" in L.hipk_last_error()           # HIPK_ERR_ARG
    assert L.hipk_csr_update_values(h._h, new.data_ptr() + 8, stream) == -3 and b"aligned" in L.hipk_last_error()   # HIPK_ERR_ALIGN
    assert h.path() == "coded" and _all_modes(hipk, h, *vec) == before
    op = hipk.OpHandle(lambda v: 2.0 * v, 5110, torch.float64, torch.device(DEV))
    assert L.hipk_csr_update_values(op.ptr, new.data_ptr(), stream) == -4 and b"matrix-free" in L.hipk_last_error()  # HIPK_ERR_UNSUPPORTED
    op.close()
    for bad, what in ((new.to(torch.float32), "dtype"), (new.cpu(), "device"), (new[:-1], "nnz")):
        with pytest.raises(ValueError, match=what):
            h.update_values(bad)
    assert _all_modes(hipk, h, *vec) == before
    assert L.hipk_version() == 300
    h.close()


# ------------------------------------------------------------------------------------------------------------ 8. the transpose, gradients
def test_the_transpose_of_an_updated_handle_is_the_new_matrix_transposed(hipk, oracle):
    from pytorch_sparse_solver.utils.matrix_utils import create_convdiff_2d_csr
    A = create_convdiff_2d_csr(31, 29)
    crow, col, val = A.crow_indices().numpy(), A.col_indices().numpy(), A.values().numpy()
    n = 31 * 29
    rows = np.repeat(np.arange(n), np.diff(crow))
    new = val * (1.0 + 0.3 * np.sin(rows + 2.0 * col))
    order = np.argsort(col, kind="stable")                        # A^T: the entries sorted by column, rows ascending within one
    crow_t = np.concatenate([[0], np.cumsum(np.bincount(col, minlength=n))])
    x = np.random.default_rng(8).standard_normal(n)
    h = hipk.CsrHandle(_dev(crow), _dev(col), _dev(val), (n, n))
    old_t = h.transposed()
    h.update_values(_dev(new))
    ht = h.transposed()
    assert ht is not old_t
    y = hipk.spmv(ht, _dev(x)).cpu().numpy()
    want = oracle.spmv(crow_t, rows[order], new[order], x)
    assert y.tobytes() == want.tobytes()
    h.close()


def test_gradients_after_refresh_matrix_are_those_of_a_fresh_cache(hipk):
    """The fresh cache is this process's cache after clear_cache(): every handle, the transposes included, is then built anew from the
    current values, which is what a new process would do; a second process is not started for it."""
    from pytorch_sparse_solver import module_a as MA
    crow, col, val = _grid(17, 13, "c", torch.float64)
    n = 17 * 13
    A0 = torch.sparse_csr_tensor(crow, col, val.clone(), size=(n, n))
    b0, w = _vectors(n, torch.float64)[:2]

    def grads():
        A, b = A0.detach().requires_grad_(), b0.clone().requires_grad_()
        x, info = MA.cg(A, b, tol=1e-10)
        assert info == 0
        (x * w).sum().backward()
        return A.grad.values().cpu().numpy().tobytes(), b.grad.cpu().numpy().tobytes()

    hipk.clear_cache()
    grads()
    h = hipk.handle_for(A0)
    A0.values().mul_(2)
    assert MA.refresh_matrix(A0) is True and hipk.handle_for(A0) is h
    got = grads()
    assert hipk.handle_for(A0) is h
    hipk.clear_cache()
    assert got == grads()
    assert hipk.handle_for(A0) is not h


# ------------------------------------------------------------------------------------------------------------ 9. the cache
def test_refresh_matrix_and_the_cache(hipk):
    from pytorch_sparse_solver.module_a import refresh_matrix
    hipk.clear_cache()
    crow, col, val = _grid(70, 73, "c", torch.float64)
    A = torch.sparse_csr_tensor(crow, col, val.clone(), size=(5110, 5110))
    assert refresh_matrix(A) is False                              # an empty cache
    h = hipk.handle_for(A)
    A.values().mul_(2)
    assert refresh_matrix(A) is True
    assert hipk.CsrHandle.last_update_kind() == 2
    assert hipk.handle_for(A) is h and hipk.cache_info()[0] == 1
    _is_fresh(hipk, h, crow, col, val * 2, path="coded")
    # a tensor of its own on the same index tensors takes the handle over
    var = _grid(70, 73, "v", torch.float64, seed=1)[2]
    B = torch.sparse_csr_tensor(A.crow_indices(), A.col_indices(), var, size=(5110, 5110))
    assert refresh_matrix(B, like=A) is True
    assert hipk.CsrHandle.last_update_kind() == 3
    assert hipk.handle_for(B) is h and hipk.cache_info()[0] == 1
    _is_fresh(hipk, h, crow, col, var, path="offset_coded")
    assert hipk.handle_for(A) is not h and hipk.cache_info()[0] == 2        # A_old builds a handle of its own again
    own = torch.sparse_csr_tensor(crow.clone(), col.clone(), var.clone(), size=(5110, 5110))
    with pytest.raises(ValueError, match="index tensors of its own"):
        refresh_matrix(own, like=B)
    for bad, what in ((B.to(torch.float32), "dtype"), (B.cpu(), "device"), (B.to_dense(), "CSR")):
        with pytest.raises(ValueError, match=what):
            refresh_matrix(bad, like=B)
    assert hipk.handle_for(B) is h
    hipk.clear_cache()
