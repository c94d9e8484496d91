"""The device side of `AggregationMultigridPreconditioner(cycle="W")` against tests/_mg_w_mirror.py and the CPU apply, every
comparison bitwise:

1. hipk_mg_add between seeded guards, both dtypes, at lengths with a ragged 16-byte group and more than one chunk;
2. hipk_mg_tail_apply_w / hipk_mg_gtail_apply_w / hipk_mg_gtail_dense_apply_w: the W launch sequence's and the mirror's bits on the
   last 2 .. 6 levels of a box, a graph and a dense-cut hierarchy and on 1 and 2 levels (W is V there), with a dense level of 512
   rows visited twice; `work` of exactly the reported bytes between guards in the four states of tests/_arena.py, a side stream;
   the error codes, each leaving z and the workspace untouched;
3. the whole apply at tail_rows 0 / 256 / 1024 against the CPU apply of the same hierarchy, and `launches_per_apply` by counting;
4. whole cg / bicgstab / gmres solves against the same solve whose M is a Python callable around the mirror."""
import ctypes

import numpy as np
import pytest
import torch

import _mg_graph_mirror as GM
import _mg_mirror as MM
import _mg_w_mirror as WM
from _arena import Arena, check_memory, guard_bytes_for, run_states
from pytorch_sparse_solver.module_a import AggregationMultigridPreconditioner as MG
from pytorch_sparse_solver.module_a import bicgstab, cg, get_last_stats, gmres
from pytorch_sparse_solver.utils.matrix_utils import create_convdiff_2d_csr, create_poisson_2d_csr, create_variable_diffusion_2d_csr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [np.float64, np.float32]
ARG, ALIGN, UNSUPPORTED, WORKSPACE = -1, -3, -4, -5


def _arena(a):
    ar = Arena(DEV, a.nbytes, 16, guard_bytes_for(a.size, a.itemsize))
    return ar, ar.put(a)


def _np(A):
    A = A.cpu()
    return A.crow_indices().numpy(), A.col_indices().numpy(), A.values().numpy()


def _vardiff(nx, ny, dtype):
    crow, col, val = _np(create_variable_diffusion_2d_csr(nx, ny))
    return crow, col, val.astype(dtype)


# ------------------------------------------------------------------------------------------------------------ 1. hipk_mg_add
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
@pytest.mark.parametrize("n", [1, 3, 4, 2047, 2049, 70001])
def test_mg_add_has_numpys_bits_between_guards(hipk, n, dtype):
    rng = np.random.default_rng([3, n])
    e, e2 = (rng.standard_normal(n).astype(dtype) for _ in range(2))
    e_ar, e_d = _arena(e)
    e2_ar, e2_d = _arena(e2)
    e2_ar.snapshot()
    hipk.mg_add(e2_d, e_d)
    torch.cuda.synchronize()
    check_memory({"e": e_ar, "e2": e2_ar}, {"e2": e2_ar}, f"hipk_mg_add {n}")
    assert MM.same_bits(e_d.cpu().numpy(), e + e2)


def test_mg_add_refuses_bad_arguments(hipk):
    L = hipk.lib()
    v = torch.zeros(64, dtype=torch.float64, device=DEV)
    w = torch.ones(64, dtype=torch.float64, device=DEV)
    assert L.hipk_mg_add(0, w.data_ptr(), v.data_ptr(), 1, None) == ARG
    assert L.hipk_mg_add(64, None, v.data_ptr(), 1, None) == ARG and L.hipk_mg_add(64, v.data_ptr(), v.data_ptr(), 1, None) == ARG
    assert L.hipk_mg_add(64, w.data_ptr() + 8, v.data_ptr(), 1, None) == ALIGN
    assert L.hipk_mg_add(64, w.data_ptr(), v.data_ptr(), 7, None) == UNSUPPORTED
    torch.cuda.synchronize()
    assert not bool(v.any())


# ------------------------------------------------------------------------------------------------------------ 2. the W tails
def _ladder(dtype):
    """512 x 4 points, row 4 i + j: couplings -1, -0.1, -1 along j and -0.01 along i.  One matching pass pairs (j0, j1) and (j2, j3)
    of every i, the next one the two pairs: 2048 -> 1024 -> 512 rows exactly."""
    nx, ny, w = 512, 4, (1.0, 0.1, 1.0, 0.0)          # w[j]: between j and j + 1 (the last one is never stored)
    crow, col, val = [0], [], []
    for i in range(nx):
        for j in range(ny):
            ent = [((i - 1) * ny + j, -0.01)] * (i > 0) + [(i * ny + j - 1, -w[j - 1])] * (j > 0) + [(i * ny + j, None)] + \
                [(i * ny + j + 1, -w[j])] * (j < ny - 1) + [((i + 1) * ny + j, -0.01)] * (i < nx - 1)
            d = 0.05 - sum(v for _, v in ent if v is not None)
            col += [c for c, _ in ent]
            val += [d if v is None else v for _, v in ent]
            crow.append(len(col))
    return np.array(crow, dtype=np.int64), np.array(col, dtype=np.int64), np.array(val, dtype=dtype)


# kind -> (the matrix of the whole hierarchy, the constructor, its level sizes, the wrapper of its W tail)
HIERARCHIES = {
    "box40x33": (lambda dt: MM.grid_matrix((40, 33), dtype=dt), lambda A, dims, **kw: MG(A, dims, **kw), "mg_tail_apply_w"),
    "graph64x64": (lambda dt: GM.shuffled(*_vardiff(64, 64, dt)), lambda A, dims, **kw: MG.from_graph(A, **kw), "mg_gtail_apply_w"),
    "dense48x48": (lambda dt: GM.stencil5(48, 48, dtype=dt), lambda A, dims, **kw: MG.from_graph(A, coarse_rows=64, **kw), "mg_gtail_dense_apply_w"),
    "dense512": (_ladder, lambda A, dims, **kw: MG.from_graph(A, passes=1, coarse_rows=512, **kw), "mg_gtail_dense_apply_w"),
}
_parents = {}


def _parent(kind, dtype):
    """The whole hierarchy of `kind`, built once per dtype on the device and never applied."""
    key = (kind, np.dtype(dtype).name)
    if key not in _parents:
        make, build, _ = HIERARCHIES[kind]
        A = MM.csr_tensor(*make(dtype), device=DEV)
        _parents[key] = build(A, (40, 33), normalize=False)
    return _parents[key]


def _tail_cases():
    for kind, most in (("box40x33", 6), ("graph64x64", 6), ("dense48x48", 5)):
        for k in range(1, most + 1):
            yield kind, k, DTYPES[k % 2], 1 + k % 2
    yield "graph64x64", 10, np.float64, 1          # from level 1 down: the last level 256 times in one launch
    yield "graph64x64", 10, np.float32, 2
    yield "dense48x48", 4, np.float32, 2
    yield "dense512", 3, np.float64, 1             # the 512-row dense step, twice
    yield "dense512", 3, np.float32, 2
    yield "dense512", 2, np.float64, 2
    yield "dense512", 1, np.float32, 1


@pytest.mark.parametrize("kind, k, dtype, degree", list(_tail_cases()), ids=lambda v: getattr(v, "__name__", str(v)))
def test_w_tail_equals_the_launch_sequence_and_the_mirror_in_every_workspace_state(hipk, oracle, kind, k, dtype, degree):
    """The last k levels of the hierarchy as a hierarchy of their own: built from the parent's level matrix, the same coarsening
    continues it."""
    parent = _parent(kind, dtype)
    lev = parent.levels[len(parent.levels) - k]
    _, build, wrapper = HIERARCHIES[kind]
    A = lev.csr
    Mt = build(A, lev.dims, degree=degree, normalize=False, tail_rows=4096, cycle="W")
    Ms = build(A, lev.dims, degree=degree, normalize=False, tail_rows=0, cycle="W")
    sizes = [v.n for v in parent.levels[len(parent.levels) - k:]]
    assert [v.n for v in Mt.levels] == [v.n for v in Ms.levels] == sizes, (sizes, [v.n for v in Mt.levels])
    assert Mt.tail_from == 0 and Mt.launches_per_apply == 1 and Ms.tail_from is None
    n, omega, scale = A.shape[0], 1.8, 0.37
    r = np.random.default_rng([5, n, k]).standard_normal(n).astype(dtype)
    Ms.scale = scale
    ref = WM.apply(oracle, Ms, r)
    zs = Ms(torch.from_numpy(r).to(DEV)).cpu().numpy()
    assert MM.same_bits(zs, ref), f"launch sequence: {np.count_nonzero(MM.bits(zs) != MM.bits(ref))} of {n} entries differ from the mirror"
    if k <= 2:
        assert MM.same_bits(ref, WM.apply(oracle, Ms, r, cycle="V")), "W on one or two levels is V"

    Mt._dev_state()                                      # builds the descriptors
    tail = Mt._tail
    assert tail.cycle == "W" and tail.nlev == k
    bytes_w = getattr(hipk.lib(), {"mg_tail_apply_w": "hipk_mg_tail_work_bytes_w", "mg_gtail_apply_w": "hipk_mg_gtail_work_bytes_w",
                                   "mg_gtail_dense_apply_w": "hipk_mg_gtail_dense_work_bytes_w"}[wrapper])
    el = 6 * sum((s + 3) & ~3 for s in sizes) * r.itemsize
    assert tail.work_bytes == bytes_w(tail.host, k, 1 if dtype == np.float64 else 0) == (el + 255) & ~255
    work = Arena(DEV, tail.work_bytes, 256, guard_bytes_for(n, r.itemsize))
    r_ar, r_d = _arena(r)
    z_ar, z_d = _arena(np.zeros_like(r))
    side = torch.cuda.Stream(device=DEV)

    def run(i):
        z_d.fill_(float("nan"))
        torch.cuda.synchronize()
        with torch.cuda.stream(side if i == 1 else torch.cuda.current_stream(DEV)):
            getattr(hipk, wrapper)(tail, omega, scale, r_d, z_d, work=work.payload)
        torch.cuda.synchronize()
        return {"z": z_d.cpu().numpy().tobytes()}

    res = run_states(work, {"z": z_ar, "r": r_ar}, {"r": r_ar}, run, label=f"{wrapper} {kind} {k} levels")
    zt = np.frombuffer(res[0]["z"], dtype=dtype)
    assert MM.same_bits(zt, ref), f"W tail: {np.count_nonzero(MM.bits(zt) != MM.bits(ref))} of {n} entries differ from the mirror"


def test_v_work_bytes_are_unchanged_and_the_w_slab_is_six_vectors(hipk):
    parent = _parent("graph64x64", np.float64)
    M = MG.from_graph(parent.levels[2].csr, normalize=False, tail_rows=4096)
    W = MG.from_graph(parent.levels[2].csr, normalize=False, tail_rows=4096, cycle="W")
    M._dev_state(), W._dev_state()
    el = sum((lev.n + 3) & ~3 for lev in M.levels) * 8
    assert M._tail.work_bytes == (5 * el + 255) & ~255 and W._tail.work_bytes == (6 * el + 255) & ~255
    with pytest.raises(AssertionError, match="built for cycle"):
        hipk.mg_gtail_apply_w(M._tail, 1.8, 1.0, torch.ones(M.shape[0], dtype=torch.float64, device=DEV),
                              torch.zeros(M.shape[0], dtype=torch.float64, device=DEV))


def _extended(hipk, struct, tail, count):
    host = (struct * count)()
    ctypes.memmove(host, tail.host, ctypes.sizeof(tail.host))
    for j in range(tail.nlev, count):                    # further levels: copies of the last one
        ctypes.memmove(ctypes.byref(host[j]), ctypes.byref(tail.host[tail.nlev - 1]), ctypes.sizeof(struct))
    return host


@pytest.mark.parametrize("kind", ["box40x33", "graph64x64", "dense48x48"])
def test_w_tail_error_codes_write_nothing(hipk, kind):
    parent = _parent(kind, np.float64)
    _, build, wrapper = HIERARCHIES[kind]
    lev = parent.levels[len(parent.levels) - 4]
    M = build(lev.csr, lev.dims, normalize=False, tail_rows=4096, cycle="W")
    M._dev_state()
    tail, L = M._tail, hipk.lib()
    struct = hipk.MgLevel if kind == "box40x33" else hipk.MgGLevel
    r = torch.ones(M.shape[0], dtype=torch.float64, device=DEV)
    z = torch.full_like(r, 7.0)
    work = torch.full((tail.work_bytes,), 0x5A, dtype=torch.uint8, device=DEV)
    last = () if getattr(tail, "cinv", None) is None else (tail.cinv.data_ptr(), tail.ld)
    entry = getattr(L, "hipk_" + wrapper)

    def call(host=None, nlev=None, degree=1, rp=None, zp=None, wp=None, wb=None, dtype=1, blob=True):
        return entry(tail.host if host is None else host, tail.blob.data_ptr() if blob else None, tail.nlev if nlev is None else nlev, degree,
                     1.8, 1.0, *last, r.data_ptr() if rp is None else rp, z.data_ptr() if zp is None else zp, dtype,
                     work.data_ptr() if wp is None else wp, tail.work_bytes if wb is None else wb, None)

    def edited(level=0, **kw):
        host = _extended(hipk, struct, tail, tail.nlev)
        for name, v in kw.items():
            setattr(host[level], name, v)
        return host

    assert call(host=_extended(hipk, struct, tail, 13), nlev=13) == UNSUPPORTED      # 13 tail levels
    assert call(host=edited(max_row=33)) == UNSUPPORTED                              # a 33-entry row
    assert call(dtype=5) == UNSUPPORTED
    assert call(host=edited(dinv=None)) == ARG and call(host=edited(level=1, val=None)) == ARG      # null pointers
    assert call(host=None, nlev=0) == ARG and call(degree=0) == ARG and call(degree=33) == ARG
    assert call(rp=0) == ARG and call(zp=0) == ARG and call(wp=0) == ARG and call(blob=False) == ARG and call(zp=r.data_ptr()) == ARG
    assert call(rp=r.data_ptr() + 8) == ALIGN and call(wp=work.data_ptr() + 16) == ALIGN
    assert call(wb=tail.work_bytes - 1) == WORKSPACE
    bytes_w = getattr(L, "hipk_" + wrapper.replace("_apply_w", "_work_bytes_w"))
    assert bytes_w(_extended(hipk, struct, tail, 13), 13, 1) == 0 and bytes_w(tail.host, 0, 1) == 0
    torch.cuda.synchronize()
    assert bool((z == 7.0).all()) and bool((work == 0x5A).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool((z == 7.0).any())


# ------------------------------------------------------------------------------------------------------------ 3. the whole apply
KINDS = {"grid": lambda A, grid, **kw: MG(A, grid, **kw), "graph": lambda A, grid, **kw: MG.from_graph(A, **kw),
         "dense": lambda A, grid, **kw: MG.from_graph(A, coarse_rows=64, **kw)}


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
@pytest.mark.parametrize("grid", [(96, 96), (257, 129)], ids=["96x96", "257x129"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_whole_w_apply_is_the_cpu_apply_at_every_tail_size(hipk, kind, grid, dtype):
    A = MM.csr_tensor(*_vardiff(*grid, dtype))
    # two matching passes make 16 levels of 257 x 129 -- level 14 would be visited 2^14 times, 19 s on a CPU --, three make 11;
    # the run of more than 12 small levels that falls back to launches is test_thirteen_small_levels_run_as_launches
    kw = {"passes": 3} if (kind, grid) == ("graph", (257, 129)) else {}
    Mc = KINDS[kind](A, grid, normalize=False, cycle="W", **kw)
    Mc.scale = 0.37
    r = torch.from_numpy(np.random.default_rng(17).standard_normal(A.shape[0]).astype(dtype))
    ref = Mc(r).numpy()
    Ad, rd = A.to(DEV), r.to(DEV)
    sizes = [lev.n for lev in Mc.levels]
    for tail_rows in (0, 256, 1024):
        M = KINDS[kind](Ad, grid, normalize=False, tail_rows=tail_rows, cycle="W", **kw)
        M.scale = 0.37
        assert [lev.n for lev in M.levels] == sizes and M.launches_per_apply == WM.launches(M)
        first = next((l for l, n in enumerate(sizes) if n <= tail_rows), None)
        fits = first is not None and len(sizes) - first <= 12 and all(lev.max_row <= 32 for lev in M.levels[first:len(sizes) - M.dense]) and \
            (not M.dense or sizes[-1] <= 512)
        assert M.tail_from == (first if fits else None)
        z = M(rd).cpu().numpy()
        assert MM.same_bits(z, ref), f"tail_rows {tail_rows}: {np.count_nonzero(MM.bits(z) != MM.bits(ref))} entries differ from the CPU apply"
    assert MM.same_bits(M(rd).cpu().numpy(), ref), "the second apply differs from the first"


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
def test_thirteen_small_levels_run_as_launches(hipk, oracle, dtype):
    """One level more than the W tails take: `tail_rows=4096` selects every level, the tail is refused and all 13 levels are
    launches (level 11 is visited 2^11 times), bitwise the CPU apply and the mirror.  A star of 12 leaves, one pair per level."""
    crow, col, val = GM.star(12, dtype=dtype)
    Mc = MG.from_graph(MM.csr_tensor(crow, col, val), passes=1, normalize=False, tail_rows=4096, cycle="W")
    M = MG.from_graph(MM.csr_tensor(crow, col, val, device=DEV), passes=1, normalize=False, tail_rows=4096, cycle="W")
    assert [lev.n for lev in M.levels] == list(range(13, 0, -1)) and M.tail_from is None
    assert MG.from_graph(MM.csr_tensor(crow, col, val, device=DEV), passes=1, normalize=False, tail_rows=4096).tail_from == 0
    assert M.launches_per_apply == WM.launches(M) == 4095 * 9 + 4094 + 2048
    r = np.random.default_rng(13).standard_normal(13).astype(dtype)
    z = M(torch.from_numpy(r).to(DEV)).cpu().numpy()
    assert MM.same_bits(z, Mc(torch.from_numpy(r)).numpy()) and MM.same_bits(z, WM.apply(oracle, M, r))


@pytest.mark.parametrize("kind, tail_rows", [("grid", 0), ("grid", 256), ("graph", 256), ("dense", 0), ("dense", 1024), ("dense", 4096)])
def test_launches_per_apply_is_the_count_of_the_wrappers_calls(hipk, monkeypatch, kind, tail_rows):
    degree, grid = 2, (96, 96)
    M = KINDS[kind](create_variable_diffusion_2d_csr(*grid, device=DEV), grid, degree=degree, normalize=False, tail_rows=tail_rows, cycle="W")
    r = torch.ones(M.shape[0], dtype=torch.float64, device=DEV)
    M(r)                                                 # builds the device state
    count = {"launches": 0, "names": {}}
    weight = dict.fromkeys(["spmv_residual", "mg_add", "mg_correct", "mg_diag", "mg_dense_apply", "mg_restrict", "mg_prolong_add",
                            "mg_restrict_agg", "mg_prolong_add_agg", "mg_tail_apply", "mg_gtail_apply", "mg_gtail_dense_apply",
                            "mg_tail_apply_w", "mg_gtail_apply_w", "mg_gtail_dense_apply_w"], 1)
    weight["cheb_apply"] = degree + 1
    for name, w in weight.items():
        def counted(*a, _f=getattr(hipk, name), _w=w, _n=name, **kw):
            count["launches"] += _w
            count["names"][_n] = count["names"].get(_n, 0) + 1
            return _f(*a, **kw)
        monkeypatch.setattr(hipk, name, counted)
    M(r)
    torch.cuda.synchronize()
    print(kind, tail_rows, [lev.n for lev in M.levels], M.tail_from, count)
    assert count["launches"] == M.launches_per_apply == WM.launches(M)
    assert not set(count["names"]) & {"mg_tail_apply", "mg_gtail_apply", "mg_gtail_dense_apply"}, "a W object ran a V tail"
    T, L = M.tail_from, len(M.levels) - 1
    if T is not None:
        tails = count["names"].get({"grid": "mg_tail_apply_w", "graph": "mg_gtail_apply_w", "dense": "mg_gtail_dense_apply_w"}[kind], 0)
        assert tails == (1 if T == 0 else 2 ** T if T < L else 2 ** (T - 1))
    assert count["names"].get("mg_add", 0) == max(2 ** (L if T is None else min(T + 1, L)) // 2 - 1, 0)


# ------------------------------------------------------------------------------------------------------------ 4. whole solves
def _mirror_callable(oracle, M):
    mirror = WM.Mirror(oracle, M)

    def fn(v):
        return torch.from_numpy(mirror(v.cpu().numpy())).to(v.device)
    return fn


def _same_solve(solver, A, b, M, fn, method, **kw):
    x, info = solver(A, b, M=M, **kw)
    st = get_last_stats()
    xr, infor = solver(A, b, M=fn, **kw)
    sr = get_last_stats()
    assert st.method == sr.method == method, (st.method, sr.method)
    assert info == infor and st.iterations == sr.iterations and st.matvecs == sr.matvecs
    assert (st.b_norm, st.residual_norm, st.x_norm, st.threshold) == (sr.b_norm, sr.residual_norm, sr.x_norm, sr.threshold)
    assert MM.same_bits(x.cpu().numpy(), xr.cpu().numpy())
    return x, info, st


@pytest.mark.parametrize("kind", list(KINDS))
def test_cg_solves_with_the_w_cycle_equal_the_mirror_driven_solves(hipk, oracle, kind):
    grid = (128, 128)
    A = create_poisson_2d_csr(*grid, device=DEV)
    b = torch.ones(A.shape[0], dtype=torch.float64, device=DEV)
    kw = {"passes": 3} if kind == "graph" else {}          # 9 levels instead of 12: the mirror walks them on the CPU
    M = KINDS[kind](A, grid, cycle="W", **kw)
    x, info, st = _same_solve(cg, A, b, M, _mirror_callable(oracle, M), "cg_callable_M", tol=1e-6)
    relres = float(torch.linalg.vector_norm(b - A @ x) / torch.linalg.vector_norm(b))
    V = KINDS[kind](A, grid, **kw)
    cg(A, b, M=V, tol=1e-6)
    print(f"{kind} 128^2 Poisson: W {st.iterations} iterations, V {get_last_stats().iterations}, relative residual {relres:.3e}")
    assert info == 0 and relres <= 1e-6 and st.iterations < get_last_stats().iterations


def test_bicgstab_and_gmres_run_the_w_cycle_as_a_deterministic_left_preconditioner(hipk, oracle):
    grid = (128, 128)
    A = create_convdiff_2d_csr(*grid, device=DEV)
    b = torch.ones(A.shape[0], dtype=torch.float64, device=DEV)
    M = MG.from_graph(A, coarse_rows=64, cycle="W")
    fn = _mirror_callable(oracle, M)
    _same_solve(bicgstab, A, b, M, fn, "bicgstab_callable_M", tol=1e-6)
    _same_solve(gmres, A, b, M, fn, "gmres_callable_M", tol=1e-6, restart=20)
