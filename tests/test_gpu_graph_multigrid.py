"""The device side of AggregationMultigridPreconditioner.from_graph against tests/_mg_graph_mirror.py, every comparison bitwise:

1. hipk_mg_restrict_agg / hipk_mg_prolong_add_agg between seeded guards, both dtypes: synthetic member lists with aggregates of
   1 .. 9 members, members adjacent and members far more than a chunk apart, from one row to 2048 * 2048 + 5 (a chunk size above 2048,
   ragged last groups on both sides), the level-0 maps of real hierarchies, and the error codes;
2. hipk_mg_gtail_apply: the launch sequence's and the mirror's bits, degrees 1 and 3, both dtypes, a last level of two unknowns; the
   workspace in the four states of tests/_arena.py with `work` of exactly hipk_mg_gtail_work_bytes, a side stream, the refusals;
3. the whole apply at tail_rows 0 / 64 / 1024 / 4096, the device-built hierarchy against the CPU one, `launches_per_apply`;
4. whole cg / bicgstab / gmres solves against the same solve whose M is a Python callable around the mirror."""
import ctypes

import numpy as np
import pytest
import torch

import _mg_graph_mirror as GM
import _mg_mirror as MM
from _arena import Arena, check_memory, guard_bytes_for, run_states
from pytorch_sparse_solver.module_a import AggregationMultigridPreconditioner as MG
from pytorch_sparse_solver.module_a import bicgstab, cg, get_last_stats, gmres
from pytorch_sparse_solver.utils.matrix_utils import create_convdiff_2d_csr, create_poisson_2d_csr, create_variable_diffusion_2d_csr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [np.float64, np.float32]
SIZES = [(1, 1), (5, 2), (4099, 1031), (70_001, 21_877), (2048 * 2048 + 5, 1_300_003)]
LOOP_MAX = 100_000          # up to here the reference is the mirror's Python loop, beyond it the numpy form of the same sums


def _np(A):
    A = A.cpu()
    return A.crow_indices().numpy(), A.col_indices().numpy(), A.values().numpy()


def _arena(a):
    """A vector between guards, exactly its bytes of payload."""
    ar = Arena(DEV, a.nbytes, 16, guard_bytes_for(a.size, a.itemsize))
    return ar, ar.put(a)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------------------------------------ 1. transfer kernels
def _check_transfers(hipk, agg, aptr, amem, dtype, label):
    n, nc = len(agg), len(aptr) - 1
    rng = np.random.default_rng([3, n, nc])
    t, e, z0 = (rng.standard_normal(k).astype(dtype) for k in (n, nc, n))
    if n <= LOOP_MAX:
        mem = GM.member_lists(agg, nc)
        assert [i for m in mem for i in m] == amem.tolist() and np.array_equal(np.cumsum([0] + [len(m) for m in mem]), aptr)
        rc_ref, z_ref = GM.restrict(t, mem), GM.prolong_add(z0, e, 1.8, agg)
        assert GM.same_bits(rc_ref, GM.restrict_np(t, aptr, amem)) and GM.same_bits(z_ref, GM.prolong_add_np(z0, e, 1.8, agg))
    else:
        rc_ref, z_ref = GM.restrict_np(t, aptr, amem), GM.prolong_add_np(z0, e, 1.8, agg)
    agg_d, aptr_d, amem_d = _dev(agg), _dev(aptr), _dev(amem)
    t_ar, t_d = _arena(t)
    rc_ar, rc_d = _arena(rng.standard_normal(nc).astype(dtype))
    t_ar.snapshot()
    hipk.mg_restrict_agg(aptr_d, amem_d, t_d, rc_d)
    torch.cuda.synchronize()
    check_memory({"rc": rc_ar, "t": t_ar}, {"t": t_ar}, f"hipk_mg_restrict_agg {label}")
    got = rc_d.cpu().numpy()
    assert GM.same_bits(got, rc_ref), f"hipk_mg_restrict_agg {label}: {np.count_nonzero(GM.bits(got) != GM.bits(rc_ref))} of {nc} differ"
    e_ar, e_d = _arena(e)
    z_ar, z_d = _arena(z0)
    e_ar.snapshot()
    hipk.mg_prolong_add_agg(agg_d, 1.8, e_d, z_d)
    torch.cuda.synchronize()
    check_memory({"z": z_ar, "e": e_ar}, {"e": e_ar}, f"hipk_mg_prolong_add_agg {label}")
    got = z_d.cpu().numpy()
    assert GM.same_bits(got, z_ref), f"hipk_mg_prolong_add_agg {label}: {np.count_nonzero(GM.bits(got) != GM.bits(z_ref))} of {n} differ"
    assert torch.equal(agg_d.cpu(), torch.from_numpy(agg)) and torch.equal(aptr_d.cpu(), torch.from_numpy(aptr)) and \
        torch.equal(amem_d.cpu(), torch.from_numpy(amem)), "an index array was modified"


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
@pytest.mark.parametrize("spread", [False, True], ids=["adjacent", "apart"])
@pytest.mark.parametrize("n, nc", SIZES, ids=lambda v: str(v))
def test_transfer_kernels_have_the_mirrors_bits_between_guards(hipk, n, nc, spread, dtype):
    agg, aptr, amem = GM.synthetic_aggregates(n, nc, spread)
    sizes = np.diff(aptr)
    assert sizes.min() >= 1 and sizes.max() <= 9 and (nc < 1000 or len(np.unique(sizes)) == 9)
    if nc > 20000:              # the distance between consecutive members of an aggregate, against the chunk (2048; 8192 above 4 M rows)
        gaps = np.diff(amem.astype(np.int64))[np.diff(np.repeat(np.arange(nc), sizes)) == 0]
        assert (np.median(gaps) > (8192 if n > 4_000_000 else 2048)) if spread else bool(np.all(gaps == 1))
    _check_transfers(hipk, agg, aptr, amem, dtype, f"n = {n}, nc = {nc}, {'apart' if spread else 'adjacent'}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
@pytest.mark.parametrize("name", ["poisson37x29", "vardiff64x64", "seven_point12x11x10"])
def test_transfer_kernels_on_the_level_0_map_of_a_real_hierarchy(hipk, name, dtype):
    M = _hierarchy(name, np.float64, 1, "cpu")
    agg = M.levels[0].agg.numpy().astype(np.int32)
    aptr, amem = GM.csr_members(agg, M.levels[1].n)
    _check_transfers(hipk, agg, aptr, amem, dtype, name)


def test_transfer_kernels_refuse_bad_arguments(hipk):
    L = hipk.lib()
    v = torch.zeros(64, dtype=torch.float64, device=DEV)
    w = torch.zeros(64, dtype=torch.float64, device=DEV)
    agg, aptr, amem = (_dev(a) for a in GM.synthetic_aggregates(64, 16, False))
    p = lambda x: x.data_ptr()
    ARG, ALIGN, UNSUPPORTED = -1, -3, -4
    assert L.hipk_mg_restrict_agg(64, 0, p(aptr), p(amem), p(v), p(w), 1, None) == ARG
    assert L.hipk_mg_restrict_agg(16, 64, p(aptr), p(amem), p(v), p(w), 1, None) == ARG           # nc > n
    assert L.hipk_mg_restrict_agg(2 ** 31, 16, p(aptr), p(amem), p(v), p(w), 1, None) == ARG
    assert L.hipk_mg_restrict_agg(64, 16, None, p(amem), p(v), p(w), 1, None) == ARG
    assert L.hipk_mg_restrict_agg(64, 16, p(aptr), p(amem), p(v), p(v), 1, None) == ARG
    assert L.hipk_mg_restrict_agg(64, 16, p(aptr), p(amem), p(v) + 8, p(w), 1, None) == ALIGN
    assert L.hipk_mg_restrict_agg(64, 16, p(aptr), p(amem) + 4, p(v), p(w), 1, None) == ALIGN
    assert L.hipk_mg_restrict_agg(64, 16, p(aptr), p(amem), p(v), p(w), 7, None) == UNSUPPORTED
    assert L.hipk_mg_prolong_add_agg(64, 16, p(agg), 1.8, None, p(w), 1, None) == ARG
    assert L.hipk_mg_prolong_add_agg(0, 0, p(agg), 1.8, p(v), p(w), 1, None) == ARG
    assert L.hipk_mg_prolong_add_agg(64, 16, p(agg), 1.8, p(w), p(w), 1, None) == ARG
    assert L.hipk_mg_prolong_add_agg(64, 16, p(agg) + 4, 1.8, p(v), p(w), 1, None) == ALIGN
    assert L.hipk_mg_prolong_add_agg(64, 16, p(agg), 1.8, p(v), p(w), 7, None) == UNSUPPORTED
    torch.cuda.synchronize()
    assert not bool(v.any()) and not bool(w.any())
    with pytest.raises(AssertionError, match="aptr"):
        hipk.mg_restrict_agg(aptr[:-1], amem, v, w[:16])
    with pytest.raises(AssertionError, match="agg"):
        hipk.mg_prolong_add_agg(agg.to(torch.int64), 1.8, v[:16], w)


# ------------------------------------------------------------------------------------------------------------ 2. the tail kernel
def _arrays(name, dtype):
    if name == "poisson37x29":
        arrs = _np(create_poisson_2d_csr(37, 29))
    elif name == "vardiff64x64":
        arrs = _np(create_variable_diffusion_2d_csr(64, 64))
    elif name == "seven_point12x11x10":
        arrs = MM.grid_matrix((12, 11, 10))
    elif name == "two_blocks":
        arrs = GM.block_diagonal(_np(create_poisson_2d_csr(19, 14)), MM.grid_matrix((23, 9), seed=2))
    elif name == "vardiff130x70":
        arrs = _np(create_variable_diffusion_2d_csr(130, 70))
    elif name == "vardiff130x70_shuffled":
        arrs = GM.shuffled(*_np(create_variable_diffusion_2d_csr(130, 70)), seed=1)
    else:
        raise KeyError(name)
    return arrs[0], arrs[1], arrs[2].astype(dtype)


_built = {}


def _hierarchy(name, dtype, degree, device, tail_rows=0):
    """One object per (matrix, dtype, degree, device, tail_rows), shared by the tests of this file (an apply does not change it)."""
    key = (name, np.dtype(dtype).name, degree, device, tail_rows)
    if key not in _built:
        _built[key] = MG.from_graph(MM.csr_tensor(*_arrays(name, dtype), device=device), degree=degree, tail_rows=tail_rows)
    return _built[key]


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
@pytest.mark.parametrize("degree", [1, 3])
@pytest.mark.parametrize("name", ["poisson37x29", "vardiff64x64", "seven_point12x11x10", "two_blocks"])
def test_tail_kernel_equals_the_launch_sequence_and_the_mirror(hipk, oracle, name, degree, dtype):
    Mt, Ms = _hierarchy(name, dtype, degree, DEV, 4096), _hierarchy(name, dtype, degree, DEV, 0)
    assert Mt.tail_from == 0 and Ms.tail_from is None and Mt.launches_per_apply == 1
    assert Ms.launches_per_apply == (len(Ms.levels) - 1) * (2 * degree + 7) + 1
    assert Mt.levels[-1].n == (2 if name == "two_blocks" else 1)
    assert Mt.scale == Ms.scale != 1.0
    n = Mt.shape[0]
    r = np.random.default_rng([5, n]).standard_normal(n).astype(dtype)
    rd = torch.from_numpy(r).to(DEV)
    zt, zs = Mt(rd).cpu().numpy(), Ms(rd).cpu().numpy()
    assert torch.equal(rd.cpu(), torch.from_numpy(r))
    ref = GM.apply(oracle, Ms, r)
    assert GM.same_bits(zs, ref), f"launch sequence: {np.count_nonzero(GM.bits(zs) != GM.bits(ref))} of {n} entries differ from the mirror"
    assert GM.same_bits(zt, ref), f"tail kernel: {np.count_nonzero(GM.bits(zt) != GM.bits(ref))} of {n} entries differ from the mirror"


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
def test_tail_kernel_workspace_states_side_stream_and_guards(hipk, oracle, dtype):
    M = _hierarchy("vardiff64x64", dtype, 3, DEV, 4096)
    n = M.shape[0]
    r = np.random.default_rng(8).standard_normal(n).astype(dtype)
    ref = GM.apply(oracle, M, r)
    M(torch.from_numpy(r).to(DEV))                       # builds the descriptors
    tail = M._tail
    assert isinstance(tail, hipk.MgGTail) and tail.nlev == len(M.levels)
    assert tail.work_bytes == hipk.lib().hipk_mg_gtail_work_bytes(tail.host, tail.nlev, 1 if dtype == np.float64 else 0) > 0
    work = Arena(DEV, tail.work_bytes, 256, guard_bytes_for(n, r.itemsize))
    r_ar, r_d = _arena(r)
    z_ar, z_d = _arena(np.zeros_like(r))
    side = torch.cuda.Stream(device=DEV)

    def run(i):
        z_d.fill_(float("nan"))
        torch.cuda.synchronize()
        with torch.cuda.stream(side if i % 2 else torch.cuda.current_stream(DEV)):
            hipk.mg_gtail_apply(tail, M.omega, M.scale, r_d, z_d, work=work.payload)
        torch.cuda.synchronize()
        return {"z": z_d.cpu().numpy().tobytes()}

    res = run_states(work, {"z": z_ar, "r": r_ar}, {"r": r_ar}, run, label="hipk_mg_gtail_apply vardiff64x64")
    assert res[0]["z"] == ref.tobytes()


def test_tail_kernel_error_codes_write_nothing(hipk):
    M = _hierarchy("poisson37x29", np.float64, 1, DEV, 4096)
    r = torch.ones(M.shape[0], dtype=torch.float64, device=DEV)
    M(r)
    tail, L = M._tail, hipk.lib()
    z = torch.full_like(r, 7.0)
    work = torch.full((tail.work_bytes,), 0x5A, dtype=torch.uint8, device=DEV)

    def call(host=None, nlev=None, degree=1, rp=None, zp=None, wp=None, wb=None, dtype=1):
        return L.hipk_mg_gtail_apply(tail.host if host is None else host, tail.blob.data_ptr(), tail.nlev if nlev is None else nlev, degree,
                                     1.8, 1.0, r.data_ptr() if rp is None else rp, z.data_ptr() if zp is None else zp, dtype,
                                     work.data_ptr() if wp is None else wp, tail.work_bytes if wb is None else wb, None)

    def edited(level=0, count=None, **kw):
        host = (hipk.MgGLevel * (count or tail.nlev))()
        ctypes.memmove(host, tail.host, ctypes.sizeof(tail.host))
        for j in range(tail.nlev, len(host)):            # further levels: copies of the last one (one unknown)
            ctypes.memmove(ctypes.byref(host[j]), ctypes.byref(tail.host[tail.nlev - 1]), ctypes.sizeof(hipk.MgGLevel))
        for k, v in kw.items():
            setattr(host[level], k, v)
        return host

    ARG, ALIGN, UNSUPPORTED, WORKSPACE = -1, -3, -4, -5
    assert call(host=edited(max_row=33)) == UNSUPPORTED               # a level with a 33-entry row
    assert call(host=edited(level=1, max_row=33)) == UNSUPPORTED
    assert call(host=edited(n=4097)) == UNSUPPORTED                   # a 4097-row level
    assert call(host=edited(count=33), nlev=33) == UNSUPPORTED        # 33 levels
    assert L.hipk_mg_gtail_work_bytes(edited(count=33), 33, 1) == 0 and L.hipk_mg_gtail_work_bytes(tail.host, 0, 1) == 0
    assert call(dtype=5) == UNSUPPORTED
    assert call(degree=0) == ARG and call(degree=33) == ARG
    assert call(nlev=0) == ARG
    assert call(host=edited(n=0)) == ARG
    assert call(host=edited(level=1, n=2000)) == ARG                  # more unknowns than the level above
    assert call(host=edited(aptr=None)) == ARG and call(host=edited(level=2, dinv=None)) == ARG
    assert call(zp=r.data_ptr()) == ARG
    assert call(rp=r.data_ptr() + 8) == ALIGN and call(wp=work.data_ptr() + 16) == ALIGN
    assert call(wb=tail.work_bytes - 1) == WORKSPACE
    torch.cuda.synchronize()
    assert bool((z == 7.0).all()) and bool((work == 0x5A).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool((z == 7.0).any())


def test_rows_beyond_the_envelope_stay_on_launches(hipk, oracle):
    crow, col, val = MM.grid_matrix((12, 12), radius=3, full_box=True)
    assert np.diff(crow).max() == 49
    M = MG.from_graph(MM.csr_tensor(crow, col, val, device=DEV), tail_rows=4096)
    assert M.tail_from is None and M.launches_per_apply == (len(M.levels) - 1) * 9 + 1
    r = np.random.default_rng(2).standard_normal(144)
    assert GM.same_bits(M(torch.from_numpy(r).to(DEV)).cpu().numpy(), GM.apply(oracle, M, r))


# ------------------------------------------------------------------------------------------------------------ 3. the whole apply
@pytest.mark.parametrize("name", ["vardiff130x70", "vardiff130x70_shuffled"])
def test_whole_apply_is_the_mirror_at_every_tail_size(hipk, oracle, name):
    A = MM.csr_tensor(*_arrays(name, np.float64), device=DEV)
    r = np.random.default_rng(17).standard_normal(A.shape[0])
    rd = torch.from_numpy(r).to(DEV)
    ref = scale = sizes = None
    for tail_rows in (0, 64, 1024, 4096):
        M = MG.from_graph(A, degree=2, tail_rows=tail_rows)
        if ref is None:
            ref, scale, sizes = GM.apply(oracle, M, r), M.scale, [lev.n for lev in M.levels]
            assert sizes[0] == 9100 and sizes[1] > 1024 and sizes[-1] == 1
        assert [lev.n for lev in M.levels] == sizes and M.scale == scale
        tail_from = next((l for l, n in enumerate(sizes) if n <= tail_rows), None)
        assert M.tail_from == tail_from
        assert M.launches_per_apply == (len(sizes) - 1 if tail_from is None else tail_from) * (2 * 2 + 7) + 1
        z = M(rd).cpu().numpy()
        assert GM.same_bits(z, ref), f"tail_rows {tail_rows}: {np.count_nonzero(GM.bits(z) != GM.bits(ref))} entries differ from the mirror"
        assert GM.same_bits(M(rd).cpu().numpy(), ref), "the second apply differs from the first"
        assert M.applies == 2


@pytest.mark.parametrize("name", ["vardiff130x70", "vardiff130x70_shuffled"])
def test_device_hierarchy_has_the_cpu_hierarchys_bits(hipk, name):
    arrs = _arrays(name, np.float64)
    Mc, Md = MG.from_graph(MM.csr_tensor(*arrs), normalize=False), MG.from_graph(MM.csr_tensor(*arrs, device=DEV), normalize=False)
    assert len(Mc.levels) == len(Md.levels) and Mc.handshake_rounds == Md.handshake_rounds
    for a, b in zip(Mc.levels, Md.levels):
        assert (a.agg is None) == (b.agg is None) and (a.agg is None or torch.equal(a.agg, b.agg.cpu()))
        assert torch.equal(a.csr.crow_indices(), b.csr.crow_indices().cpu()) and torch.equal(a.csr.col_indices(), b.csr.col_indices().cpu())
        assert GM.same_bits(a.csr.values().numpy(), b.csr.values().cpu().numpy()) and GM.same_bits(a.dinv.numpy(), b.dinv.cpu().numpy())
        assert (a.c0, a.c1, a.c2) == (b.c0, b.c1, b.c2)
    with pytest.raises(ValueError, match="applied to"):
        Md(torch.ones(9100, dtype=torch.float64))


@pytest.mark.parametrize("tail_rows", [0, 64, 4096])
def test_launches_per_apply_is_the_count_of_the_wrappers_calls(hipk, monkeypatch, tail_rows):
    degree = 2
    M = MG.from_graph(MM.csr_tensor(*_arrays("vardiff130x70", np.float64), device=DEV), degree=degree, normalize=False, tail_rows=tail_rows)
    r = torch.ones(9100, dtype=torch.float64, device=DEV)
    M(r)                                                 # builds the device state
    count = {"launches": 0, "names": set()}
    weight = {"cheb_apply": degree + 1, "spmv_residual": 1, "mg_restrict_agg": 1, "mg_prolong_add_agg": 1, "mg_correct": 1, "mg_diag": 1,
              "mg_gtail_apply": 1, "mg_restrict": 1, "mg_prolong_add": 1, "mg_tail_apply": 1}
    for name, w in weight.items():
        def counted(*a, _f=getattr(hipk, name), _w=w, _n=name, **kw):
            count["launches"] += _w
            count["names"].add(_n)
            return _f(*a, **kw)
        monkeypatch.setattr(hipk, name, counted)
    M(r)
    torch.cuda.synchronize()
    assert count["launches"] == M.launches_per_apply
    assert not count["names"] & {"mg_restrict", "mg_prolong_add", "mg_tail_apply"}, "a graph hierarchy ran a grid kernel"
    assert ("mg_gtail_apply" in count["names"]) == (tail_rows > 0) and ("mg_diag" in count["names"]) == (tail_rows == 0)


# ------------------------------------------------------------------------------------------------------------ 4. whole solves
def _mirror_callable(oracle, M):
    def fn(v):
        return torch.from_numpy(GM.apply(oracle, M, v.cpu().numpy())).to(v.device)
    return fn


def _same_solve(solver, A, b, M, fn, method, **kw):
    x, info = solver(A, b, M=M, **kw)
    st = get_last_stats()
    xr, infor = solver(A, b, M=fn, **kw)
    sr = get_last_stats()
    assert st.method == sr.method == method, (st.method, sr.method)
    assert info == infor and st.iterations == sr.iterations and st.matvecs == sr.matvecs
    assert (st.b_norm, st.residual_norm, st.x_norm, st.threshold) == (sr.b_norm, sr.residual_norm, sr.x_norm, sr.threshold)
    assert GM.same_bits(x.cpu().numpy(), xr.cpu().numpy())
    return x, info, st


@pytest.mark.parametrize("name", ["vardiff130x70", "vardiff130x70_shuffled"])
def test_cg_solves_equal_the_mirror_driven_solves(hipk, oracle, name):
    A = MM.csr_tensor(*_arrays(name, np.float64), device=DEV)
    b = torch.ones(A.shape[0], dtype=torch.float64, device=DEV)
    M = MG.from_graph(A)
    x, info, st = _same_solve(cg, A, b, M, _mirror_callable(oracle, M), "cg_callable_M", tol=1e-6)
    relres = float(torch.linalg.vector_norm(b - A @ x) / torch.linalg.vector_norm(b))
    print(f"{name}: {st.iterations} iterations, relative residual {relres:.3e}")
    assert info == 0 and relres <= 1e-6 and M.applies >= st.iterations + 2      # the host queues iterations ahead of the stop word


def test_bicgstab_and_gmres_run_it_as_a_deterministic_left_preconditioner(hipk, oracle):
    A = create_convdiff_2d_csr(48, 32, device=DEV)
    b = torch.ones(A.shape[0], dtype=torch.float64, device=DEV)
    M = MG.from_graph(A)
    fn = _mirror_callable(oracle, M)
    _same_solve(bicgstab, A, b, M, fn, "bicgstab_callable_M", tol=1e-6)
    _same_solve(gmres, A, b, M, fn, "gmres_callable_M", tol=1e-6, restart=20)
