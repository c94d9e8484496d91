"""The device side of AggregationMultigridPreconditioner.from_graph(coarse_rows=K) against tests/_mg_dense_mirror.py, every comparison
bitwise:

1. hipk_mg_dense_apply between seeded guards: every size at which the segments or the workgroups change (one segment, 63 / 64 / 65
   columns, 255 - 257, 511 - 513, 1024, the envelope's last two), ld = n rounded up and padded by four more (the padding holds NaN:
   it is never read), both dtypes, scale 1 and != 1, the current and a side stream; the error codes, each writing no byte;
2. hipk_mg_gtail_dense_apply: the launch sequence's and the mirror's bits on hierarchies cut to 1, 2 and 4 or more levels, dense
   levels of 1, 15, 18, 35, 169, 328, 394, 473 and 512 unknowns, degrees 1 and 3, both dtypes; the workspace in the four states of
   tests/_arena.py with `work` of exactly hipk_mg_gtail_dense_work_bytes, a side stream, the refusals;
3. the whole apply at tail_rows 0 / 64 / 4096 x coarse_rows 64 / 512 / 2048, the two ways off the tail (a 49-entry row above the cut,
   a dense level of 513 rows), `launches_per_apply`, the device-built hierarchy and inverse against the CPU-built ones;
4. whole cg / bicgstab / gmres solves against the same solve whose M is a Python callable around the mirror."""
import ctypes

import numpy as np
import pytest
import torch

import _mg_dense_mirror as DM
import _mg_graph_mirror as GM
import _mg_mirror as MM
from _arena import Arena, check_memory, guard_bytes_for, run_states
from pytorch_sparse_solver.module_a import AggregationMultigridPreconditioner as MG
from pytorch_sparse_solver.module_a import bicgstab, cg, get_last_stats, gmres
from pytorch_sparse_solver.utils.matrix_utils import create_convdiff_2d_csr, create_poisson_2d_csr, create_variable_diffusion_2d_csr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [np.float64, np.float32]
ARG, ALIGN, UNSUPPORTED, WORKSPACE = -1, -3, -4, -5


def _np(A):
    A = A.cpu()
    return A.crow_indices().numpy(), A.col_indices().numpy(), A.values().numpy()


def _arena(a):
    """An array between guards, exactly its bytes of payload."""
    ar = Arena(DEV, a.nbytes, 16, guard_bytes_for(a.size, a.itemsize))
    return ar, ar.put(a)


# ------------------------------------------------------------------------------------------------------------ 1. the dense launch
def _stored(C, ld):
    """C[i, j] at j * ld + i, the padding NaN."""
    n = C.shape[0]
    flat = np.full(n * ld, np.nan, dtype=C.dtype)
    for j in range(n):
        flat[j * ld:j * ld + n] = C[:, j]
    return flat


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1024, 2047, 2048])
def test_dense_apply_has_the_mirrors_bits_between_guards(hipk, n, dtype):
    rng = np.random.default_rng([9, n])
    C, r = rng.standard_normal((n, n)).astype(dtype), rng.standard_normal(n).astype(dtype)
    C[n // 2, :] = 0.0                                    # a row of signed zeros: s = 0, s = s + p_q gives +0
    ref = DM.segmented(C, r)
    side = torch.cuda.Stream(device=DEV)
    r_ar, r_d = _arena(r)
    r_ar.snapshot()
    for ld, scale, stream in (((n + 3) & ~3, 1.0, None), (((n + 3) & ~3) + 4, 0.37, side), ((n + 3) & ~3, 0.37, None)):
        c_ar, c_d = _arena(_stored(C, ld))
        c_ar.snapshot()
        z_ar, z_d = _arena(np.full(n, np.nan, dtype=dtype))
        torch.cuda.synchronize()
        with torch.cuda.stream(side if stream is not None else torch.cuda.current_stream(DEV)):
            hipk.mg_dense_apply(c_d, ld, scale, r_d, z_d)
        torch.cuda.synchronize()
        check_memory({"z": z_ar, "r": r_ar, "cinv": c_ar}, {"r": r_ar, "cinv": c_ar}, f"hipk_mg_dense_apply n = {n}, ld = {ld}")
        got, want = z_d.cpu().numpy(), (dtype(scale) * ref if scale != 1.0 else ref)
        assert DM.same_bits(got, want), f"n = {n}, ld = {ld}, scale {scale}: {np.count_nonzero(DM.bits(got) != DM.bits(want))} of {n} differ"


def test_dense_apply_error_codes_write_nothing(hipk):
    L = hipk.lib()
    n, ld = 64, 64
    c = torch.full((2052 * 2052,), 3.0, dtype=torch.float64, device=DEV)
    r = torch.ones(2052, dtype=torch.float64, device=DEV)
    z = torch.full((2052,), 7.0, dtype=torch.float64, device=DEV)
    p = lambda x: x.data_ptr()
    assert L.hipk_mg_dense_apply(0, 0, p(c), 1.0, p(r), p(z), 1, None) == ARG
    assert L.hipk_mg_dense_apply(2049, 2052, p(c), 1.0, p(r), p(z), 1, None) == UNSUPPORTED
    assert L.hipk_mg_dense_apply(n, n - 4, p(c), 1.0, p(r), p(z), 1, None) == ARG           # ld < n
    assert L.hipk_mg_dense_apply(63, 63, p(c), 1.0, p(r), p(z), 1, None) == ALIGN           # an odd ld
    assert L.hipk_mg_dense_apply(n, ld + 2, p(c), 1.0, p(r), p(z), 1, None) == ALIGN
    assert L.hipk_mg_dense_apply(n, ld, None, 1.0, p(r), p(z), 1, None) == ARG
    assert L.hipk_mg_dense_apply(n, ld, p(c), 1.0, None, p(z), 1, None) == ARG
    assert L.hipk_mg_dense_apply(n, ld, p(c), 1.0, p(r), None, 1, None) == ARG
    assert L.hipk_mg_dense_apply(n, ld, p(c) + 8, 1.0, p(r), p(z), 1, None) == ALIGN
    assert L.hipk_mg_dense_apply(n, ld, p(c), 1.0, p(r) + 8, p(z), 1, None) == ALIGN
    assert L.hipk_mg_dense_apply(n, ld, p(c), 1.0, p(r), p(z) + 8, 1, None) == ALIGN
    assert L.hipk_mg_dense_apply(n, ld, p(c), 1.0, p(z), p(z), 1, None) == ARG              # r == z
    assert L.hipk_mg_dense_apply(n, ld, p(c), 1.0, p(r), p(z), 7, None) == UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((z == 7.0).all()) and bool((r == 1.0).all()) and bool((c == 3.0).all())
    assert L.hipk_mg_dense_apply(n, ld, p(c), 1.0, p(r), p(z), 1, None) == 0
    torch.cuda.synchronize()
    assert bool((z[:n] == 192.0).all()) and bool((z[n:] == 7.0).all())
    with pytest.raises(AssertionError, match="cinv"):
        hipk.mg_dense_apply(c[:n * ld - 1], ld, 1.0, r[:n], z[:n])


# ------------------------------------------------------------------------------------------------------------ 2. the tail kernel
def _arrays(name, dtype):
    if name == "poisson37x29":
        arrs = _np(create_poisson_2d_csr(37, 29))
    elif name == "poisson47x36":
        arrs = _np(create_poisson_2d_csr(47, 36))
    elif name == "poisson39x43":
        arrs = _np(create_poisson_2d_csr(39, 43))
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
    elif name == "box49_12x12":
        arrs = MM.grid_matrix((12, 12), radius=3, full_box=True)
    else:
        raise KeyError(name)
    return arrs[0], arrs[1], arrs[2].astype(dtype)


_built = {}


def _hierarchy(name, dtype, degree, device, tail_rows, coarse_rows):
    """One object per argument list, shared by the tests of this file (an apply does not change it)."""
    key = (name, np.dtype(dtype).name, degree, device, tail_rows, coarse_rows)
    if key not in _built:
        _built[key] = MG.from_graph(MM.csr_tensor(*_arrays(name, dtype), device=device), degree=degree, tail_rows=tail_rows,
                                    coarse_rows=coarse_rows)
    return _built[key]


# (matrix, coarse_rows, the level sizes it gives)
TAIL_CASES = [("two_blocks", 473, [473]), ("poisson37x29", 328, [1073, 328]), ("seven_point12x11x10", 394, [1320, 394]),
              ("poisson47x36", 512, [1692, 512]), ("vardiff64x64", 169, [4096, 1275, 446, 169]), ("poisson37x29", 15, [1073, 328, 107, 37, 15]),
              ("seven_point12x11x10", 35, [1320, 394, 115, 35]), ("two_blocks", 18, [473, 145, 50, 18]),
              ("vardiff64x64", 1, [4096, 1275, 446, 169, 72, 34, 16, 10, 6, 4, 2, 1])]


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
@pytest.mark.parametrize("degree", [1, 3])
@pytest.mark.parametrize("name, K, sizes", TAIL_CASES, ids=[f"{c[0]}-{c[1]}" for c in TAIL_CASES])
def test_tail_kernel_equals_the_launch_sequence_and_the_mirror(hipk, oracle, name, K, sizes, degree, dtype):
    Mt, Ms = _hierarchy(name, dtype, degree, DEV, 4096, K), _hierarchy(name, dtype, degree, DEV, 0, K)
    assert [lev.n for lev in Mt.levels] == sizes == [lev.n for lev in Ms.levels] and Mt.dense and Ms.dense
    assert Mt.tail_from == 0 and Ms.tail_from is None and Mt.launches_per_apply == 1
    assert Ms.launches_per_apply == (len(sizes) - 1) * (2 * degree + 7) + 1
    assert Mt.scale == Ms.scale != 1.0
    n = Mt.shape[0]
    r = np.random.default_rng([5, n]).standard_normal(n).astype(dtype)
    rd = torch.from_numpy(r).to(DEV)
    zt, zs = Mt(rd).cpu().numpy(), Ms(rd).cpu().numpy()
    assert torch.equal(rd.cpu(), torch.from_numpy(r))
    assert isinstance(Mt._tail, hipk.MgGTail) and Mt._tail.cinv is not None and Mt._tail.nlev == len(sizes)
    ref = DM.apply(oracle, Ms, r)
    assert DM.same_bits(zs, ref), f"launch sequence: {np.count_nonzero(DM.bits(zs) != DM.bits(ref))} of {n} entries differ from the mirror"
    assert DM.same_bits(zt, ref), f"tail kernel: {np.count_nonzero(DM.bits(zt) != DM.bits(ref))} of {n} entries differ from the mirror"


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
@pytest.mark.parametrize("name, K", [("vardiff64x64", 169), ("two_blocks", 473)])
def test_tail_kernel_workspace_states_side_stream_and_guards(hipk, oracle, name, K, dtype):
    M = _hierarchy(name, dtype, 3, DEV, 4096, K)
    n = M.shape[0]
    r = np.random.default_rng(8).standard_normal(n).astype(dtype)
    ref = DM.apply(oracle, M, r)
    M(torch.from_numpy(r).to(DEV))                       # builds the descriptors
    tail = M._tail
    assert tail.work_bytes == hipk.lib().hipk_mg_gtail_dense_work_bytes(tail.host, tail.nlev, 1 if dtype == np.float64 else 0) > 0
    assert tail.work_bytes == (sum(5 * ((lev.n + 3) & ~3) for lev in M.levels) * r.itemsize + 255) // 256 * 256
    work = Arena(DEV, tail.work_bytes, 256, guard_bytes_for(n, r.itemsize))
    r_ar, r_d = _arena(r)
    z_ar, z_d = _arena(np.zeros_like(r))
    side = torch.cuda.Stream(device=DEV)

    def run(i):
        z_d.fill_(float("nan"))
        torch.cuda.synchronize()
        with torch.cuda.stream(side if i % 2 else torch.cuda.current_stream(DEV)):
            hipk.mg_gtail_dense_apply(tail, M.omega, M.scale, r_d, z_d, work=work.payload)
        torch.cuda.synchronize()
        return {"z": z_d.cpu().numpy().tobytes()}

    res = run_states(work, {"z": z_ar, "r": r_ar}, {"r": r_ar}, run, label=f"hipk_mg_gtail_dense_apply {name}")
    assert res[0]["z"] == ref.tobytes()


def test_tail_kernel_error_codes_write_nothing(hipk):
    M = _hierarchy("poisson47x36", np.float64, 1, DEV, 4096, 512)
    r = torch.ones(M.shape[0], dtype=torch.float64, device=DEV)
    M(r)
    tail, L = M._tail, hipk.lib()
    assert tail.nlev == 2 and tail.host[1].n == 512 and tail.ld == 512 and not tail.host[1].crow and not tail.host[1].dinv
    z = torch.full_like(r, 7.0)
    work = torch.full((tail.work_bytes,), 0x5A, dtype=torch.uint8, device=DEV)

    def call(host=None, nlev=None, degree=1, cp=0, ld=None, rp=None, zp=None, wp=None, wb=None, dtype=1):
        return L.hipk_mg_gtail_dense_apply(tail.host if host is None else host, tail.blob.data_ptr(), tail.nlev if nlev is None else nlev, degree,
                                           1.8, 1.0, tail.cinv.data_ptr() if cp == 0 else cp, tail.ld if ld is None else ld,
                                           r.data_ptr() if rp is None else rp, z.data_ptr() if zp is None else zp, dtype,
                                           work.data_ptr() if wp is None else wp, tail.work_bytes if wb is None else wb, None)

    def edited(level=0, count=None, **kw):
        host = (hipk.MgGLevel * (count or tail.nlev))()
        ctypes.memmove(host, tail.host, ctypes.sizeof(tail.host))
        for j in range(tail.nlev, len(host)):            # further levels: copies of the last one
            ctypes.memmove(ctypes.byref(host[j]), ctypes.byref(tail.host[tail.nlev - 1]), ctypes.sizeof(hipk.MgGLevel))
        for k, v in kw.items():
            setattr(host[level], k, v)
        return host

    assert call(host=edited(level=1, n=513)) == UNSUPPORTED           # a dense level of 513 rows
    assert call(host=edited(max_row=33)) == UNSUPPORTED               # a sparse level with a 33-entry row
    assert call(host=edited(n=4097)) == UNSUPPORTED
    assert call(host=edited(level=1, max_row=33)) == 0                # of the last descriptor only n is read
    torch.cuda.synchronize()
    assert not bool((z == 7.0).any())
    z.fill_(7.0)
    work.fill_(0x5A)
    assert call(host=edited(count=33), nlev=33) == UNSUPPORTED
    assert L.hipk_mg_gtail_dense_work_bytes(edited(count=33), 33, 1) == 0 and L.hipk_mg_gtail_dense_work_bytes(tail.host, 0, 1) == 0
    assert call(dtype=5) == UNSUPPORTED
    assert call(degree=0) == ARG and call(degree=33) == ARG
    assert call(nlev=0) == ARG
    assert call(host=edited(level=1, n=0)) == ARG and call(host=edited(n=0)) == ARG
    assert call(host=edited(n=500)) == ARG                            # the dense level has more unknowns than the level above
    assert call(host=edited(aptr=None)) == ARG and call(host=edited(dinv=None)) == ARG
    assert call(cp=None) == ARG and call(ld=508) == ARG and call(ld=514) == ALIGN and call(cp=tail.cinv.data_ptr() + 8) == ALIGN
    assert call(zp=r.data_ptr()) == ARG
    assert call(rp=r.data_ptr() + 8) == ALIGN and call(wp=work.data_ptr() + 16) == ALIGN
    assert call(wb=tail.work_bytes - 1) == WORKSPACE
    torch.cuda.synchronize()
    assert bool((z == 7.0).all()) and bool((work == 0x5A).all())
    M0 = _hierarchy("poisson37x29", np.float64, 1, DEV, 4096, None)      # a tail without a dense level, and the other way round
    M0(r[:1073].clone())
    with pytest.raises(AssertionError, match="dense"):
        hipk.mg_gtail_dense_apply(M0._tail, 1.8, 1.0, r[:1073].clone(), z[:1073].clone())
    with pytest.raises(AssertionError, match="dense"):
        hipk.mg_gtail_apply(tail, 1.8, 1.0, r, z)


# ------------------------------------------------------------------------------------------------------------ 3. the whole apply
def _count_launches(hipk, monkeypatch, M, r, degree):
    """The wrappers one apply calls (name -> calls) and their launches, a Chebyshev apply counting degree + 1."""
    weight = {"cheb_apply": degree + 1, "spmv_residual": 1, "mg_restrict_agg": 1, "mg_prolong_add_agg": 1, "mg_correct": 1, "mg_diag": 1,
              "mg_gtail_apply": 1, "mg_restrict": 1, "mg_prolong_add": 1, "mg_tail_apply": 1, "mg_dense_apply": 1, "mg_gtail_dense_apply": 1}
    count = {"launches": 0, "names": {}}
    with monkeypatch.context() as mp:
        for name, w in weight.items():
            def counted(*a, _f=getattr(hipk, name), _w=w, _n=name, **kw):
                count["launches"] += _w
                count["names"][_n] = count["names"].get(_n, 0) + 1
                return _f(*a, **kw)
            mp.setattr(hipk, name, counted)
        z = M(r)
        torch.cuda.synchronize()
    return count, z


@pytest.mark.parametrize("K", [64, 512, 2048])
@pytest.mark.parametrize("name", ["vardiff130x70", "vardiff130x70_shuffled"])
def test_whole_apply_is_the_mirror_at_every_tail_size_and_cut(hipk, oracle, monkeypatch, name, K):
    A = MM.csr_tensor(*_arrays(name, np.float64), device=DEV)
    r = np.random.default_rng(17).standard_normal(A.shape[0])
    rd = torch.from_numpy(r).to(DEV)
    default = [lev.n for lev in _hierarchy(name, np.float64, 1, "cpu", 0, None).levels]
    assert default[:4] in ([9100, 2847, 1002, 376], [9100, 2852, 1006, 394])
    ref = scale = None
    sizes = default[:next(l for l, n in enumerate(default) if n <= K) + 1]
    for tail_rows in (0, 64, 4096):
        M = MG.from_graph(A, degree=2, tail_rows=tail_rows, coarse_rows=K)
        if ref is None:
            ref, scale = DM.apply(oracle, M, r), M.scale
        assert [lev.n for lev in M.levels] == sizes and M.scale == scale and M.dense
        first = next((l for l, n in enumerate(sizes) if n <= tail_rows), None)
        tail_from = first if first is not None and sizes[-1] <= 512 else None
        assert M.tail_from == tail_from, (K, tail_rows)
        assert M.launches_per_apply == (len(sizes) - 1 if tail_from is None else tail_from) * (2 * 2 + 7) + 1
        z = M(rd).cpu().numpy()
        assert DM.same_bits(z, ref), f"coarse_rows {K}, tail_rows {tail_rows}: {np.count_nonzero(DM.bits(z) != DM.bits(ref))} entries differ"
        count, z2 = _count_launches(hipk, monkeypatch, M, rd, 2)
        assert DM.same_bits(z2.cpu().numpy(), ref), "the second apply differs from the first"
        assert count["launches"] == M.launches_per_apply and M.applies == 2
        last = "mg_dense_apply" if tail_from is None else "mg_gtail_dense_apply"
        others = {"mg_diag", "mg_gtail_apply", "mg_tail_apply", "mg_restrict", "mg_prolong_add", "mg_dense_apply", "mg_gtail_dense_apply"} - {last}
        assert count["names"].get(last) == 1 and not set(count["names"]) & others


@pytest.mark.parametrize("name, K, why", [("box49_12x12", 20, "a row of 49 entries above the cut"), ("poisson39x43", 513, "a dense level of 513 rows")])
def test_hierarchies_outside_the_tails_envelope_stay_on_launches_and_end_in_the_dense_launch(hipk, oracle, monkeypatch, name, K, why):
    arrs = _arrays(name, np.float64)
    M = MG.from_graph(MM.csr_tensor(*arrs, device=DEV), tail_rows=4096, coarse_rows=K)
    L = len(M.levels) - 1
    assert M.dense and L >= 1 and M.levels[0].n <= 4096, why
    if name == "box49_12x12":
        assert np.diff(arrs[0]).max() == 49 and M.levels[0].max_row == 49 and M.levels[-1].n <= 20
    else:
        assert M.levels[-1].n == 513 and all(lev.max_row <= 32 for lev in M.levels)
    assert M.tail_from is None and M.launches_per_apply == L * 9 + 1
    r = np.random.default_rng(2).standard_normal(M.shape[0])
    count, z = _count_launches(hipk, monkeypatch, M, torch.from_numpy(r).to(DEV), 1)
    assert count["launches"] == M.launches_per_apply and count["names"].get("mg_dense_apply") == 1
    assert not set(count["names"]) & {"mg_diag", "mg_gtail_apply", "mg_gtail_dense_apply"}
    assert DM.same_bits(z.cpu().numpy(), DM.apply(oracle, M, r))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
@pytest.mark.parametrize("name, K", [("vardiff130x70", 2048), ("vardiff130x70_shuffled", 512), ("two_blocks", 473)])
def test_device_hierarchy_and_inverse_have_the_cpu_built_bits(hipk, name, K, dtype):
    arrs = _arrays(name, dtype)
    Mc = MG.from_graph(MM.csr_tensor(*arrs), normalize=False, coarse_rows=K)
    Md = MG.from_graph(MM.csr_tensor(*arrs, device=DEV), normalize=False, coarse_rows=K)
    assert len(Mc.levels) == len(Md.levels) and Mc.handshake_rounds == Md.handshake_rounds and Mc.dense and Md.dense
    assert (Mc.tail_from, Mc.launches_per_apply) == (Md.tail_from, Md.launches_per_apply)
    for a, b in zip(Mc.levels, Md.levels):
        assert (a.agg is None) == (b.agg is None) and (a.agg is None or torch.equal(a.agg, b.agg.cpu()))
        assert torch.equal(a.csr.crow_indices(), b.csr.crow_indices().cpu()) and torch.equal(a.csr.col_indices(), b.csr.col_indices().cpu())
        assert DM.same_bits(a.csr.values().numpy(), b.csr.values().cpu().numpy())
        assert (a.c0, a.c1, a.c2) == (b.c0, b.c1, b.c2) and (a.dinv is None) == (b.dinv is None)
        assert a.dinv is None or DM.same_bits(a.dinv.numpy(), b.dinv.cpu().numpy())
    a, b = Mc.levels[-1], Md.levels[-1]
    assert b.cinv.device.type == "cuda" and a.cinv.shape == b.cinv.shape == (a.n, (a.n + 3) & ~3) and a.ld == b.ld
    assert DM.same_bits(a.cinv.numpy(), b.cinv.cpu().numpy())
    ref = DM.stored_inverse(DM.dense_matrix(*_np(a.csr)))
    assert DM.same_bits(b.cinv.cpu().reshape(-1).numpy(), ref)


# ------------------------------------------------------------------------------------------------------------ 4. whole solves
def _mirror_callable(oracle, M):
    def fn(v):
        return torch.from_numpy(DM.apply(oracle, M, v.cpu().numpy())).to(v.device)
    return fn


def _same_solve(solver, A, b, M, fn, method, **kw):
    x, info = solver(A, b, M=M, **kw)
    st = get_last_stats()
    xr, infor = solver(A, b, M=fn, **kw)
    sr = get_last_stats()
    assert st.method == sr.method == method, (st.method, sr.method)
    assert info == infor and st.iterations == sr.iterations and st.matvecs == sr.matvecs
    assert (st.b_norm, st.residual_norm, st.x_norm, st.threshold) == (sr.b_norm, sr.residual_norm, sr.x_norm, sr.threshold)
    assert DM.same_bits(x.cpu().numpy(), xr.cpu().numpy())
    return x, info, st


@pytest.mark.parametrize("name, K", [("vardiff130x70", 512), ("vardiff130x70_shuffled", 2048)])
def test_cg_solves_equal_the_mirror_driven_solves(hipk, oracle, name, K):
    A = MM.csr_tensor(*_arrays(name, np.float64), device=DEV)
    b = torch.ones(A.shape[0], dtype=torch.float64, device=DEV)
    M = MG.from_graph(A, coarse_rows=K)
    assert M.dense and (M.tail_from is None) == (K == 2048)
    x, info, st = _same_solve(cg, A, b, M, _mirror_callable(oracle, M), "cg_callable_M", tol=1e-6)
    relres = float(torch.linalg.vector_norm(b - A @ x) / torch.linalg.vector_norm(b))
    print(f"{name}, coarse_rows {K}: {len(M.levels)} levels, {st.iterations} iterations, relative residual {relres:.3e}")
    assert info == 0 and relres <= 1e-6 and M.applies >= st.iterations + 2      # the host queues iterations ahead of the stop word


def test_bicgstab_and_gmres_run_it_as_a_deterministic_left_preconditioner(hipk, oracle):
    A = create_convdiff_2d_csr(48, 32, device=DEV)
    b = torch.ones(A.shape[0], dtype=torch.float64, device=DEV)
    M = MG.from_graph(A, coarse_rows=256)
    assert M.dense and [lev.n for lev in M.levels] == [1536, 473, 156]
    fn = _mirror_callable(oracle, M)
    _same_solve(bicgstab, A, b, M, fn, "bicgstab_callable_M", tol=1e-6)
    _same_solve(gmres, A, b, M, fn, "gmres_callable_M", tol=1e-6, restart=20)
