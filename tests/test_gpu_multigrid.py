"""The device side of AggregationMultigridPreconditioner against tests/_mg_mirror.py, every comparison bitwise:

1. hipk_mg_restrict / hipk_mg_prolong_add (and hipk_mg_correct / hipk_mg_diag) between seeded guards, both dtypes, on grids with
   ragged 16-byte groups, an odd last row or plane, a dimension of 1, a single point, and one of two million points (more than a
   thousand chunks, each thread several rounds of its chunk's loop);
2. hipk_mg_tail_apply: the launch sequence's and the mirror's bits on small grids, Poisson / variable-coefficient / shuffled-row
   matrices, degrees 1 - 3, both dtypes; the workspace in the four states of tests/_arena.py, a side stream, the error codes, and a
   matrix with rows of 49 entries that the tail must refuse; hipk_mg_gtail_apply on the boxes written out as index arrays, which
   must return the same bits;
3. the whole apply at tail_rows 0 / 256 / 1024 / 4096 with levels above the tail, and `launches_per_apply`;
4. whole cg / bicgstab / gmres solves against the same solve whose M is a Python callable around the mirror;
5. one user-sized cg solve: a tenth of plain cg's iterations."""
import ctypes

import numpy as np
import pytest
import torch

import _mg_mirror as MM
from _arena import Arena, check_memory, guard_bytes_for, run_states
from _batch_patterns import build_pattern
from _order_cases import TRANSFORMS
from pytorch_sparse_solver.module_a import AggregationMultigridPreconditioner as MG
from pytorch_sparse_solver.module_a import bicgstab, cg, get_last_stats, gmres
from pytorch_sparse_solver.module_a.multigrid import _aggregate_of
from pytorch_sparse_solver.utils.matrix_utils import create_convdiff_2d_csr, create_poisson_2d_csr, create_variable_diffusion_2d_csr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [np.float64, np.float32]
TRANSFER_GRIDS = [(1, 1), (1, 2), (2, 1), (3, 3), (17, 13), (64, 64), (255, 257), (1030, 3), (5, 1, 3), (2, 2, 2), (9, 8, 7), (1449, 1451)]


def _arena(a):
    """A vector between guards, exactly its bytes of payload."""
    ar = Arena(DEV, a.nbytes, 16, guard_bytes_for(a.size, a.itemsize))
    return ar, ar.put(a)


# ------------------------------------------------------------------------------------------------------------ 1. transfer kernels
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
@pytest.mark.parametrize("grid", TRANSFER_GRIDS, ids=lambda g: "x".join(map(str, g)))
def test_transfer_kernels_have_the_mirrors_bits_between_guards(hipk, grid, dtype):
    n, nc = int(np.prod(grid)), int(np.prod(MM.coarse(grid)))
    rng = np.random.default_rng([3, n])
    t, e, z0 = (rng.standard_normal(k).astype(dtype) for k in (n, nc, n))
    t_ar, t_d = _arena(t)
    rc_ar, rc_d = _arena(rng.standard_normal(nc).astype(dtype))
    t_ar.snapshot()
    hipk.mg_restrict(grid, t_d, rc_d)
    torch.cuda.synchronize()
    check_memory({"rc": rc_ar, "t": t_ar}, {"t": t_ar}, f"hipk_mg_restrict {grid}")
    assert MM.same_bits(rc_d.cpu().numpy(), MM.restrict(t, grid)), f"hipk_mg_restrict {grid}"

    e_ar, e_d = _arena(e)
    z_ar, z_d = _arena(z0)
    e_ar.snapshot()
    hipk.mg_prolong_add(grid, 1.8, e_d, z_d)
    torch.cuda.synchronize()
    check_memory({"z": z_ar, "e": e_ar}, {"e": e_ar}, f"hipk_mg_prolong_add {grid}")
    z1 = MM.prolong_add(z0, e, 1.8, grid)
    assert MM.same_bits(z_d.cpu().numpy(), z1), f"hipk_mg_prolong_add {grid}"

    f = dtype
    hipk.mg_correct(0.37, t_d, z_d)                      # z = scale * (z + d)
    torch.cuda.synchronize()
    check_memory({"z": z_ar, "t": t_ar}, {"t": t_ar}, f"hipk_mg_correct {grid}")
    assert MM.same_bits(z_d.cpu().numpy(), f(0.37) * (z1 + t))
    hipk.mg_diag(1.0, t_d, torch.from_numpy(z0).to(DEV), z_d)      # z = scale * (dinv * r)
    torch.cuda.synchronize()
    check_memory({"z": z_ar, "t": t_ar}, {"t": t_ar}, f"hipk_mg_diag {grid}")
    assert MM.same_bits(z_d.cpu().numpy(), f(1.0) * (t * z0))


def test_transfer_kernels_refuse_bad_arguments(hipk):
    L = hipk.lib()
    v = torch.zeros(64, dtype=torch.float64, device=DEV)
    w = torch.zeros(64, dtype=torch.float64, device=DEV)
    assert L.hipk_mg_restrict(0, 4, 4, v.data_ptr(), w.data_ptr(), 1, None) == -1
    assert L.hipk_mg_restrict(1, 4, 4, v.data_ptr(), v.data_ptr(), 1, None) == -1
    assert L.hipk_mg_restrict(1, 4, 4, v.data_ptr() + 8, w.data_ptr(), 1, None) == -3
    assert L.hipk_mg_prolong_add(1, 4, 4, 1.8, None, w.data_ptr(), 1, None) == -1
    assert L.hipk_mg_prolong_add(1, 4, 4, 1.8, v.data_ptr(), w.data_ptr(), 7, None) == -4
    torch.cuda.synchronize()
    assert not bool(v.any()) and not bool(w.any())


# ------------------------------------------------------------------------------------------------------------ 2. the tail kernel
def _matrix(kind, grid, dtype):
    """(crow, col, val) of a grid matrix: 'poisson' (constant stencil), 'vardiff' (seeded weights), 'shuf' (seeded weights, every
    row in a seeded order)."""
    if kind == "poisson":
        return MM.grid_matrix(grid, dtype=dtype)
    arrs = MM.grid_matrix(grid, seed=9, dtype=dtype)
    return TRANSFORMS["shuf"](*arrs, seed=4) if kind == "shuf" else arrs


TAIL_GRIDS = [(64, 64), (63, 65), (17, 13), (2, 1), (1, 1), (16, 16, 16), (5, 1, 3)]
KINDS = ("poisson", "vardiff", "shuf")


def _tail_cases():
    """Every grid with every matrix kind; degree and dtype rotate so that each grid sees degrees 1, 2, 3 and both dtypes, and (17, 13), ragged
    in both dimensions on most levels, the full cross."""
    for gi, grid in enumerate(TAIL_GRIDS):
        for ki, kind in enumerate(KINDS):
            if grid == (17, 13):
                for degree in (1, 2, 3):
                    for dtype in DTYPES:
                        yield grid, kind, degree, dtype
            else:
                yield grid, kind, ki + 1, DTYPES[(gi + ki) % 2]
                yield grid, kind, (ki + 1) % 3 + 1, DTYPES[(gi + ki + 1) % 2]


@pytest.mark.parametrize("grid, kind, degree, dtype", list(_tail_cases()),
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else getattr(v, "__name__", str(v)))
def test_tail_kernel_equals_the_launch_sequence_and_the_mirror(hipk, oracle, grid, kind, degree, dtype):
    A = MM.csr_tensor(*_matrix(kind, grid, dtype), device=DEV)
    Mt = MG(A, grid, degree=degree, tail_rows=4096)
    Ms = MG(A, grid, degree=degree, tail_rows=0)
    assert Mt.tail_from == 0 and Ms.tail_from is None and Mt.launches_per_apply == 1
    assert Mt.scale == Ms.scale != 1.0
    r = np.random.default_rng([5, A.shape[0]]).standard_normal(A.shape[0]).astype(dtype)
    rd = torch.from_numpy(r).to(DEV)
    zt, zs = Mt(rd).cpu().numpy(), Ms(rd).cpu().numpy()
    assert torch.equal(rd.cpu(), torch.from_numpy(r))
    ref = MM.apply(oracle, Ms, r)
    assert MM.same_bits(zs, ref), f"launch sequence: {np.count_nonzero(MM.bits(zs) != MM.bits(ref))} of {r.size} entries differ from the mirror"
    assert MM.same_bits(zt, ref), f"tail kernel: {np.count_nonzero(MM.bits(zt) != MM.bits(ref))} of {r.size} entries differ from the mirror"


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
def test_tail_kernel_workspace_states_side_stream_and_guards(hipk, oracle, dtype):
    grid = (63, 65)
    A = MM.csr_tensor(*_matrix("vardiff", grid, dtype), device=DEV)
    M = MG(A, grid, degree=2, tail_rows=4096)
    r = np.random.default_rng(8).standard_normal(A.shape[0]).astype(dtype)
    ref = MM.apply(oracle, M, r)
    M(torch.from_numpy(r).to(DEV))                       # builds the descriptors
    tail = M._tail
    assert tail.work_bytes == hipk.lib().hipk_mg_tail_work_bytes(tail.host, tail.nlev, 1 if dtype == np.float64 else 0) > 0
    work = Arena(DEV, tail.work_bytes, 256, guard_bytes_for(A.shape[0], r.itemsize))
    r_ar, r_d = _arena(r)
    z_ar, z_d = _arena(np.zeros_like(r))
    side = torch.cuda.Stream(device=DEV)

    def run(i):
        z_d.fill_(float("nan"))
        torch.cuda.synchronize()
        with torch.cuda.stream(side if i % 2 else torch.cuda.current_stream(DEV)):
            hipk.mg_tail_apply(tail, M.omega, M.scale, r_d, z_d, work=work.payload)
        torch.cuda.synchronize()
        return {"z": z_d.cpu().numpy().tobytes()}

    res = run_states(work, {"z": z_ar, "r": r_ar}, {"r": r_ar}, run, label=f"hipk_mg_tail_apply {grid}")
    assert res[0]["z"] == ref.tobytes()


def test_tail_kernel_error_codes_write_nothing(hipk):
    grid = (17, 13)
    A = MM.csr_tensor(*_matrix("poisson", grid, np.float64), device=DEV)
    M = MG(A, grid, tail_rows=4096)
    r = torch.ones(A.shape[0], dtype=torch.float64, device=DEV)
    M(r)
    tail, L = M._tail, hipk.lib()
    z = torch.full_like(r, 7.0)
    work = torch.full((tail.work_bytes,), 0x5A, dtype=torch.uint8, device=DEV)

    def call(host=None, nlev=None, degree=1, rp=None, zp=None, wp=None, wb=None, dtype=1):
        return L.hipk_mg_tail_apply(tail.host if host is None else host, tail.blob.data_ptr(), tail.nlev if nlev is None else nlev, degree,
                                    1.8, 1.0, r.data_ptr() if rp is None else rp, z.data_ptr() if zp is None else zp, dtype,
                                    work.data_ptr() if wp is None else wp, tail.work_bytes if wb is None else wb, None)

    def edited(**kw):
        host = (hipk.MgLevel * tail.nlev)()
        ctypes.memmove(host, tail.host, ctypes.sizeof(host))
        for k, v in kw.items():
            setattr(host[0], k, v)
        return host

    assert call(host=edited(max_row=33)) == -4                        # HIPK_ERR_UNSUPPORTED: a row beyond the envelope
    assert call(host=edited(n=4097, n0=1, n1=1, n2=4097)) == -4
    assert call(dtype=5) == -4
    assert call(degree=0) == -1 and call(degree=33) == -1             # HIPK_ERR_ARG
    assert call(nlev=0) == -1 and call(nlev=17) == -1
    assert call(nlev=tail.nlev - 1) == -1                             # the last level must have one unknown
    assert call(host=edited(n1=16)) == -1                             # n is not the product of the dimensions
    assert call(zp=r.data_ptr()) == -1
    assert call(rp=r.data_ptr() + 8) == -3 and call(wp=work.data_ptr() + 16) == -3      # HIPK_ERR_ALIGN
    assert call(wb=tail.work_bytes - 1) == -5                         # HIPK_ERR_WORKSPACE
    assert L.hipk_mg_tail_work_bytes(tail.host, 0, 1) == 0
    torch.cuda.synchronize()
    assert bool((z == 7.0).all()) and bool((work == 0x5A).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool((z == 7.0).any())


@pytest.mark.parametrize("pattern, transform, grid, max_row, in_tail", [
    (("rag32", 300), None, (20, 15), 32, True),        # rows of 1 .. 32 stored entries side by side, two 256-row tiles
    (("dense32",), None, (4, 8), 32, True),            # every row exactly 32
    (("dense32",), "dup", (4, 8), 33, False),          # one entry of every row split in two: 33, outside the envelope
], ids=["rag32", "dense32", "dense32_dup"])
def test_tail_kernel_at_the_32_entry_edge(hipk, oracle, pattern, transform, grid, max_row, in_tail):
    crow, col, vals = build_pattern(pattern, transform, "cg", 1, np.random.default_rng(1))
    A = MM.csr_tensor(crow, col, vals[0], device=DEV)
    Mt, Ms = MG(A, grid, degree=2, tail_rows=4096), MG(A, grid, degree=2, tail_rows=0)
    assert Mt.levels[0].max_row == max_row == int(np.diff(crow).max())
    assert Mt.tail_from == (0 if in_tail else None) and Mt.scale == Ms.scale
    r = np.random.default_rng(6).standard_normal(A.shape[0])
    rd = torch.from_numpy(r).to(DEV)
    ref = MM.apply(oracle, Ms, r)
    assert MM.same_bits(Ms(rd).cpu().numpy(), ref) and MM.same_bits(Mt(rd).cpu().numpy(), ref)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
@pytest.mark.parametrize("grid, sizes, members", [((17, 13), [221, 63, 20, 6, 2, 1], 4), ((5, 4, 3), [60, 12, 2, 1], 8)], ids=["17x13", "5x4x3"])
def test_box_and_index_levels_are_one_walk(hipk, grid, sizes, members, dtype):
    """hipk_mg_tail_kernel and hipk_mg_gtail_kernel differ in the two transfers only: given the boxes as index arrays -- members in
    ascending fine index are exactly the box order -- the index-array tail returns the box tail's bits, and both the launch
    sequence's.  Odd and even extents: aggregates of 1, 2 and 4 (in three dimensions up to 8) members."""
    A = MM.csr_tensor(*_matrix("poisson", grid, dtype), device=DEV)
    Mt = MG(A, grid, degree=2, normalize=False, tail_rows=4096)
    Ms = MG(A, grid, degree=2, normalize=False, tail_rows=0)
    assert [lev.n for lev in Mt.levels] == sizes and Mt.tail_from == 0 and Ms.tail_from is None
    levels = [dict(s) for s in Mt._dev_state()]          # the dicts Mt._tail was built from
    for s, lev in zip(levels[:-1], Mt.levels):
        agg = _aggregate_of(torch.arange(lev.n, device=DEV), lev.dims)
        counts = torch.bincount(agg)
        assert 1 <= int(counts.min()) and int(counts.max()) <= members
        s["agg"] = hipk.aligned(agg.to(torch.int32))
        s["amem"] = hipk.aligned(torch.sort(agg, stable=True)[1].to(torch.int32))
        s["aptr"] = hipk.aligned(torch.cat([counts.new_zeros(1), torch.cumsum(counts, 0)]).to(torch.int32))
    assert int(torch.bincount(levels[0]["agg"].to(torch.int64)).max()) == members
    gtail = hipk.MgGTail(levels, 2)
    rd = torch.from_numpy(np.random.default_rng([11, sizes[0]]).standard_normal(sizes[0]).astype(dtype)).to(DEV)
    omega, scale = 1.8, 0.37
    zb = hipk.mg_tail_apply(Mt._tail, omega, scale, rd, torch.full_like(rd, float("nan"))).cpu().numpy()
    zi = hipk.mg_gtail_apply(gtail, omega, scale, rd, torch.full_like(rd, float("nan"))).cpu().numpy()
    Ms.scale = scale
    zs = Ms(rd).cpu().numpy()
    assert Ms.omega == omega and np.isfinite(zs).all()
    assert MM.same_bits(zi, zb), f"{np.count_nonzero(MM.bits(zi) != MM.bits(zb))} of {zb.size} entries differ between the two tails"
    assert MM.same_bits(zb, zs), f"{np.count_nonzero(MM.bits(zb) != MM.bits(zs))} of {zs.size} entries differ from the launch sequence"
    assert MM.same_bits(zi, zs)


def test_rows_beyond_the_envelope_fall_back_to_launches(hipk, oracle):
    crow, col, val = MM.grid_matrix((12, 12), radius=3, full_box=True)
    assert np.diff(crow).max() == 49
    M = MG(MM.csr_tensor(crow, col, val, device=DEV), (12, 12), tail_rows=4096)
    assert M.tail_from is None and M.launches_per_apply == 4 * 9 + 1
    r = np.random.default_rng(2).standard_normal(144)
    assert MM.same_bits(M(torch.from_numpy(r).to(DEV)).cpu().numpy(), MM.apply(oracle, M, r))


# ------------------------------------------------------------------------------------------------------------ 3. the whole apply
@pytest.mark.parametrize("grid, levels", [((130, 70), [9100, 2275, 594, 153, 45, 15, 6, 2, 1]),
                                          ((300, 200), [60000, 15000, 3750, 950, 247, 70, 20, 6, 2, 1])],
                         ids=["130x70", "300x200"])
def test_whole_apply_is_the_mirror_at_every_tail_size(hipk, oracle, grid, levels):
    A = create_variable_diffusion_2d_csr(*grid, device=DEV)
    r = np.random.default_rng(17).standard_normal(A.shape[0])
    rd = torch.from_numpy(r).to(DEV)
    ref, scale = None, None
    for tail_rows in (0, 256, 1024, 4096):
        M = MG(A, grid, degree=2, tail_rows=tail_rows)
        assert [lev.n for lev in M.levels] == levels
        tail_from = next((l for l, n in enumerate(levels) if n <= tail_rows), None)
        assert M.tail_from == tail_from
        assert M.launches_per_apply == (len(levels) - 1 if tail_from is None else tail_from) * (2 * 2 + 7) + 1
        if ref is None:
            ref, scale = MM.apply(oracle, M, r), M.scale
        assert M.scale == scale
        z = M(rd).cpu().numpy()
        assert MM.same_bits(z, ref), f"tail_rows {tail_rows}: {np.count_nonzero(MM.bits(z) != MM.bits(ref))} entries differ from the mirror"
        assert MM.same_bits(M(rd).cpu().numpy(), ref), "the second apply differs from the first"
        assert M.applies == 2


def test_device_hierarchy_has_the_cpu_hierarchys_bits(hipk):
    A = create_variable_diffusion_2d_csr(130, 70)
    Mc, Md = MG(A, (130, 70), normalize=False), MG(A.to(DEV), (130, 70), normalize=False)
    for a, b in zip(Mc.levels, Md.levels):
        assert torch.equal(a.csr.crow_indices(), b.csr.crow_indices().cpu()) and torch.equal(a.csr.col_indices(), b.csr.col_indices().cpu())
        assert MM.same_bits(a.csr.values().numpy(), b.csr.values().cpu().numpy()) and MM.same_bits(a.dinv.numpy(), b.dinv.cpu().numpy())
        assert (a.c0, a.c1, a.c2) == (b.c0, b.c1, b.c2)
    with pytest.raises(ValueError, match="applied to"):
        Md(torch.ones(9100, dtype=torch.float64))
    with pytest.raises(ValueError, match="applied to"):
        Mc(torch.ones(9100, dtype=torch.float64, device=DEV))


# ------------------------------------------------------------------------------------------------------------ 4. whole solves
def _mirror_callable(oracle, M):
    def fn(v):
        return torch.from_numpy(MM.apply(oracle, M, v.cpu().numpy())).to(v.device)
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


@pytest.mark.parametrize("name, make, grid", [("vardiff130x70", create_variable_diffusion_2d_csr, (130, 70)), ("poisson96x40", create_poisson_2d_csr, (96, 40))])
def test_cg_solves_equal_the_mirror_driven_solves(hipk, oracle, name, make, grid):
    A = make(*grid, device=DEV)
    b = torch.ones(A.shape[0], dtype=torch.float64, device=DEV)
    M = MG(A, grid)
    x, info, st = _same_solve(cg, A, b, M, _mirror_callable(oracle, M), "cg_callable_M", tol=1e-6)
    relres = float(torch.linalg.vector_norm(b - A @ x) / torch.linalg.vector_norm(b))
    print(f"{name}: {st.iterations} iterations, relative residual {relres:.3e}")
    assert info == 0 and relres <= 1e-6 and M.applies >= st.iterations + 2      # the host queues iterations ahead of the stop word


def test_bicgstab_and_gmres_run_it_as_a_deterministic_left_preconditioner(hipk, oracle):
    grid = (48, 32)
    A = create_convdiff_2d_csr(*grid, device=DEV)
    b = torch.ones(A.shape[0], dtype=torch.float64, device=DEV)
    M = MG(A, grid)
    fn = _mirror_callable(oracle, M)
    _same_solve(bicgstab, A, b, M, fn, "bicgstab_callable_M", tol=1e-6)
    _same_solve(gmres, A, b, M, fn, "gmres_callable_M", tol=1e-6, restart=20)


# ------------------------------------------------------------------------------------------------------------ 5. a user-sized solve
def test_user_sized_cg_solve_takes_a_tenth_of_plain_cgs_iterations(hipk, oracle):
    grid = (500, 400)
    A = create_poisson_2d_csr(*grid, device=DEV)
    b = torch.ones(A.shape[0], dtype=torch.float64, device=DEV)
    x0, info0 = cg(A, b, tol=1e-6)
    plain = get_last_stats().iterations
    M = MG(A, grid)
    x, info = cg(A, b, tol=1e-6, M=M)
    its = get_last_stats().iterations
    oracle.set_threads(16)
    try:
        xm, infom = cg(A, b, tol=1e-6, M=_mirror_callable(oracle, M))
    finally:
        oracle.set_threads(1)
    print(f"500 x 400 Poisson: plain cg {plain} iterations, multigrid {its}, mirror-driven {get_last_stats().iterations}")
    assert info0 == 0 and info == 0 and infom == 0
    assert its == get_last_stats().iterations and MM.same_bits(x.cpu().numpy(), xm.cpu().numpy())
    assert 10 * its <= plain
