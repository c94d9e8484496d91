"""The device side of AggregationMultigridPreconditioner.update, every comparison bitwise:

1. hipk_mg_level_scan between seeded guards around dinv, the results and the workspace, against the scalar loops of
   tests/_mg_refresh_mirror.py: n = 1, 2, 255, 256, 257, 2049 and 70 001 rows of 0, 1, 5, 32, 33 and 70 entries, a diagonal stored
   twice, unsorted rows, stored zeros, and -- in the "rough" flavour -- empty rows, rows without a diagonal, one negative diagonal and
   one NaN value; both dtypes, the bound on and off, a side stream, the workspace in the four states of tests/_arena.py with exactly
   hipk_mg_level_scan_work_bytes; every error code with nothing written;
2. the refresh plan through hipk_mg_restrict_agg reproduces _mg_graph_mirror.galerkin_agg on the shuffled, split-entry and
   stored-zero 17 x 13 matrices;
3. whole updates on the device are the CPU update -- level values, dinv, coefficients, cinv, scale -- on the grid class (33 x 31,
   9 x 7 x 5) and on graph hierarchies of 48 x 48 (tail_rows 0 and default; coarse_rows 64 and 600, whose dense levels of 30 and 221
   unknowns are the tail's last level, and 1024, whose 696 unknowns are outside the tail); the device apply after the update is the mirror apply; index arrays and work vectors are the objects they were;
4. cg / bicgstab / gmres with a refreshed object equal the same solves with the mirror as callable M, and a solve before the update
   leaves nothing behind: the solve after it is the new system's."""
import numpy as np
import pytest
import torch

import _mg_dense_mirror as DM
import _mg_graph_mirror as GM
import _mg_mirror as MM
import _mg_refresh_mirror as RM
from _arena import Arena, guard_bytes_for, run_states
from _order_cases import TRANSFORMS
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


def _arena(a, align=16):
    """An array between guards, exactly its bytes of payload."""
    ar = Arena(DEV, a.nbytes, align, guard_bytes_for(a.size, a.itemsize))
    return ar, ar.put(a)


# ------------------------------------------------------------------------------------------------------------ 1. the level scan
LENGTHS = (5, 0, 1, 32, 33, 70)


def _scan_level(n, dtype, flavour):
    """(crow, col, val) int32 / int32 / dtype.  "tame": every row has 1, 5, 32, 33 or 70 entries and a positive diagonal, some rows
    store it twice, columns in seeded order, stored zeros of both signs.  "rough": also empty rows and rows without a diagonal,
    one negative diagonal and one NaN."""
    rng = np.random.default_rng([31, n, flavour == "rough"])
    choices = [v for v in LENGTHS if v or flavour == "rough"]
    weight = np.array([8.0 if v in (1, 5) else 1.0 for v in choices])
    lens = rng.choice(choices, n, p=weight / weight.sum())
    lens[:min(n, len(choices))] = choices[:min(n, len(choices))]
    crow = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    nnz = int(crow[-1])
    col = rng.integers(0, n, nnz).astype(np.int32)
    val = rng.standard_normal(nnz)
    val[rng.random(nnz) < 0.05] = 0.0
    val[rng.random(nnz) < 0.02] = -0.0
    for i in np.flatnonzero(lens):
        lo, hi = int(crow[i]), int(crow[i + 1])
        if flavour == "rough" and i % 11 == 10:
            continue                                              # left as drawn: most of these rows have no diagonal entry
        on = col[lo:hi] == i
        val[lo:hi][on] = 0.25 + np.abs(val[lo:hi][on])
        k = lo + int(rng.integers(0, hi - lo))                    # the diagonal at a seeded place of the row
        col[k], val[k] = i, 4.0 + abs(val[k])
        if hi - lo >= 5 and i % 3 == 0:                           # ... and a second time
            k2 = lo + int(rng.integers(0, hi - lo))
            col[k2], val[k2] = i, 0.5 + abs(val[k2])
    if flavour == "rough":
        i = int(np.flatnonzero(lens == 1)[-1]) if (lens == 1).any() else 0
        val[crow[i]:crow[i + 1]][col[crow[i]:crow[i + 1]] == i] *= -1.0       # one negative diagonal
        if n > 2:
            val[int(crow[n // 2 + 1]) - 1 if lens[n // 2] else 0] = np.nan
    return crow, col, val.astype(dtype)


_scan_refs = {}


def _scan_ref(n, dtype, flavour):
    key = (n, np.dtype(dtype).name, flavour)
    if key not in _scan_refs:
        arrs = _scan_level(n, dtype, flavour)
        _scan_refs[key] = (arrs, RM.level_scan(*arrs, want_lmax=True))
    return _scan_refs[key]


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
@pytest.mark.parametrize("flavour", ["tame", "rough"])
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 2049, 70001])
def test_level_scan_has_the_mirrors_bits_between_guards(hipk, n, flavour, dtype):
    (crow, col, val), (dinv, lmax, bad) = _scan_ref(n, dtype, flavour)
    if flavour == "tame":
        assert bad == 0 and np.isfinite(lmax) and np.isfinite(dinv).all()
    elif n >= 255:
        assert bad > 2 and np.isnan(lmax) and (np.diff(crow) == 0).any() and np.isinf(dinv).any() and (dinv < 0).any()
    if n >= 255:
        assert set(np.diff(crow)) == {v for v in LENGTHS if v or flavour == "rough"}
    wb = hipk.mg_level_scan_work_bytes(n)
    assert wb == 16 * ((n + 2047) // 2048)
    ro = {}
    for name, a in (("crow", crow), ("col", col), ("val", val)):
        ro[name] = _arena(a)
    d_ar, d_d = _arena(np.zeros(n, dtype=dtype))
    o_ar, o_d = _arena(np.zeros(2))
    work = Arena(DEV, wb, 16, guard_bytes_for(n, 8))
    side = torch.cuda.Stream(device=DEV)

    def run(i, want=True):
        d_d.fill_(float("nan"))
        o_d.fill_(-7.0)
        torch.cuda.synchronize()
        with torch.cuda.stream(side if i % 2 else torch.cuda.current_stream(DEV)):
            hipk.mg_level_scan(ro["crow"][1], ro["col"][1], ro["val"][1], want, d_d, o_d, work.payload)
        torch.cuda.synchronize()
        return {"dinv": d_d.cpu().numpy().tobytes(), "out": o_d.cpu().numpy().tobytes()}

    guarded = {"dinv": d_ar, "out": o_ar, **{k: v[0] for k, v in ro.items()}}
    res = run_states(work, guarded, {k: v[0] for k, v in ro.items()}, run, label=f"hipk_mg_level_scan n = {n} {flavour}")
    got = np.frombuffer(res[0]["dinv"], dtype=dtype)
    assert DM.same_bits(got, dinv), f"{np.count_nonzero(DM.bits(got) != DM.bits(dinv))} of {n} entries of dinv differ"
    out = np.frombuffer(res[0]["out"])
    print(f"n = {n} {flavour}: lmax {out[0]} (mirror {lmax}), {out[1]} non-positive diagonal entries (mirror {bad})")
    assert (np.isnan(lmax) and np.isnan(out[0])) or out[0] == lmax
    assert out[1] == bad
    off = run_states(work, guarded, {k: v[0] for k, v in ro.items()}, lambda i: run(i, want=False), label=f"hipk_mg_level_scan n = {n}, no bound")
    assert off[0]["dinv"] == res[0]["dinv"] and np.array_equal(np.frombuffer(off[0]["out"]), [0.0, bad])


def test_level_scan_error_codes_write_nothing(hipk):
    L = hipk.lib()
    n = 300
    crow, col, val = _scan_level(n, np.float64, "tame")
    crow_d, col_d, val_d = (torch.from_numpy(a).to(DEV) for a in (crow, col, val))
    dinv = torch.full((n + 2,), 7.0, dtype=torch.float64, device=DEV)
    out = torch.full((4,), 7.0, dtype=torch.float64, device=DEV)
    wb = hipk.mg_level_scan_work_bytes(n)
    work = torch.full((wb + 64,), 0x5A, dtype=torch.uint8, device=DEV)
    assert wb == 16 and L.hipk_mg_level_scan_work_bytes(0) == 0 and L.hipk_mg_level_scan_work_bytes(2 ** 31) == 0
    assert L.hipk_mg_level_scan_work_bytes(2 ** 31 - 1) == 16 * 2048 and L.hipk_mg_level_scan_work_bytes(-3) == 0
    p = lambda x: x.data_ptr()

    def call(n=n, crow=p(crow_d), col=p(col_d), val=p(val_d), dtype=1, want=1, dinv=p(dinv), out=p(out), work=p(work), wb=wb):
        return L.hipk_mg_level_scan(n, crow, col, val, dtype, want, dinv, out, work, wb, None)

    for name in ("crow", "col", "val", "dinv", "out", "work"):
        assert call(**{name: None}) == ARG, name
    assert call(n=0) == ARG and call(n=-1) == ARG and call(n=2 ** 31) == ARG
    assert call(want=2) == ARG and call(want=-1) == ARG
    assert call(dinv=p(val_d)) == ARG                               # val == dinv
    assert call(dtype=7) == UNSUPPORTED and call(dtype=-1) == UNSUPPORTED
    for name, t, step in (("crow", crow_d, 4), ("col", col_d, 4), ("val", val_d, 8), ("dinv", dinv, 8), ("out", out, 8), ("work", work, 8)):
        assert call(**{name: p(t) + step}) == ALIGN, name
    assert call(wb=wb - 1) == WORKSPACE and call(wb=0) == WORKSPACE
    torch.cuda.synchronize()
    assert bool((dinv == 7.0).all()) and bool((out == 7.0).all()) and bool((work == 0x5A).all())
    assert call() == 0 and call(dtype=1, want=0, out=p(out) + 16) == 0
    torch.cuda.synchronize()
    ref = RM.level_scan(crow, col, val)
    assert DM.same_bits(dinv[:n].cpu().numpy(), ref[0]) and bool((dinv[n:] == 7.0).all())
    assert out.cpu().tolist() == [ref[1], 0.0, 0.0, 0.0] and bool((work[wb:] == 0x5A).all())
    with pytest.raises(AssertionError, match="crow"):
        hipk.mg_level_scan(crow_d[:-1], col_d, val_d, True, dinv[:n], out[:2], work)


# ------------------------------------------------------------------------------------------------------------ 2. the plan's sums
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
@pytest.mark.parametrize("transform", ["shuf", "dup", "zero"])
def test_the_plan_through_restrict_agg_is_the_mirrors_galerkin_sum(hipk, transform, dtype):
    crow, col, val = TRANSFORMS[transform](*_np(create_poisson_2d_csr(17, 13)), seed=5)
    val = (val * np.random.default_rng(4).uniform(0.5, 2.0, len(val))).astype(dtype)      # sums that depend on their order
    M = MG.from_graph(MM.csr_tensor(crow, col, val, device=DEV), normalize=False)
    Mc = MG.from_graph(MM.csr_tensor(crow, col, val), normalize=False)
    plan, plan_c = M._refresh_plan(), Mc._refresh_plan()
    assert len(plan["steps"]) == len(M.levels) - 1 >= 2 and M.refresh_plan_bytes > 0
    arrs = (crow, col, val)
    for l, (step, step_c) in enumerate(zip(plan["steps"], plan_c["steps"])):
        nnz, nnz_next = M.levels[l].csr.values().numel(), M.levels[l + 1].csr.values().numel()
        assert step["gsrc"].dtype == step["gptr"].dtype == torch.int32 and step["gsrc"].is_cuda
        assert step_c["gsrc"].dtype == step_c["gptr"].dtype == torch.int64
        assert step["gsrc"].numel() == nnz and step["gptr"].numel() == nnz_next + 1
        assert torch.equal(step["gsrc"].cpu().long(), step_c["gsrc"]) and torch.equal(step["gptr"].cpu().long(), step_c["gptr"])
        ref = GM.galerkin_agg(*arrs, M.levels[l].agg.cpu().numpy(), M.levels[l + 1].n)
        out = torch.full((nnz_next,), float("nan"), dtype=M.dtype, device=DEV)
        hipk.mg_restrict_agg(step["gptr"], step["gsrc"], torch.from_numpy(arrs[2]).to(DEV), out)
        assert DM.same_bits(out.cpu().numpy(), ref[2]), f"level {l + 1}"
        arrs = ref


# ------------------------------------------------------------------------------------------------------------ 3. whole updates
def _system(name, dtype):
    """(grid or None, the arrays the object is built from, other values on the same pattern)."""
    if name == "grid33x31":
        grid, a, b = (33, 31), _np(create_poisson_2d_csr(33, 31)), _np(create_variable_diffusion_2d_csr(33, 31, contrast=3.0, seed=7))
    elif name == "grid9x7x5":
        grid, a, b = (9, 7, 5), MM.grid_matrix((9, 7, 5)), MM.grid_matrix((9, 7, 5), seed=3)
    else:
        grid, a, b = None, _np(create_poisson_2d_csr(48, 48)), _np(create_variable_diffusion_2d_csr(48, 48, contrast=3.0, seed=7))
    assert RM.same_pattern(a, b)
    return grid, (a[0], a[1], a[2].astype(dtype)), (b[0], b[1], b[2].astype(dtype))


# name -> (system, constructor keywords)
HIERARCHIES = {"grid33x31": ("grid33x31", {}), "grid9x7x5": ("grid9x7x5", {}), "graph48_no_tail": ("graph48", {"tail_rows": 0}),
               "graph48": ("graph48", {}), "graph48_dense64": ("graph48", {"coarse_rows": 64}), "graph48_dense600": ("graph48", {"coarse_rows": 600}),
               "graph48_dense1024": ("graph48", {"coarse_rows": 1024})}


def _build(name, arrs, grid, device, **more):
    kw = dict(HIERARCHIES[name][1], **more)
    A = MM.csr_tensor(*arrs, device=device)
    return MG(A, grid, **kw) if grid is not None else MG.from_graph(A, **kw)


def _same_numbers(Mc, Md):
    assert len(Mc.levels) == len(Md.levels) and Mc.scale == Md.scale
    for l, (a, b) in enumerate(zip(Mc.levels, Md.levels)):
        assert torch.equal(a.csr.crow_indices(), b.csr.crow_indices().cpu()) and torch.equal(a.csr.col_indices(), b.csr.col_indices().cpu())
        assert DM.same_bits(a.csr.values().numpy(), b.csr.values().cpu().numpy()), f"level {l}: values"
        assert (a.c0, a.c1, a.c2) == (b.c0, b.c1, b.c2), f"level {l}: coefficients"
        for x, y, what in ((a.dinv, b.dinv, "dinv"), (a.cinv, b.cinv, "cinv")):
            assert (x is None) == (y is None) and (x is None or DM.same_bits(x.numpy(), y.cpu().numpy())), f"level {l}: {what}"


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
@pytest.mark.parametrize("name", list(HIERARCHIES))
def test_device_update_is_the_cpu_update_and_the_apply_is_the_mirrors(hipk, oracle, name, dtype):
    grid, first, other = _system(HIERARCHIES[name][0], dtype)
    Mc, Md = _build(name, first, grid, "cpu", degree=2), _build(name, first, grid, DEV, degree=2)
    n = Md.shape[0]
    if name in ("graph48_dense64", "graph48_dense600"):        # levels 2304, 696, 221, 77, 30: the dense level is the tail's last one
        assert Md.dense and Md.tail_from == 1 and Md.levels[-1].n == (30 if name == "graph48_dense64" else 221)
    if name == "graph48_dense1024":                               # 696 unknowns: above the tail's 512, a launch of its own
        assert Md.dense and Md.tail_from is None and Md.levels[-1].n == 696
    if name == "graph48_no_tail":
        assert Md.tail_from is None and not Md.dense
    r = np.random.default_rng(5).standard_normal(n).astype(dtype)
    rd = torch.from_numpy(r).to(DEV)
    Md(rd)
    kept = dict(Md._keep)
    assert kept and Md.refresh_plan_bytes == 0
    B = MM.csr_tensor(*other, device=DEV)
    assert Md.update(B) is Md and Mc.update(MM.csr_tensor(*other)) is Mc
    assert Md.updates == 1 and Md.applies == 0 and Md.refresh_plan_bytes > 0
    _same_numbers(Mc, Md)
    assert all(Md._keep[k] is v for k, v in kept.items()), "an index array or work vector was rebuilt"
    assert all(lev.csr.values().is_cuda and (lev.dinv is None or lev.dinv.is_cuda) for lev in Md.levels)
    z = Md(rd).cpu().numpy()
    ref = DM.apply(oracle, Md, r) if Md.graph else MM.apply(oracle, Md, r)
    assert DM.same_bits(z, ref), f"{np.count_nonzero(DM.bits(z) != DM.bits(ref))} of {n} entries of the apply differ from the mirror"
    assert DM.same_bits(Mc(torch.from_numpy(r)).numpy(), ref)
    if grid is not None:                                           # the boxes do not depend on the values: the fresh object
        _same_numbers(_build(name, other, grid, "cpu", degree=2), Md)
    Md.update(MM.csr_tensor(*first, device=DEV))                   # and back, on the plan alone
    _same_numbers(_build(name, first, grid, "cpu", degree=2), Md)
    assert Md.updates == 2


def test_device_update_errors_leave_the_object_as_it_was(hipk):
    grid, first, other = _system("graph48", np.float64)
    M = _build("graph48_dense64", first, grid, DEV)
    M.update(MM.csr_tensor(*other, device=DEV))
    r = torch.from_numpy(np.random.default_rng(6).standard_normal(M.shape[0])).to(DEV)
    z0 = M(r).clone()
    crow, col, val = other
    negated = val.copy()
    negated[int(np.flatnonzero(col[crow[70]:crow[71]] == 70)[0]) + int(crow[70])] *= -1.0
    for A_new, match in ((MM.csr_tensor(crow, col, negated, device=DEV), r"level 0 \(2304\): zero or negative entry on the diagonal"),
                         (MM.csr_tensor(*other), "cpu"), (MM.csr_tensor(crow, col, val.astype(np.float32), device=DEV), "float32"),
                         (create_poisson_2d_csr(47, 48, device=DEV), "shape"),
                         (MM.csr_tensor(*TRANSFORMS["zero"](crow, col, val, seed=1), device=DEV), "pattern")):
        with pytest.raises(ValueError, match=match):
            M.update(A_new)
        assert M.updates == 1 and torch.equal(M(r), z0)
    Mc = _build("graph48_dense64", first, grid, "cpu")
    with pytest.raises(ValueError, match="cuda"):
        Mc.update(MM.csr_tensor(*other, device=DEV))


# ------------------------------------------------------------------------------------------------------------ 4. whole solves
def _mirror_callable(oracle, M):
    apply = DM.apply if M.graph else MM.apply

    def fn(v):
        return torch.from_numpy(apply(oracle, M, v.cpu().numpy())).to(v.device)
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


@pytest.mark.parametrize("name", ["grid33x31", "graph48", "graph48_dense600", "graph48_dense1024"])
def test_cg_before_and_after_an_update_solves_the_new_system(hipk, oracle, name):
    """A solve with the object, then `update`, then a solve: no stale handle, descriptor or cached tail survives."""
    grid, first, other = _system(HIERARCHIES[name][0], np.float64)
    A, B = MM.csr_tensor(*first, device=DEV), MM.csr_tensor(*other, device=DEV)
    b = torch.ones(A.shape[0], dtype=torch.float64, device=DEV)
    M = _build(name, first, grid, DEV)
    x0, info0 = cg(A, b, tol=1e-6, M=M)
    assert info0 == 0
    M.update(B)
    x, info, st = _same_solve(cg, B, b, M, _mirror_callable(oracle, M), "cg_callable_M", tol=1e-6)
    relres = float(torch.linalg.vector_norm(b - B @ x) / torch.linalg.vector_norm(b))
    print(f"{name}: {len(M.levels)} levels, {st.iterations} iterations after the update, relative residual {relres:.3e}")
    assert info == 0 and relres <= 1e-6
    N = _build(name, first, grid, DEV, normalize=False)            # never applied before its update
    N.update(B)
    N.scale = M.scale
    xn, _ = cg(B, b, tol=1e-6, M=N)
    assert DM.same_bits(x.cpu().numpy(), xn.cpu().numpy())


def test_bicgstab_and_gmres_with_a_refreshed_object_equal_the_mirror_driven_solves(hipk, oracle):
    A = create_convdiff_2d_csr(48, 32, device=DEV)
    crow, col, val = _np(A)
    rows = np.repeat(np.arange(len(crow) - 1), np.diff(crow))
    other = val * (1.0 + 0.3 * np.sin(rows))                       # the same pattern, every row scaled by up to 30 %
    B = MM.csr_tensor(crow, col, other, device=DEV)
    b = torch.ones(A.shape[0], dtype=torch.float64, device=DEV)
    M = MG.from_graph(A, coarse_rows=256)
    bicgstab(A, b, tol=1e-6, M=M, maxiter=100)
    M.update(B)
    fn = _mirror_callable(oracle, M)
    # (on CPU tensors these take 10 iterations and one cycle; maxiter keeps a regression from running the mirror for minutes)
    x, info, st = _same_solve(bicgstab, B, b, M, fn, "bicgstab_callable_M", tol=1e-6, maxiter=100)
    assert info == 0
    x, info, st = _same_solve(gmres, B, b, M, fn, "gmres_callable_M", tol=1e-6, restart=20, maxiter=20)
    assert info == 0
