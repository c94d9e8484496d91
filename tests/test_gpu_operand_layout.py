"""Every Python entry takes its operands in any layout: a view that is contiguous but starts off a 16-byte boundary
(`buf[1:n + 1]`, a slab `state[n:2 * n]` with odd n), a strided view, a column of a row-major matrix, the other float type.
The C ABI refuses vectors that are not 16-byte aligned (HIPK_ERR_ALIGN, tested where the ABI is); the wrappers route every
operand through `_hipk.aligned`, which copies exactly the ones the library could not take.

`same_as_fresh`: the call with every operand a fresh tensor, then again with ONE operand in a layout of tests/_layout_cases.py;
the result's bytes, `info`, the bit patterns of the statistics and `hipk_last_solve_path` must be the same, the operand's whole
allocation (payload and sentinels) byte for byte what it was, and the result a contiguous tensor of its own.  Once per entry and
dtype the fresh arm is held against the CPU oracle, so "the same" means "the oracle's bits".  All comparisons are bitwise.

Without `_hipk.aligned` (the wrappers prepared operands with `.contiguous()`, which keeps a contiguous view where it starts) the
contiguous views off the boundary were refused with a HipkError naming the alignment -- nothing launched: b of every solver
with and without Jacobi (A, B), the result of a callable M under cg (C), b with a matrix-free A (D), CSR and coalesced-COO values
(E), the dispatcher's b, the residual's x, b and the gradient of cg_differentiable (I), a row block's b (J).  The strided, column
and dtype layouts, the callable M of bicgstab / gmres, the dense matrices, cg_multi / bicgstab_multi, the batch solves and the
Chebyshev and multigrid applies passed before as well and stay as pins.  Index views (E, G), `_block_solve` (F) and the
block-Jacobi apply (H) reach C entries that do not check those pointers: they are aligned copies now.

Systems: the smallest with an odd n at each partition the wrappers meet -- 7 x 5 (n = 35, one chunk), 293 x 7 (n = 2051, two
reduction chunks, the last one ragged), 131 x 127 (n = 16637, nine chunks: the one-launch loop of mid-size systems)."""
import json
import struct

import numpy as np
import pytest
import torch

import _layout_cases as lc
import _solve_runner as sr
from pytorch_sparse_solver.utils.matrix_utils import create_convdiff_2d_csr, create_poisson_2d_csr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64, F32 = torch.float64, torch.float32
DTN = {F64: "f64", F32: "f32"}
TOL = {F64: 1e-8, F32: 1e-5}
MAXITER = 50
GRIDS = {"n35": (7, 5), "n2051": (293, 7), "n16637": (131, 127), "n221": (17, 13)}
X0_LAYOUTS = ("off1", "slab", "stride2", "column")
SOLVERS = ("cg", "bicgstab", "gmres")

_systems = {}


def system(kind, size, dt):
    """(A on the device, its CSR arrays as numpy int32 / values): Poisson or convection-diffusion on GRIDS[size]; the entries of
    both are exact in fp32."""
    key = (kind, size, dt)
    if key not in _systems:
        nx, ny = GRIDS[size]
        A = (create_poisson_2d_csr if kind == "poisson" else create_convdiff_2d_csr)(nx, ny, dtype=dt)
        arrs = (A.crow_indices().numpy().astype(np.int32), A.col_indices().numpy().astype(np.int32), A.values().numpy())
        _systems[key] = (A.to(DEV), arrs)
    return _systems[key]


def kind_for(solver, size):
    return "convdiff" if solver != "cg" and size == "n35" else "poisson"


def solve_kw(solver, dt):
    kw = dict(tol=TOL[dt], maxiter=MAXITER)
    if solver == "gmres":
        kw["restart"] = 20
    return kw


def module_a():
    from pytorch_sparse_solver import module_a as m
    return m


class Obs:
    """What one call left behind: the result tensor, and (bytes of x, info, statistics bits, path) as `key`."""

    def __init__(self, x, info, stats, path, st=None):
        self.x, self.st, self.key = x, st, (x.detach().cpu().numpy().tobytes(), info, stats, path)


def observe(hipk, ret):
    """Of a single solve's `(x, info)`."""
    x, info = ret
    st = module_a().get_last_stats()
    return Obs(x, int(info), sr.stat_bits(st), hipk.last_solve_path(), st)


def observe_multi(hipk, ret):
    """Of cg_multi / bicgstab_multi / _block_solve: the statistics of every column."""
    X, info = ret
    st = module_a().get_last_stats()
    return Obs(X, tuple(int(i) for i in info), (b"".join(sr.stat_bits(c) for c in st.columns), st.block_spmvs), hipk.last_solve_path())


BATCH_FIELDS = ("iterations", "matvecs", "info", "breakdown", "b_norm", "residual_norm", "x_norm", "threshold", "recurrence_rs")


def observe_batch(hipk, ret):
    """Of cg_batch / bicgstab_batch / gmres_batch: the per-system lists, the route and the launches."""
    X, info = ret
    st = module_a().get_last_stats()
    bits = b"".join(struct.pack("<qqii5d", *(getattr(st, f)[s] for f in BATCH_FIELDS)) for s in range(len(st.info)))
    return Obs(X, tuple(int(i) for i in info), (bits, st.launches), st.path)


def same_as_fresh(hipk, call, values, operand, layout, obs=observe):
    """`call(**operands)` with every operand fresh, then with `operand` as a view in `layout`; returns the fresh arm's observation."""
    fresh = {k: None if v is None else lc.build("fresh", v, DEV)[0] for k, v in values.items()}
    base = obs(hipk, call(**fresh))
    placed = {operand: lc.build(layout, values[operand], DEV)}
    args = dict(fresh, **{name: p[0] for name, p in placed.items()})
    got = obs(hipk, call(**args))
    torch.cuda.synchronize()
    what = f"{operand} as {layout}"
    assert got.key[0] == base.key[0], f"{what}: other bits in the result"
    assert got.key[1:] == base.key[1:], f"{what}: info / statistics / path differ: {got.key[1:]} vs {base.key[1:]}"
    for name, (view, owner, snap) in placed.items():
        assert torch.equal(lc.owner_bytes(owner), snap), f"{name} as {layout}: the operand's allocation was written to"
        assert not lc.shares_storage(got.x, owner), f"{what}: the result lives in {name}'s allocation"
    assert got.x.is_contiguous() and all(t is None or not lc.shares_storage(got.x, t) for t in fresh.values())
    return base


def hold(obs, ref, what):
    """The fresh arm against an oracle result: the bits of x, iterations, info."""
    x, st = obs.x.cpu().numpy(), obs.st
    assert x.dtype == ref.x.dtype and np.array_equal(sr_bits(x), sr_bits(ref.x)), f"{what}: not the oracle's bits"
    assert (st.iterations, int(st.info)) == (ref.iterations, ref.info), (what, st.iterations, st.info, ref.iterations, ref.info)


def sr_bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def oracle_solve(oracle, solver, dt, arrs, b, dinv=None, x0=None):
    name = {"cg": "cg", "bicgstab": "bicgstab", "gmres": "gmres"}[solver] if dinv is None else \
        {"cg": "pcg_jacobi", "bicgstab": "bicgstab_jacobi", "gmres": "gmres_jacobi"}[solver]
    fn = getattr(oracle, name + ("32" if dt == F32 else ""))
    kw = dict(solve_kw(solver, dt), x0=x0)
    if solver == "gmres":
        kw["gpu_tolerances"] = True
    args = arrs + ((dinv,) if dinv is not None else ()) + (b,)
    return fn(*args, **kw)


def values_for(size, dt, x0=False):
    n = GRIDS[size][0] * GRIDS[size][1]
    return {"b": lc.payload(n, dt, 11), "x0": 0.125 * lc.payload(n, dt, 12) if x0 else None}


# ------------------------------------------------------------------------------------------- A. the three solvers, M = None
def _cases_a():
    for solver in SOLVERS:
        for dt in (F64, F32):
            for size in ("n35", "n2051"):
                for layout in lc.layouts_1d(dt)[1:]:
                    yield pytest.param(solver, dt, size, "b", layout, id=f"{solver}-{DTN[dt]}-{size}-b-{layout}")
                for layout in X0_LAYOUTS:
                    yield pytest.param(solver, dt, size, "x0", layout, id=f"{solver}-{DTN[dt]}-{size}-x0-{layout}")
    for dt in (F64, F32):
        for layout in lc.layouts_1d(dt)[1:]:
            yield pytest.param("cg", dt, "n16637", "b", layout, id=f"cg-{DTN[dt]}-n16637-b-{layout}")


@pytest.mark.parametrize("solver,dt,size,operand,layout", list(_cases_a()))
def test_a_plain_solves_take_b_and_x0_in_any_layout(hipk, solver, dt, size, operand, layout):
    A, _ = system(kind_for(solver, size), size, dt)
    fn = getattr(module_a(), solver)
    same_as_fresh(hipk, lambda b, x0: fn(A, b, x0, **solve_kw(solver, dt)), values_for(size, dt, operand == "x0"), operand, layout)


@pytest.mark.parametrize("dt", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("solver,size", [(s, z) for s in SOLVERS for z in ("n35", "n2051")] + [("cg", "n16637")])
def test_a_fresh_arm_is_the_oracle(hipk, oracle, solver, size, dt):
    A, arrs = system(kind_for(solver, size), size, dt)
    v = values_for(size, dt)
    got = observe(hipk, getattr(module_a(), solver)(A, v["b"].to(DEV), **solve_kw(solver, dt)))
    hold(got, oracle_solve(oracle, solver, dt, arrs, v["b"].numpy()), f"{solver} {size} {DTN[dt]}")


# ------------------------------------------------------------------------------------------- B. with JacobiPreconditioner
@pytest.mark.parametrize("layout", ["off1", "slab"])
@pytest.mark.parametrize("size", ["n35", "n2051"])
@pytest.mark.parametrize("dt", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("solver", SOLVERS)
def test_b_jacobi_solves_take_b_in_any_layout(hipk, oracle, solver, dt, size, layout):
    A, arrs = system(kind_for(solver, size), size, dt)
    J = module_a().JacobiPreconditioner(A)
    fn = getattr(module_a(), solver)
    v = values_for(size, dt)
    base = same_as_fresh(hipk, lambda b, x0: fn(A, b, x0, M=J, **solve_kw(solver, dt)), v, "b", layout)
    if layout == "off1":
        hold(base, oracle_solve(oracle, solver, dt, arrs, v["b"].numpy(), dinv=J.dinv.cpu().numpy()), f"{solver} jacobi {size}")


# ------------------------------------------------------------------------------------------- C. a callable M
class CallableM:
    """M(r) = dinv * r, returned in `kind`: "fresh" (the reference arm), a layout of _layout_cases (a new allocation per call),
    or "persistent_off1" / "persistent_aligned": ONE buffer of M's own, written and returned on every call."""

    def __init__(self, dinv, kind):
        self.dinv, self.kind, self.calls = dinv, kind, 0
        if kind.startswith("persistent"):
            n = dinv.numel()
            self.owner = lc._owner(2 * lc.GUARD + 1 + n, dinv, DEV, kind)
            k = 1 if kind == "persistent_off1" else 0
            self.view = self.owner[lc.GUARD + k:lc.GUARD + k + n]
            assert self.view.data_ptr() % 16 == (k * dinv.element_size()) % 16
            self.guards = (self.owner[:lc.GUARD].clone(), self.owner[lc.GUARD + k + n:].clone())

    def __call__(self, r):
        self.calls += 1
        z = self.dinv * r
        if self.kind == "fresh":
            return z
        if self.kind == "fresh_other":       # the reference arm of the `dtype` layout: the product in the other float type
            return z.to(lc.other_float(z.dtype))
        if self.kind.startswith("persistent"):
            self.view.copy_(z)
            return self.view
        return lc.build(self.kind, z, DEV, snapshot=False)[0]

    def check(self):
        if self.kind.startswith("persistent"):
            k = 1 if self.kind == "persistent_off1" else 0
            n = self.dinv.numel()
            assert torch.equal(self.owner[:lc.GUARD], self.guards[0]) and torch.equal(self.owner[lc.GUARD + k + n:], self.guards[1])


M_KINDS = ("off1", "stride2", "column", "dtype", "persistent_off1", "persistent_aligned")


@pytest.mark.parametrize("kind", M_KINDS)
@pytest.mark.parametrize("dt", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("solver", SOLVERS)
def test_c_callable_m_may_return_any_layout(hipk, solver, dt, kind):
    size = "n35" if kind in ("stride2", "column") else "n2051"
    A, _ = system(kind_for(solver, size), size, dt)
    dinv = module_a().JacobiPreconditioner(A).dinv
    fn = getattr(module_a(), solver)
    b = values_for(size, dt)["b"].to(DEV)
    ref_M = CallableM(dinv, "fresh_other" if kind == "dtype" else "fresh")
    base = observe(hipk, fn(A, b, M=ref_M, **solve_kw(solver, dt)))
    assert "callable_M" in module_a().get_last_stats().method
    M = CallableM(dinv, kind)
    got = observe(hipk, fn(A, b, M=M, **solve_kw(solver, dt)))
    torch.cuda.synchronize()
    # (the C loops read their stop word a batch late: how many applies follow convergence depends on timing, their results do not count)
    assert M.calls > 2 and ref_M.calls > 2
    assert got.key == base.key, f"M returning {kind}: the solve differs from the one with a fresh tensor"
    M.check()
    assert got.x.is_contiguous() and (not kind.startswith("persistent") or not lc.shares_storage(got.x, M.owner))


@pytest.mark.parametrize("solver", SOLVERS)
def test_c_fresh_arm_is_the_jacobi_oracle(hipk, oracle, solver):
    """M = (r -> dinv * r) as a callable: cg (the step API) and bicgstab (the C callback) give the Jacobi forms' bits; gmres
    applies M in roundings of its own, so its counts are the oracle's and x agrees to 1e-9 (the bound of the solve tables)."""
    size, dt = "n2051", F64
    A, arrs = system(kind_for(solver, size), size, dt)
    dinv = module_a().JacobiPreconditioner(A).dinv
    b = values_for(size, dt)["b"]
    got = observe(hipk, getattr(module_a(), solver)(A, b.to(DEV), M=CallableM(dinv, "fresh"), **solve_kw(solver, dt)))
    ref = oracle_solve(oracle, solver, dt, arrs, b.numpy(), dinv=dinv.cpu().numpy())
    if solver != "gmres":
        hold(got, ref, f"{solver} callable M")
    else:
        assert (got.st.iterations, int(got.st.info)) == (ref.iterations, ref.info)
        assert np.linalg.norm(got.x.cpu().numpy() - ref.x) <= 1e-9 * np.linalg.norm(ref.x)


# ------------------------------------------------------------------------------------------- D. a matrix-free A
@pytest.mark.parametrize("jacobi", [False, True], ids=["plain", "jacobi"])
@pytest.mark.parametrize("out", ["off1", "stride2"])
@pytest.mark.parametrize("op", ["spmv", "torch"])
@pytest.mark.parametrize("solver", SOLVERS)
def test_d_matrix_free_operator_may_return_any_layout(hipk, solver, op, out, jacobi):
    size, dt = ("n35" if out == "stride2" else "n2051"), F64
    A, _ = system(kind_for(solver, size), size, dt)
    h = hipk.handle_for(A)
    Ad = A.to_dense() if op == "torch" else None
    product = (lambda v: hipk.spmv(h, v)) if op == "spmv" else (lambda v: torch.mv(Ad, v))
    calls = {"fresh": 0, out: 0}

    def operator(kind):
        def apply(v):
            calls[kind] += 1
            y = product(v)
            return y if kind == "fresh" else lc.build(kind, y, DEV, snapshot=False)[0]
        return apply
    M = module_a().JacobiPreconditioner(A) if jacobi else None
    fn = getattr(module_a(), solver)
    vals = values_for(size, dt)
    base = observe(hipk, fn(operator("fresh"), vals["b"].to(DEV), M=M, **solve_kw(solver, dt)))
    assert "matrix_free" in module_a().get_last_stats().method
    b, owner, snap = lc.build("off1", vals["b"], DEV)
    got = observe(hipk, fn(operator(out), b, M=M, **solve_kw(solver, dt)))
    torch.cuda.synchronize()
    assert calls["fresh"] > 2 and calls[out] > 2
    assert got.key == base.key, f"A returning {out}, b as off1: the solve differs"
    assert torch.equal(lc.owner_bytes(owner), snap) and got.x.is_contiguous() and not lc.shares_storage(got.x, owner)


# ------------------------------------------------------------------------------------------- E. the matrix's own parts
def _parts(A):
    return A.crow_indices(), A.col_indices(), A.values()


def _matrix_variants(dt):
    for layout in ("off1", "slab") + (("off2", "off3") if dt == F32 else ()):
        yield f"csr-values-{layout}"
    for it in ("i64", "i32"):
        yield f"csr-indices-off1-{it}"
    yield "coo-values-off1"
    yield "dense-inner-block"
    yield "dense-flat-off1"


def _build_matrix(variant, A):
    """(the matrix with parts as views, the same matrix from cloned parts, [(owner, snapshot)])."""
    n = A.shape[0]
    crow, col, val = (t.cpu() for t in _parts(A))
    kept = []

    def view(layout, t):
        v, owner, snap = lc.build(layout, t, DEV)
        kept.append((owner, snap))
        return v
    if variant.startswith("csr-values-"):
        parts = (crow.to(DEV), col.to(DEV), view(variant.rsplit("-", 1)[1], val))
    elif variant.startswith("csr-indices-"):
        it = torch.int64 if variant.endswith("i64") else torch.int32
        parts = (view("off1", crow.to(it)), view("off1", col.to(it)), val.to(DEV))
    if variant.startswith("csr-"):
        mk = lambda p: torch.sparse_csr_tensor(*p, size=(n, n))
        V = mk(parts)
        assert all(a.data_ptr() == b.data_ptr() for a, b in zip(_parts(V), parts)), "torch copied a part: not the case meant"
        return V, mk(tuple(p.clone() for p in parts)), kept
    if variant == "coo-values-off1":
        rows = torch.repeat_interleave(torch.arange(n), crow[1:] - crow[:-1])
        idx = torch.stack([rows, col]).to(DEV)
        vals = view("off1", val)
        return (torch.sparse_coo_tensor(idx, vals, (n, n), is_coalesced=True), torch.sparse_coo_tensor(idx.clone(), vals.clone(), (n, n), is_coalesced=True), kept)
    dense = A.cpu().to_dense()
    if variant == "dense-inner-block":
        big = lc._sentinels((n + 2) * (n + 2), dense.dtype, variant).view(n + 2, n + 2).to(DEV)
        big[1:n + 1, 1:n + 1] = dense.to(DEV)
        kept.append((big, lc.owner_bytes(big)))
        V = big[1:n + 1, 1:n + 1]
        assert not V.is_contiguous()
    else:
        V = view("flat_off1", dense)
        assert V.is_contiguous() and V.data_ptr() % 16 != 0
    return V, V.clone(memory_format=torch.contiguous_format), kept


@pytest.mark.parametrize("variant,dt", [pytest.param(v, dt, id=f"{v}-{DTN[dt]}") for dt in (F64, F32) for v in _matrix_variants(dt)])
@pytest.mark.parametrize("solver", ["cg", "bicgstab"])
def test_e_matrix_parts_may_be_views(hipk, solver, variant, dt):
    hipk.clear_cache()
    A, _ = system(kind_for(solver, "n35"), "n35", dt)
    V, C, kept = _build_matrix(variant, A)
    h = hipk.handle_for(V)
    assert h.val.data_ptr() % 16 == 0 and h.val.is_contiguous() and h.n == 35
    assert hipk.handle_for(V) is h, "the second handle_for of the same tensor is not a cache hit"
    fn = getattr(module_a(), solver)
    b = values_for("n35", dt)["b"].to(DEV)
    base = observe(hipk, fn(C, b, **solve_kw(solver, dt)))
    got = observe(hipk, fn(V, b, **solve_kw(solver, dt)))
    torch.cuda.synchronize()
    assert got.key == base.key, f"{variant}: not the solve of the matrix built from cloned parts"
    assert hipk.handle_for(V) is h
    for owner, snap in kept:
        assert torch.equal(lc.owner_bytes(owner), snap), f"{variant}: a part's allocation was written to"
    hipk.clear_cache()


# ------------------------------------------------------------------------------------------- F. many right-hand sides
def _multi_call(entry, A, kw):
    from pytorch_sparse_solver.module_a import multi_rhs
    if entry.startswith("block_"):
        return lambda B, X0: multi_rhs._block_solve(entry[6:], A, B, X0, kw["tol"], 0.0, kw["maxiter"], None)
    return lambda B, X0: getattr(module_a(), entry)(A, B, X0, **kw)


@pytest.mark.parametrize("layout", ["flat_off1", "transposed"])
@pytest.mark.parametrize("operand", ["B", "X0"])
@pytest.mark.parametrize("size", ["n35", "n2051"])
@pytest.mark.parametrize("dt", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("entry", ["cg_multi", "bicgstab_multi", "block_cg", "block_bicgstab"])
def test_f_multi_rhs_take_b_and_x0_in_any_layout(hipk, oracle, entry, dt, size, operand, layout):
    solver = entry.replace("_multi", "").replace("block_", "")
    A, arrs = system(kind_for(solver, size), size, dt)
    n, k = A.shape[0], 3
    vals = {"B": lc.payload((n, k), dt, 21), "X0": 0.125 * lc.payload((n, k), dt, 22) if operand == "X0" else None}
    base = same_as_fresh(hipk, _multi_call(entry, A, solve_kw(solver, dt)), vals, operand, layout, obs=observe_multi)
    if entry.startswith("block_"):
        assert base.key[3] == f"hipk_{solver}_multi launch sequence", base.key[3]
    if (operand, layout) == ("B", "flat_off1"):            # once per entry, dtype and size: every column is the oracle's solve
        X = base.x.cpu().numpy()
        for j in range(k):
            ref = oracle_solve(oracle, solver, dt, arrs, np.ascontiguousarray(vals["B"].numpy()[:, j]))
            assert np.array_equal(sr_bits(np.ascontiguousarray(X[:, j])), sr_bits(ref.x)) and base.key[1][j] == ref.info, (entry, j)


# ------------------------------------------------------------------------------------------- G. batches of small systems
def _batch_values(solver, dt, S):
    """(crow, col, values (S, nnz)): the 7 x 5 system with the diagonal of system s raised by s / 4 (exact in fp32)."""
    A, _ = system(kind_for(solver, "n35"), "n35", dt)
    crow, col, val = (t.cpu() for t in _parts(A))
    rows = torch.repeat_interleave(torch.arange(35), crow[1:] - crow[:-1])
    vals = val.repeat(S, 1)
    vals[:, col == rows] += 0.25 * torch.arange(S, dtype=dt)[:, None]
    return crow, col, vals


def _batch_m(kind, A):
    m = module_a()
    return None if kind == "plain" else m.BatchedJacobiPreconditioner(A) if kind == "jacobi" else m.BatchedBlockJacobiPreconditioner(A, block_size=4)


@pytest.mark.parametrize("operand", ["B", "X0", "values"])
@pytest.mark.parametrize("pre", ["plain", "jacobi", "blockjacobi"])
@pytest.mark.parametrize("S", [8, 2])
@pytest.mark.parametrize("dt", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("solver", SOLVERS)
def test_g_batch_solves_take_operands_as_flat_off1(hipk, oracle, solver, dt, S, pre, operand):
    m = module_a()
    crow, col, vals = _batch_values(solver, dt, S)
    fn = getattr(m, solver + "_batch")
    kw = solve_kw(solver, dt)
    crow_d, col_d = crow.to(DEV), col.to(DEV)

    def call(B, X0, values):
        A = m.BatchedCSR(crow_d, col_d, values)
        return fn(A, B, X0, M=_batch_m(pre, A), **kw)
    v = {"B": lc.payload((S, 35), dt, 31), "X0": 0.125 * lc.payload((S, 35), dt, 32) if operand == "X0" else None, "values": vals}
    base = same_as_fresh(hipk, call, v, operand, "flat_off1", obs=observe_batch)
    kernel = S >= (m.batch.BJ_BATCH_MIN_SYSTEMS if pre == "blockjacobi" else m.batch.BATCH_MIN_SYSTEMS) and not (solver == "gmres" and pre == "blockjacobi")
    assert (base.key[3] != "loop") == kernel, (base.key[3], S, pre)
    if pre == "plain" and operand == "B":                  # once per entry, dtype and route: every system is the oracle's solve
        X = base.x.cpu().numpy()
        for s in range(S):
            arrs = (crow.numpy().astype(np.int32), col.numpy().astype(np.int32), vals[s].numpy())
            ref = oracle_solve(oracle, solver, dt, arrs, v["B"][s].numpy())
            assert np.array_equal(sr_bits(X[s]), sr_bits(ref.x)) and base.key[1][s] == ref.info, (solver, s)


@pytest.mark.parametrize("it", [torch.int64, torch.int32], ids=["i64", "i32"])
def test_g_batch_pattern_may_be_views(hipk, it):
    m = module_a()
    crow, col, vals = _batch_values("cg", F64, 8)
    B = lc.payload((8, 35), F64, 31).to(DEV)
    base = observe_batch(hipk, m.cg_batch(m.BatchedCSR(crow.to(it).to(DEV), col.to(it).to(DEV), vals.to(DEV)), B, tol=1e-8))
    (cv, co, cs), (lv, lo, ls) = lc.build("off1", crow.to(it), DEV), lc.build("off1", col.to(it), DEV)
    A = m.BatchedCSR(cv, lv, vals.to(DEV))
    assert A.crow32.data_ptr() % 16 == 0 and A.col32.data_ptr() % 16 == 0
    got = observe_batch(hipk, m.cg_batch(A, B, tol=1e-8))
    torch.cuda.synchronize()
    assert got.key == base.key and got.key[3] != "loop"
    assert torch.equal(lc.owner_bytes(co), cs) and torch.equal(lc.owner_bytes(lo), ls)


# ------------------------------------------------------------------------------------------- H. preconditioner applies
PRECONDITIONERS = ("jacobi", "blockjacobi", "chebyshev", "mg_grid", "mg_graph", "mg_graph_dense")
_pre = {}


def preconditioner(name, dt):
    if (name, dt) not in _pre:
        m = module_a()
        A, arrs = system("poisson", "n221", dt)
        MG = m.AggregationMultigridPreconditioner
        _pre[name, dt] = {"jacobi": lambda: m.JacobiPreconditioner(A), "blockjacobi": lambda: m.BlockJacobiPreconditioner(A, block_size=4),
                          "chebyshev": lambda: m.ChebyshevPreconditioner(A, degree=2), "mg_grid": lambda: MG(A, GRIDS["n221"]),
                          "mg_graph": lambda: MG.from_graph(A), "mg_graph_dense": lambda: MG.from_graph(A, coarse_rows=64)}[name]()
    return _pre[name, dt]


def _mirror_apply(oracle, name, dt, P, r):
    """The suite's CPU reference of each apply, on the object's own coefficients."""
    _, (crow, col, val) = system("poisson", "n221", dt)
    if name == "jacobi":
        return P.dinv.cpu().numpy() * r
    if name == "blockjacobi":
        return oracle.block_jacobi_apply(P.binv.cpu().numpy(), r) if dt == F64 else None
    if name == "chebyshev":
        from _cheb_mirror import mirror
        return mirror(oracle, crow, col, val, P, r, dtype=r.dtype.type)
    import _mg_dense_mirror as DM
    import _mg_graph_mirror as GM
    import _mg_mirror as MM
    return {"mg_grid": MM, "mg_graph": GM, "mg_graph_dense": DM}[name].apply(oracle, P, r)


@pytest.mark.parametrize("layout", ["off1", "slab", "stride2"])
@pytest.mark.parametrize("dt", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", PRECONDITIONERS)
def test_h_preconditioner_applies_take_v_in_any_layout(hipk, oracle, name, dt, layout):
    P = preconditioner(name, dt)
    values = lc.payload(221, dt, 41)
    want = P(values.to(DEV))
    v, owner, snap = lc.build(layout, values, DEV)
    z = P(v)
    torch.cuda.synchronize()
    assert z.dtype == want.dtype and torch.equal(z.view(torch.uint8), want.view(torch.uint8)), f"{name}: other bits for v as {layout}"
    assert torch.equal(lc.owner_bytes(owner), snap), f"{name}: v was written to"
    assert z.is_contiguous() and not lc.shares_storage(z, owner)
    if layout == "off1":
        ref = _mirror_apply(oracle, name, dt, P, values.numpy())
        if ref is not None:
            assert np.array_equal(sr_bits(want.cpu().numpy()), sr_bits(np.asarray(ref, dtype=values.numpy().dtype))), f"{name}: not the mirror's bits"


# ------------------------------------------------------------------------------------------- I. the dispatcher and autograd
@pytest.mark.parametrize("dt", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("solver", SOLVERS)
def test_i_dispatcher_takes_b_as_off1(hipk, solver, dt):
    import pytorch_sparse_solver as pss
    A, _ = system(kind_for(solver, "n2051"), "n2051", dt)
    rec = {}

    def call(b, x0):
        x, rec["r"] = pss.solve(A, b, method=solver, **solve_kw(solver, dt))
        return x, 0 if rec["r"].converged else -1
    same_as_fresh(hipk, call, values_for("n2051", dt), "b", "off1")
    assert rec["r"].backend == "module_a" and rec["r"].residual is not None


def test_i_relative_residual_takes_x_as_off1(hipk):
    from pytorch_sparse_solver.solver import SparseSolver
    A, _ = system("poisson", "n2051", F64)
    vals = values_for("n2051", F64)
    b = vals["b"].to(DEV)
    want = SparseSolver._relative_residual(A, b.clone(), b)
    x, owner, snap = lc.build("off1", vals["b"], DEV)
    assert SparseSolver._relative_residual(A, x, b) == want
    assert torch.equal(lc.owner_bytes(owner), snap)


@pytest.mark.parametrize("size", ["n35", "n2051"])
def test_i_differentiable_cg_takes_views_forward_and_backward(hipk, size):
    m = module_a()
    A, _ = system("poisson", size, F64)
    n = A.shape[0]
    vals, gvals = lc.payload(n, F64, 51), lc.payload(n, F64, 52)

    def run(b, g):
        b.requires_grad_(True)
        x = m.cg_differentiable(A, b, tol=1e-8, maxiter=MAXITER)
        x.backward(g)
        return x.detach().cpu().numpy().tobytes(), b.grad.detach().cpu().numpy().tobytes()
    base = run(vals.to(DEV), gvals.to(DEV))
    b_owner = lc._owner(2 * lc.GUARD + 1 + n, vals, DEV, "b")
    b_owner[lc.GUARD + 1:lc.GUARD + 1 + n] = vals.to(DEV)
    b_snap = lc.owner_bytes(b_owner)
    b = b_owner[lc.GUARD + 1:lc.GUARD + 1 + n].detach()        # a leaf that IS the off1 view
    g, g_owner, g_snap = lc.build("off1", gvals, DEV)
    assert b.data_ptr() % 16 == 8 and g.data_ptr() % 16 == 8
    got = run(b, g)
    torch.cuda.synchronize()
    assert got == base, "x or b.grad differ from the fresh arm's bits"
    assert torch.equal(lc.owner_bytes(b_owner), b_snap) and torch.equal(lc.owner_bytes(g_owner), g_snap)


# ------------------------------------------------------------------------------------------- J. the row-partitioned cg
def test_j_row_partitioned_cg_takes_b_local_as_off1(tmp_path):
    """World 1 through the worker of tests/test_dist_jacobi.py, with this rank's b an off1 view: what that file's tests assert of
    the run (the oracle's and the single-device solve's bits, twice), and the view's allocation untouched."""
    import test_dist_jacobi as tdj
    args = {"kind": "vardiff", "nx": 41, "ny": 37, "solver": "cg", "pmode": "local", "entry": "module_a", "tol": 1e-8, "maxiter": -1,
            "b_layout": "off1"}
    r = tdj._run(1, "hip", args, tmp_path)
    tdj._check(r)
    assert r["b_mod16"] == 8 and r["b_owner_unchanged"] is True, json.dumps({k: r[k] for k in ("b_mod16", "b_owner_unchanged")})
