"""Unsorted and duplicate CSR rows on a single-device handle: every SpMV kernel family, every solve form family, the Chebyshev
epilogue kernels, the transpose and the Python surface, each pinned bit for bit to the CPU oracle run on the SAME arrays.

include/hipk.h (hipk_csr_create) promises that a row is summed in stored order whatever the order and multiplicity of its
columns; DESIGN.md 7 rests the rank-count invariance of the row-partitioned solves on it.  The case tables are
tests/_order_cases.py (transformations rev, diag_first, shuf, dup, dup_diag, dup_shuf, zero of the sorted matrices of the other
case tables); tests/test_order_cases.py checks them without a GPU.

  SpMV sweep   per case hipk_spmv_ex in all eight modes and with w == x: the literal kernel note, y and the fused-dot chunk
               partials with the oracle's bits, inputs unchanged, the same bits on the plain CSR kernels; the oracle itself within
               the derived bound of a long-double reference (gamma_L sum |a x|; residual form gamma_(L+1) (|b| + sum |a x|));
               six cases again with int32 indices; switches read once per process in a child (tests/_spmv_inst_worker.py).
  solver sweep one case per form family under rev and dup_shuf, the duplicate on each guard edge it moves: literal path and form,
               x, info, iterations, matvecs, breakdown and recurrence_rs equal to the oracle's (callback-M GMRES as
               tests/test_gpu_pcg.py compares it: its ||M(.)||^2 is a chunked dot, the oracle's a tiled one).
  Chebyshev    hipk_cheb_apply at degree 3 against tests/_cheb_mirror.py on the same arrays, with the expected note.
  transpose    CsrHandle.transposed() equals a numpy stable sort by column (duplicates keep their source order).
  Python       cg / bicgstab / gmres on torch.sparse_csr_tensor(crow, col, val) of such arrays: handle_for neither sorts nor
               coalesces; Jacobi, Chebyshev and block-Jacobi preconditioners add duplicate diagonal entries.

Every comparison is bitwise or uses a bound derived where it stands."""
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

import _cheb_cases as CC
import _order_cases as OC
import _spmv_cases as S
from _cheb_mirror import mirror
from _oracle_cases import _check_stats_long_double
from _spmv_inst_worker import OnDevice, References, differs, run_case
from test_order_cases import high_precision_worst

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_spmv_inst_worker.py")
CHILD_SECONDS = 300


def _reported(notes=(), forms=()):
    """No kernel template or form family of _order_cases.UNREACHABLE_UNSORTED (empty today) is ever reported."""
    got = OC.spmv_templates(notes) | {OC.form_family(f) for f in forms}
    assert not got & set(OC.UNREACHABLE_UNSORTED), got & set(OC.UNREACHABLE_UNSORTED)


# ---------------------------------------------------------------------------------------------- SpMV sweep
_held = {}


def _references(hipk, oracle, case):
    key = (case["matrix"], case["transform"], case["dtype"])
    if key not in _held:
        if OC.base_rows(key[0]) > S.N_SMALL:
            for k in [k for k in _held if OC.base_rows(k[0]) > S.N_SMALL]:
                del _held[k]
        crow, col, val = OC.arrays(*key)
        ref = References(oracle, key[0], key[2], int(hipk.lib().hipk_chunk_size(len(crow) - 1)), arrays=(crow, col, val),
                         vectors=OC.vectors(key[0], key[2]))
        oracle_worst = high_precision_worst(ref.crow, ref.col, ref.val, ref.x, ref.b, ref.y[False], ref.y[True],
                                            2.0 ** -53 if key[2] == OC.DOUBLE else 2.0 ** -24)
        print(f"{key}: oracle against np.longdouble, largest error / bound {oracle_worst:.3f}", flush=True)
        assert 0.0 < oracle_worst <= 1.0
        _held[key] = (ref, OnDevice(ref))
    return _held[key]


IN_PROCESS = sorted((n for n, c in OC.SPMV.items() if c["fresh"] is None),
                    key=lambda n: (OC.SPMV[n]["matrix"], OC.SPMV[n]["transform"], OC.SPMV[n]["dtype"], n))


@pytest.mark.parametrize("name", IN_PROCESS)
def test_spmv_on_unsorted_or_duplicate_rows(hipk, oracle, monkeypatch, name):
    case = OC.SPMV[name]
    ref, dev = _references(hipk, oracle, case)

    def setenv(k, v):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)

    notes, failures = run_case(hipk, name, ref, dev, setenv, case=case)
    print(name, sorted({n[3] for n in notes}), flush=True)
    _reported(notes={n[3] for n in notes})
    assert not failures, "\n".join(failures)
    assert len(notes) == len(case["runs"])


@pytest.mark.parametrize("group", OC.FRESH_GROUPS)
def test_spmv_fresh_process_group(hipk, tmp_path, group):
    """One child per setting of a switch the library reads once per process; never retried."""
    _held.clear()
    names = sorted(n for n, c in OC.SPMV.items() if c["fresh"] == group)
    out = str(tmp_path / "result.json")
    try:
        p = subprocess.run([sys.executable, WORKER, "order:" + group, out] + names, capture_output=True, text=True, timeout=CHILD_SECONDS)
    except subprocess.TimeoutExpired as e:
        pytest.fail(f"group {group}: the child did not finish in {CHILD_SECONDS} s\n{(e.stdout or b'')[-2000:]}\n{(e.stderr or b'')[-4000:]}")
    assert p.returncode == 0, f"group {group}: exit status {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}"
    with open(out) as f:
        results = json.load(f)
    failures = []
    for name in names:
        assert name in results, f"group {group}: no result for {name}\n{p.stdout[-2000:]}"
        case, r = OC.SPMV[name], results[name]
        failures += r["failures"]
        want = [[si, mode, wx, notes[mode]] for si, (_, notes) in enumerate(case["steps"]) for mode, wx in case["runs"]]
        if r["notes"] != want:
            failures.append(f"{name}: notes {r['notes']}, expected {want}")
        _reported(notes={n[3] for n in r["notes"]})
        print(name, sorted({n[3] for n in r["notes"]}), flush=True)
    assert not failures, "\n".join(failures)


# ---------------------------------------------------------------------------------------------- solver sweep
ORACLE = {"cg": "cg", "pcg": "pcg_jacobi", "bicgstab": "bicgstab", "pbicgstab": "bicgstab_jacobi", "gmres": "gmres", "pgmres": "gmres_jacobi"}
_built = {}
SOLVE_RUNS = [(c, False) for c in OC.SOLVES] + [(c, True) for c in OC.SOLVES if c[0] in OC.SOLVES_I32]


def _solver_arrays(key, transform, dt):
    if (key, transform, dt) not in _built:
        _built[(key, transform, dt)] = OC.solver_matrix(key, transform, dt)
    return _built[(key, transform, dt)]


@pytest.mark.parametrize("case, idx32", SOLVE_RUNS, ids=[c[0] + ("-i32" if i else "") for c, i in SOLVE_RUNS])
def test_solver_form_on_unsorted_or_duplicate_rows(hipk, oracle, monkeypatch, case, idx32):
    import scipy.sparse as sp
    cid, solver, key, transform, dtn, kw, env, x0kind, path, form = case
    dt = np.float64 if dtn == OC.F64 else np.float32
    for k, v in env.items():     # before the handle exists
        monkeypatch.setenv(k, v)
    crow, col, val = _solver_arrays(key, transform, dt)
    n = len(crow) - 1
    it = torch.int32 if idx32 else torch.int64
    h = hipk.CsrHandle(torch.from_numpy(crow).to(DEV).to(it), torch.from_numpy(col).to(DEV).to(it), torch.from_numpy(val).to(DEV), (n, n))
    try:
        rng = np.random.default_rng(zlib.crc32(cid.encode()))
        x0 = rng.standard_normal(n).astype(dt) if x0kind == "rand" else None
        b = rng.standard_normal(n).astype(dt)
        pre = solver in ("pcg", "pbicgstab", "pgmres")
        callback = bool(kw.get("callback"))
        dinv = None
        if pre:      # the stored diagonal entries of a row add (two of them at the most: one rounding), then the reciprocal
            diag = np.zeros(n, dtype=np.float64)
            on = col == OC._rows(crow)
            np.add.at(diag, col[on], val[on].astype(np.float64))
            dinv = (1.0 / diag.astype(dt).astype(np.float64)).astype(dt)
        bd = torch.from_numpy(b).to(DEV)
        xd = torch.zeros_like(bd) if x0 is None else torch.from_numpy(x0).to(DEV)
        dd = torch.from_numpy(dinv).to(DEV) if pre else None
        gkw = {k: v for k, v in kw.items() if k in ("restart", "solve_method")}
        print("entry order solver case", cid, flush=True)
        if callback and solver == "pbicgstab":
            st = hipk.solve_bicgstab_callable(h, lambda v: dd * v, bd, xd, tol=kw["tol"], atol=0.0, maxiter=kw["maxiter"])
        elif callback:
            st = hipk.solve_gmres_callable(h, lambda v: dd * v, bd, xd, tol=kw["tol"], atol=0.0, maxiter=kw["maxiter"], **gkw)
        elif not pre:
            st = hipk.solve(solver, h, bd, xd, tol=kw["tol"], atol=0.0, maxiter=kw["maxiter"], **gkw)
        elif solver == "pgmres":
            st = hipk.solve_pgmres(h, dd, bd, xd, tol=kw["tol"], atol=0.0, maxiter=kw["maxiter"], **gkw)
        else:
            st = hipk.solve_pcg(h, dd, bd, xd, tol=kw["tol"], atol=0.0, maxiter=kw["maxiter"], method={"pcg": "cg", "pbicgstab": "bicgstab"}[solver])
        got_path, got_form = hipk.last_solve_path(), hipk.last_solve_form()
        x = xd.cpu().numpy()
    finally:
        h.close()
    _reported(forms=[got_form])
    assert got_path == path, (cid, got_path, got_form)
    assert got_form == form, (cid, got_form)
    assert np.array_equal(bd.cpu().numpy(), b), cid

    fn = getattr(oracle, ORACLE[solver] + ("32" if dt == np.float32 else ""))
    args = (crow, col, val) + ((dinv,) if pre else ()) + (b,)
    okw = dict(x0=x0, tol=kw["tol"], atol=0.0, maxiter=kw["maxiter"])
    if solver in ("gmres", "pgmres"):
        okw.update(gkw, gpu_tolerances=True)
    oracle.set_threads(4 if n >= 10_000 else 1)
    try:
        ref = fn(*args, **okw)
    finally:
        oracle.set_threads(1)
    print("  iterations", st.iterations, "matvecs", st.matvecs, "info", st.info, "breakdown", st.breakdown, "| oracle", ref.iterations,
          ref.matvecs, ref.info, ref.breakdown, flush=True)
    assert ref.matvecs > 1, cid          # the loop ran
    if callback and solver == "pgmres":
        assert (st.iterations, st.matvecs, st.info) == (ref.iterations, ref.matvecs, ref.info), cid
        assert np.linalg.norm(x.astype(np.float64) - ref.x) <= 1e-9 * np.linalg.norm(ref.x), cid
    else:
        assert (st.iterations, st.matvecs, st.info, st.breakdown) == (ref.iterations, ref.matvecs, ref.info, ref.breakdown), \
            (cid, (st.iterations, st.matvecs, st.info, st.breakdown), (ref.iterations, ref.matvecs, ref.info, ref.breakdown))
        assert np.array_equal(x, ref.x, equal_nan=True), cid
        assert st.recurrence_rs == ref.recurrence_rs, (cid, st.recurrence_rs, ref.recurrence_rs)
    _check_stats_long_double(solver, dt, sp.csr_matrix((val, col, crow), shape=(n, n)), dinv, b, x, st, kw)


# ---------------------------------------------------------------------------------------------- Chebyshev epilogue
@pytest.mark.parametrize("name", sorted(OC.CHEB))
def test_cheb_apply_on_unsorted_or_duplicate_rows(hipk, oracle, monkeypatch, name):
    matrix, transform, dtype, env, plain_only, note = OC.CHEB[name]
    f = np.float64 if dtype == OC.DOUBLE else np.float32
    n, degree = OC.N_CHEB, 3
    crow, col, val, diag = CC.band(n, OC.CHEB_OFFSETS[matrix])
    crow, col, val = OC.TRANSFORMS[transform](crow, col, val, seed=len(matrix))
    val = val.astype(f)
    dinv, r = CC.apply_inputs(n, diag, f)
    M, coef = CC.apply_coefficients(degree, dinv)
    ref = mirror(oracle, crow, col, val, M, r, dtype=f)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("HIPK_CHEB_FUSED", "1")
    h = hipk.CsrHandle(torch.from_numpy(crow).to(DEV), torch.from_numpy(col).to(DEV), torch.from_numpy(val).to(DEV), (n, n))
    try:
        assert h.path() == "coded"
        if plain_only:
            h.set_path(plain_only=True)
        rd, dd = torch.from_numpy(r).to(DEV), torch.from_numpy(dinv).to(DEV)
        r0, d0 = rd.clone(), dd.clone()
        z = hipk.cheb_apply(h, degree, dd, coef, rd)
        got = hipk.CsrHandle.last_spmv_kernel()
        z = z.cpu().numpy()
        _reported(notes=[got])
        assert got == note, got
        assert torch.equal(rd, r0) and torch.equal(dd, d0)
        d = differs(z, ref)
        assert d is None, f"{name} [{got}]: {d}"
    finally:
        h.close()


# ---------------------------------------------------------------------------------------------- transpose
def _with_empty_rows(crow, col, val):
    """Rows r % 7 == 3 emptied and every entry of a column c % 11 == 5 dropped: empty rows in A and in A^T."""
    rows = OC._rows(crow)
    keep = (rows % 7 != 3) & (col % 11 != 5)
    lens = np.bincount(rows[keep], minlength=len(crow) - 1)
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), col[keep], val[keep]


def _transpose_in_arenas(hipk, h, n_cols, nnz, ht):
    """hipk_csr_transpose with `work` in a guarded arena of exactly hipk_csr_transpose_work_bytes and crow_t, col_t, val_t in arenas
    of exactly n_cols + 1, nnz and nnz elements (tests/_arena.py), in the four workspace states: no byte outside them is written,
    and the outputs are those of CsrHandle.transposed() whatever the workspace held."""
    from _arena import Arena, guard_bytes_for, run_states
    L = hipk.lib()
    wb = int(L.hipk_csr_transpose_work_bytes(h.ptr))
    item = ht.val.element_size()
    g = guard_bytes_for(max(nnz, n_cols + 1), 8)
    out = {"crow_t": Arena(DEV, 4 * (n_cols + 1), 16, g), "col_t": Arena(DEV, 4 * nnz, 16, g), "val_t": Arena(DEV, item * nnz, 16, g)}
    work = Arena(DEV, wb, 256, g)

    def run(i):
        for a in out.values():
            a.fill(0xA5)
        hipk._check(L.hipk_csr_transpose(h.ptr, out["crow_t"].data_ptr(), out["col_t"].data_ptr(), out["val_t"].data_ptr(),
                                         work.data_ptr(), wb, hipk._stream(h.device)), "hipk_csr_transpose")
        return {k: a.payload.cpu().numpy().tobytes() for k, a in out.items()}
    res = run_states(work, out, {}, run, label="hipk_csr_transpose")
    for k, t in (("crow_t", ht.crow), ("col_t", ht.col), ("val_t", ht.val)):
        assert res[0][k] == t.cpu().numpy().tobytes(), k


@pytest.mark.parametrize("dtype", [OC.DOUBLE, OC.FLOAT])
@pytest.mark.parametrize("empty", [False, True], ids=["square", "empty_rows"])
@pytest.mark.parametrize("transform", ["shuf", "dup_shuf", "zero"])
def test_transpose_is_a_stable_sort_by_column(hipk, oracle, transform, empty, dtype):
    f = np.float64 if dtype == OC.DOUBLE else np.float32
    n = 5003
    M = OC._band(n, (1, 2, 7), sym=False, seed=3)      # 7 entries per row, 20 tiles, the last of 139 rows
    crow, col, val = M.indptr.astype(np.int64), M.indices.astype(np.int64), M.data.astype(np.float64)
    if empty:
        crow, col, val = _with_empty_rows(crow, col, val)
    crow, col, val = OC.TRANSFORMS[transform](crow, col, val, seed=5)
    val = val.astype(f)
    rows = OC._rows(crow)
    order = np.argsort(col, kind="stable")           # by column; entries of one column keep their source (row-major) order
    crow_t = np.concatenate([[0], np.cumsum(np.bincount(col, minlength=n))]).astype(np.int64)
    col_t, val_t = rows[order], val[order]
    if empty:
        assert (np.diff(crow) == 0).any() and (np.diff(crow_t) == 0).any()
    h = hipk.CsrHandle(torch.from_numpy(crow).to(DEV), torch.from_numpy(col).to(DEV), torch.from_numpy(val).to(DEV), (n, n))
    try:
        ht = h.transposed()
        assert ht.crow.dtype == torch.int32 and ht.col.dtype == torch.int32 and ht.val.dtype == torch.from_numpy(val).dtype
        assert np.array_equal(ht.crow.cpu().numpy(), crow_t) and np.array_equal(ht.col.cpu().numpy(), col_t)
        got = ht.val.cpu().numpy()
        assert np.array_equal(got.view(np.int64 if f == np.float64 else np.int32), val_t.view(np.int64 if f == np.float64 else np.int32))
        _transpose_in_arenas(hipk, h, n, len(col), ht)
        x = np.random.default_rng(n).standard_normal(n).astype(f)
        y = hipk.spmv(ht, torch.from_numpy(x).to(DEV)).cpu().numpy()
        _reported(notes=[hipk.CsrHandle.last_spmv_kernel()])
        spmv = oracle.spmv if f == np.float64 else oracle.spmv32
        d = differs(y, spmv(crow_t, col_t.astype(np.int64), val_t, x))
        assert d is None, d
        d = differs(hipk.spmv(h, torch.from_numpy(x).to(DEV)).cpu().numpy(), spmv(crow, col, val, x))
        assert d is None, d
        ht.close()
    finally:
        h.close()


# ---------------------------------------------------------------------------------------------- Python surface
def _dyadic(sym, transform):
    """A 12-entry band, n = 2085, whose entries are multiples of 2^-10 (the diagonal: the off-diagonal absolute row sum + 0.5, exact),
    so that sums of stored entries and of their absolute values are exact in ANY order: (crow, col, val) under `transform`.  The
    quarter of a split entry is a multiple of 2^-12, still exact."""
    import scipy.sparse as sp
    M = OC._band(2085, (1, 2, 3, 4, 5), match=300, sym=sym, seed=2)
    M.setdiag(0.0)
    M.eliminate_zeros()
    M.data = np.round(M.data * 1024.0) / 1024.0
    M = (M + sp.diags(np.asarray(abs(M).sum(axis=1)).ravel() + 0.5)).tocsr()
    M.sort_indices()
    assert np.array_equal(M.data * 1024.0, np.round(M.data * 1024.0)) and int(np.diff(M.indptr).max()) == 12
    return OC.TRANSFORMS[transform](M.indptr.astype(np.int64), M.indices.astype(np.int64), M.data.astype(np.float64), seed=1)


def _csr_tensor(crow, col, val):
    n = len(crow) - 1
    return torch.sparse_csr_tensor(torch.from_numpy(crow), torch.from_numpy(col), torch.from_numpy(val), size=(n, n)).to(DEV)


@pytest.mark.parametrize("transform", ["shuf", "dup_diag"])
@pytest.mark.parametrize("solver", ["cg", "bicgstab", "gmres"])
def test_python_solvers_neither_sort_nor_coalesce(hipk, oracle, solver, transform):
    from pytorch_sparse_solver import module_a as A_
    crow, col, val = _dyadic(solver == "cg", transform)
    n = len(crow) - 1
    A = _csr_tensor(crow, col, val)
    h = hipk.handle_for(A)
    assert h.nnz == len(col) and np.array_equal(h.col.cpu().numpy(), col) and np.array_equal(h.val.cpu().numpy(), val)
    b = np.random.default_rng(n).standard_normal(n)
    kw = dict(tol=1e-10, maxiter=300) if solver != "gmres" else dict(tol=1e-10, restart=20, maxiter=5)
    x, info = getattr(A_, solver)(A, torch.from_numpy(b).to(DEV), **kw)
    st = A_.get_last_stats()
    ref = getattr(oracle, solver)(crow, col, val, b, **kw, **({"gpu_tolerances": True} if solver == "gmres" else {}))
    _reported(forms=[hipk.last_solve_form()])
    assert np.array_equal(x.cpu().numpy(), ref.x)
    assert (info, st.iterations, st.matvecs, st.breakdown) == (ref.info, ref.iterations, ref.matvecs, ref.breakdown) and ref.matvecs > 1
    assert st.residual_norm == ref.residual_norm and st.recurrence_rs == ref.recurrence_rs
    hipk.clear_cache()


def _ulps(a, ref):
    """|a - ref| in units in the last place of a's dtype at ref (ref: long double)."""
    f = a.dtype.type
    return np.abs(a.astype(np.longdouble) - ref) / np.spacing(np.abs(ref).astype(f)).astype(np.longdouble)


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
def test_preconditioners_add_duplicate_diagonal_entries(hipk, oracle, dt):
    from pytorch_sparse_solver.module_a import (BlockJacobiPreconditioner, ChebyshevPreconditioner, JacobiPreconditioner, bicgstab, cg,
                                                get_last_stats, gmres)
    crow, col, val = _dyadic(True, "dup_diag")
    val = val.astype(dt)             # multiples of 2^-12 below 16: exact in fp32 as well
    assert np.array_equal(val.astype(np.float64), _dyadic(True, "dup_diag")[2])
    n = len(crow) - 1
    rows = OC._rows(crow)
    on = col == rows
    assert np.array_equal(np.bincount(rows[on], minlength=n), np.full(n, 2))
    Ld = np.longdouble
    diag = np.zeros(n, dtype=Ld)
    np.add.at(diag, rows[on], val[on].astype(Ld))
    A = _csr_tensor(crow, col, val)
    J = JacobiPreconditioner(A)
    dinv = J.dinv.cpu().numpy()
    # one rounding for the sum of the two stored entries, one for the reciprocal: 2 ulp of the exact reciprocal
    assert dinv.dtype == dt and float(_ulps(dinv, 1 / diag).max()) <= 2.0
    C = ChebyshevPreconditioner(A, degree=3)
    assert float(_ulps(C.dinv.cpu().numpy(), 1 / diag).max()) <= 2.0
    # Gershgorin: max_i (sum over the STORED entries of |a_ij|) / d_i -- every sum here is exact in any order
    absum = np.zeros(n, dtype=np.float64)
    np.add.at(absum, rows, np.abs(val).astype(np.float64))
    assert np.array_equal(C._abs_row_sums().cpu().numpy().astype(np.float64), absum)
    assert C.lmax == float((absum / diag.astype(np.float64)).max())
    bs = 4
    B = BlockJacobiPreconditioner(A, block_size=bs)
    nb = (n + bs - 1) // bs
    blocks = np.zeros((nb, bs, bs), dtype=dt)
    inb = rows // bs == col // bs
    np.add.at(blocks, (rows[inb] // bs, rows[inb] % bs, col[inb] % bs), val[inb])
    for i in range(n, nb * bs):
        blocks[nb - 1, i % bs, i % bs] = 1.0
    from pytorch_sparse_solver.module_a.preconditioners import _diagonal_blocks
    assert np.array_equal(_diagonal_blocks(A, bs).cpu().numpy(), blocks)
    assert np.array_equal(B.binv.cpu().numpy(), torch.linalg.inv(torch.from_numpy(blocks).to(DEV)).cpu().numpy())

    b = np.random.default_rng(n + 1).standard_normal(n).astype(dt)
    bd = torch.from_numpy(b).to(DEV)
    sfx = "" if dt == np.float64 else "32"
    tol = 1e-10 if dt == np.float64 else 1e-5
    for solve, name, okw in ((cg, "pcg_jacobi", {}), (bicgstab, "bicgstab_jacobi", {}), (gmres, "gmres_jacobi", {"gpu_tolerances": True})):
        kw = dict(tol=tol, maxiter=200) if solve is not gmres else dict(tol=tol, restart=20, maxiter=4)
        x, info = solve(A, bd, M=J, **kw)
        st = get_last_stats()
        ref = getattr(oracle, name + sfx)(crow, col, val, dinv, b, **kw, **okw)
        assert np.array_equal(x.cpu().numpy(), ref.x), name
        assert (info, st.iterations, st.matvecs) == (ref.info, ref.iterations, ref.matvecs) and ref.matvecs > 1, name
        assert st.residual_norm == ref.residual_norm, name
    if dt == np.float64:
        x, info = cg(A, bd, M=B, tol=tol, maxiter=200)
        st = get_last_stats()
        ref = oracle.pcg_blockjacobi(crow, col, val, B.binv.cpu().numpy(), b, tol=tol, maxiter=200)
        assert "callable_M" in st.method and st.matvecs == ref.matvecs and np.array_equal(x.cpu().numpy(), ref.x)
    # the Chebyshev apply on the device against the mirror on the same arrays, and a solve through it that converges
    z = C(bd).cpu().numpy()
    d = differs(z, mirror(oracle, crow, col, val, C, b, dtype=dt))
    assert d is None, d
    x, info = cg(A, bd, M=C, tol=tol, maxiter=200)
    assert info == 0 and "callable_M" in get_last_stats().method
    hipk.clear_cache()
