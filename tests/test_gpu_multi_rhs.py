"""GPU: the block solves of cg_multi / bicgstab_multi (csrc/hipk_multi.hip, reached through multi_rhs._block_solve).  Every column
of a block solve is bit for bit the single solve of that column on the device and the oracle's solve of it, with the same info,
iterations and matvecs; the block loop ran (its path name), and the block-SpMV launch count is max_j matvecs_j per block of 16
columns -- not the sum a column-by-column loop would give.  The public cg_multi / bicgstab_multi route device operands to the
column loop (measured faster, multi_rhs._multi): pinned here too, with the same bits.

The k sweeps and the tile / chunk edge sizes also run the block solve on guarded memory (tests/_arena.py): B and X (ldb = ldx = k)
in arenas of exactly n * k elements, `work` in one of exactly hipk_multi_work_bytes, in the four workspace states; every run must
leave the guards and B alone and reproduce, bit for bit, the X and the column stats pinned above."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _csr_np(A):
    Ac = A.cpu()
    if Ac.layout != torch.sparse_csr:
        Ac = Ac.to_sparse_csr()
    return Ac.crow_indices().numpy(), Ac.col_indices().numpy(), Ac.values().numpy()


def _oracle_solve(oracle, kind, A, dinv, b, x0, dtype, kw):
    crow, col, val = _csr_np(A)
    f32 = dtype == torch.float32
    name = {("cg", False): "cg", ("cg", True): "pcg_jacobi", ("bicgstab", False): "bicgstab",
            ("bicgstab", True): "bicgstab_jacobi"}[(kind, dinv is not None)]
    fn = getattr(oracle, name + ("32" if f32 else ""))
    args = (crow, col, val) + ((dinv,) if dinv is not None else ()) + (b,)
    return fn(*args, x0=x0, **kw)


def _bits(t):
    """Bit patterns: equal NaNs compare equal, as bitwise parity means."""
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def _same(a, b):
    return a == b or (a != a and b != b)


def _check_in_arenas(kind, A, B, X0, M, X, st, kw):
    """hipk_{cg,bicgstab}_solve_multi with B, X and work in guarded memory, once per workspace state: equal to (X, st) every time."""
    from pytorch_sparse_solver import _hipk
    from _arena import Arena, guard_bytes_for, run_states
    from _solve_runner import stat_bits
    h = _hipk.handle_for(A)
    n, k = B.shape
    item = X.element_size()
    g = guard_bytes_for(n, item)
    ba, xa = Arena(DEV, n * k * item, 16, g), Arena(DEV, n * k * item, 16, g)
    Bd = ba.put(B.to(X.dtype)).view(n, k)
    X0d = torch.zeros_like(X) if X0 is None else X0.to(X.dtype).contiguous()
    Xd = xa.view(X.dtype, n * k).view(n, k)
    guarded, readonly = {"X": xa, "B": ba}, {"B": ba}
    dinv = None
    if M is not None:
        da = Arena(DEV, n * item, 16, g)
        dinv = da.put(M.dinv.to(X.dtype))
        guarded["dinv"] = readonly["dinv"] = da
    work = Arena(DEV, _hipk.multi_work_bytes(n, k, X.dtype, kind, dinv is not None), 256, g)

    def run(i):
        Xd.copy_(X0d)
        s = _hipk.solve_multi(kind, h, dinv, Bd, Xd, tol=kw.get("tol", 1e-5), atol=kw.get("atol", 0.0), maxiter=kw.get("maxiter"),
                              work=work.payload)
        assert _hipk.last_solve_path() == f"hipk_{kind}_multi launch sequence"
        return {"X": xa.payload.cpu().numpy().tobytes(), "stats": b"".join(stat_bits(c) for c in s.columns),
                "block_spmvs": s.block_spmvs}
    res = run_states(work, guarded, readonly, run, label=f"{kind}_multi n={n} k={k}")
    assert res[0]["X"] == X.contiguous().cpu().numpy().tobytes(), "the block solve on guarded memory differs from the one on fresh tensors"
    assert res[0]["stats"] == b"".join(stat_bits(c) for c in st.columns) and res[0]["block_spmvs"] == st.block_spmvs


def check(oracle, kind, A, B, X0=None, M=None, use_oracle=True, arenas=False, **kw):
    """Runs the block solve and, column by column, the single solve and the oracle; asserts the whole contract.
    arenas: also on guarded memory in every workspace state (_check_in_arenas)."""
    from pytorch_sparse_solver import _hipk
    from pytorch_sparse_solver.module_a import bicgstab, bicgstab_multi, cg, cg_multi, get_last_stats
    from pytorch_sparse_solver.module_a.multi_rhs import _block_solve
    multi, single = (cg_multi, cg) if kind == "cg" else (bicgstab_multi, bicgstab)
    # the public entry point: routed to the column loop for device operands (multi_rhs._multi), the same bits
    Xp, infop = multi(A, B, X0, M=M, **kw)
    assert get_last_stats().block_spmvs == 0 and "multi" not in _hipk.last_solve_path()
    X, info = _block_solve(kind, A, B, X0, kw.get("tol", 1e-5), kw.get("atol", 0.0), kw.get("maxiter"), M)
    st = get_last_stats()
    assert _hipk.last_solve_path() == f"hipk_{kind}_multi launch sequence"
    assert np.array_equal(_bits(Xp), _bits(X)) and torch.equal(infop, info)
    assert isinstance(st, _hipk.MultiSolveStats)
    if arenas:
        _check_in_arenas(kind, A, B, X0, M, X, st, kw)
    n, k = B.shape
    wdt = torch.float32 if A.dtype == torch.float32 else torch.float64
    assert X.shape == (n, k) and X.dtype == wdt and X.device == B.device
    assert info.dtype == torch.int64 and info.device.type == "cpu" and info.shape == (k,)
    assert len(st.columns) == k
    dinv = None if M is None else M.dinv.to(wdt).cpu().numpy()
    for j in range(k):
        x0j = None if X0 is None else X0[:, j].clone()
        xs, infs = single(A, B[:, j].clone(), x0j, M=M, **kw)   # a copy: the single path wants a 16-byte aligned vector
        ss = get_last_stats()
        c = st.columns[j]
        assert np.array_equal(_bits(X[:, j]), _bits(xs)), f"column {j} differs from the single solve"
        assert (int(info[j]), c.iterations, c.matvecs, c.breakdown) == (infs, ss.iterations, ss.matvecs, ss.breakdown), j
        assert _same(c.residual_norm, ss.residual_norm) and _same(c.x_norm, ss.x_norm) and c.b_norm == ss.b_norm, j
        if use_oracle:
            bj = B[:, j].to(wdt).cpu().numpy()
            x0n = None if x0j is None else x0j.to(wdt).cpu().numpy()
            ref = _oracle_solve(oracle, kind, A, dinv, bj, x0n, wdt, kw)
            assert np.array_equal(_bits(X[:, j]), _bits(ref.x)), f"column {j} differs from the oracle"
            assert (int(info[j]), c.iterations, c.matvecs, c.breakdown) == (ref.info, ref.iterations, ref.matvecs, ref.breakdown), j
            assert _same(c.recurrence_rs, ref.recurrence_rs), j
    mv = [c.matvecs for c in st.columns]
    assert st.block_spmvs == sum(max(mv[j:j + 16]) for j in range(0, k, 16))
    return X, info, st


def _poisson(nx, dtype=torch.float64):
    from pytorch_sparse_solver.utils.matrix_utils import create_poisson_2d_csr
    return create_poisson_2d_csr(nx, nx, device=DEV, dtype=dtype)


def _convdiff(nx, dtype=torch.float64):
    from pytorch_sparse_solver.utils.matrix_utils import create_convdiff_2d_csr
    return create_convdiff_2d_csr(nx, nx, device=DEV, dtype=dtype).to(DEV)


def _rhs(n, k, seed, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, k, generator=g, dtype=torch.float64).to(dtype).to(DEV)


def _random_spd(n, seed, long_rows=False):
    """Sparse diagonally dominant symmetric matrix of n rows (tridiagonal + random couplings; optionally row/column 0 dense)."""
    rng = np.random.default_rng(seed)
    D = {}
    for i in range(n):
        if i + 1 < n:
            D[(i, i + 1)] = D[(i + 1, i)] = -1.0
    for _ in range(2 * n):
        i, j = rng.integers(0, n, 2)
        if i != j:
            v = -rng.uniform(0.05, 0.5)
            D[(i, j)] = D[(j, i)] = v
    if long_rows:
        for j in range(1, n):
            D[(0, j)] = D[(j, 0)] = -0.01
    rows = [[] for _ in range(n)]
    for (i, j), v in D.items():
        rows[i].append((j, v))
    crow, col, val = [0], [], []
    for i in range(n):
        ent = sorted(rows[i] + [(i, 1.0 + sum(-v for _, v in rows[i]))])
        col += [j for j, _ in ent]
        val += [v for _, v in ent]
        crow.append(len(col))
    return torch.sparse_csr_tensor(torch.tensor(crow), torch.tensor(col), torch.tensor(val, dtype=torch.float64),
                                   size=(n, n)).to(DEV)


def _eigvec(nx, p, q):
    i = torch.arange(nx, dtype=torch.float64)
    v = torch.sin(np.pi * p * (i + 1) / (nx + 1))[:, None] * torch.sin(np.pi * q * (i + 1) / (nx + 1))[None, :]
    return v.reshape(-1).to(DEV)


# ------------------------------------------------------------------ k: padding (KP 2, 4, 8, 16) and the 16-column split
@pytest.mark.parametrize("k", [1, 2, 3, 8, 16, 17])
def test_cg_multi_k_sweep(hipk, oracle, k):
    A = _poisson(40)
    _, info, st = check(oracle, "cg", A, _rhs(1600, k, k), arenas=True, tol=1e-6)
    assert (info == 0).all()


@pytest.mark.parametrize("k", [1, 2, 3, 8, 16, 17])
def test_bicgstab_multi_k_sweep(hipk, oracle, k):
    A = _convdiff(40)
    check(oracle, "bicgstab", A, _rhs(1600, k, 100 + k), arenas=True, tol=1e-6)


# ------------------------------------------------------------------ n at tile (256) and chunk (2048) edges
@pytest.mark.parametrize("n", [1, 255, 257, 2049])
@pytest.mark.parametrize("kind", ["cg", "bicgstab"])
def test_multi_tile_and_chunk_edges(hipk, oracle, kind, n):
    A = _random_spd(n, seed=n)
    check(oracle, kind, A, _rhs(n, 3, n), arenas=True, tol=1e-7)


@pytest.mark.parametrize("kind,nx,maxiter", [("cg", 200, None), ("bicgstab", 200, None), ("cg", 500, 300)])
def test_multi_mid_sizes(hipk, oracle, kind, nx, maxiter):
    """n = 40 000 and 250 000: the sizes whose single solves run the one-launch loops -- the block launch sequence matches them."""
    A = _poisson(nx) if kind == "cg" else _convdiff(nx)
    check(oracle, kind, A, _rhs(nx * nx, 4, nx), tol=1e-6, maxiter=maxiter)


def test_cg_multi_general_csr_4m(hipk, oracle):
    """N = 4 M variable-coefficient matrix (no coded form), bounded maxiter: 1954 reduction chunks, 15625 tiles."""
    from pytorch_sparse_solver.utils.matrix_utils import create_variable_diffusion_2d_csr
    A = create_variable_diffusion_2d_csr(2000, 2000, device=DEV).to(DEV)
    _, info, st = check(oracle, "cg", A, _rhs(4_000_000, 2, 7), tol=1e-8, maxiter=20)
    assert [c.iterations for c in st.columns] == [20, 20] and st.block_spmvs == 22


@pytest.mark.parametrize("kind", ["cg", "bicgstab"])
def test_multi_long_rows(hipk, oracle, kind):
    """Row 0 and column 0 are dense (300 entries): the 64-lane split of rows longer than 32 entries."""
    A = _random_spd(300, seed=5, long_rows=True)
    check(oracle, kind, A, _rhs(300, 3, 5), tol=1e-8)


# ------------------------------------------------------------------ fp32 and Jacobi
@pytest.mark.parametrize("jacobi", [False, True])
@pytest.mark.parametrize("kind", ["cg", "bicgstab"])
def test_multi_fp32(hipk, oracle, kind, jacobi):
    from pytorch_sparse_solver.module_a import JacobiPreconditioner
    A = (_poisson(30) if kind == "cg" else _convdiff(30)).to(torch.float32)
    M = JacobiPreconditioner(A) if jacobi else None
    X, _, _ = check(oracle, kind, A, _rhs(900, 5, 11, torch.float32), M=M, tol=1e-4)
    assert X.dtype == torch.float32


@pytest.mark.parametrize("kind", ["cg", "bicgstab"])
def test_multi_jacobi_fp64(hipk, oracle, kind):
    from pytorch_sparse_solver.module_a import JacobiPreconditioner
    from pytorch_sparse_solver.utils.matrix_utils import create_variable_diffusion_2d_csr
    A = create_variable_diffusion_2d_csr(40, 40, device=DEV).to(DEV)
    check(oracle, kind, A, _rhs(1600, 5, 12), M=JacobiPreconditioner(A), tol=1e-7)


# ------------------------------------------------------------------ freezing: columns stopping at very different iterations
@pytest.mark.parametrize("jacobi", [False, True])
@pytest.mark.parametrize("kind", ["cg", "bicgstab"])
def test_multi_columns_stop_apart(hipk, oracle, kind, jacobi):
    """A zero column, an exact x0 (b = A x0), one eigenvector (a few iterations) and two hard columns: each column stops at its own
    iteration and the frozen ones are left alone (bitwise = their single solves)."""
    from pytorch_sparse_solver.module_a import JacobiPreconditioner
    nx = 40
    A = _poisson(nx) if kind == "cg" else _convdiff(nx)
    n = nx * nx
    R = _rhs(n, 2, 21)
    x_ex = _rhs(n, 1, 22)[:, 0]
    b_ex = hipk.spmv(hipk.handle_for(A), x_ex)   # the library's own product: b - A x_ex is exactly zero
    B = torch.stack([torch.zeros(n, dtype=torch.float64, device=DEV), b_ex, _eigvec(nx, 1, 2), R[:, 0], R[:, 1]], dim=1)
    X0 = torch.zeros_like(B)
    X0[:, 1] = x_ex
    M = JacobiPreconditioner(A) if jacobi else None
    _, info, st = check(oracle, kind, A, B, X0, M=M, tol=1e-6)
    its = [c.iterations for c in st.columns]
    assert its[0] == 0 and its[1] == 0 and len(set(its)) >= 3


@pytest.mark.parametrize("kind", ["cg", "bicgstab"])
def test_multi_maxiter_hit_by_some_columns(hipk, oracle, kind):
    nx = 40
    A = _poisson(nx) if kind == "cg" else _convdiff(nx)
    n = nx * nx
    B = torch.stack([_eigvec(nx, 1, 1), _rhs(n, 1, 31)[:, 0], torch.zeros(n, dtype=torch.float64, device=DEV)], dim=1)
    _, info, st = check(oracle, kind, A, B, tol=1e-6, maxiter=10)
    its = [c.iterations for c in st.columns]
    assert its[1] == 10 and int(info[1]) == -1 and its[2] == 0
    if kind == "cg":   # an eigenvector of the Poisson matrix: a Krylov space of dimension one
        assert its[0] < 10 and int(info[0]) == 0


# ------------------------------------------------------------------ BiCGStab breakdowns in one column only
@pytest.mark.parametrize("code", ["-10", "-11"])
def test_bicgstab_multi_breakdown_in_one_column(hipk, oracle, code):
    case = json.load(open(os.path.join(GOLD, "bicgstab_breakdown.json")))[code]
    A = torch.tensor(case["A"], dtype=torch.float64, device=DEV)
    n = A.shape[0]
    b = torch.tensor(case["b"], dtype=torch.float64, device=DEV)
    e0 = torch.zeros(n, dtype=torch.float64, device=DEV)
    e0[0] = 1.0
    B = torch.stack([e0, b, torch.arange(1, n + 1, dtype=torch.float64, device=DEV)], dim=1)
    _, info, st = check(oracle, "bicgstab", A, B, tol=1e-8)
    assert st.columns[1].breakdown == int(code)
    assert any(st.columns[j].breakdown != int(code) for j in (0, 2))


# ------------------------------------------------------------------ contract of the device route
def test_multi_device_route_errors(hipk):
    from pytorch_sparse_solver.module_a import cg_multi
    A = _poisson(8)
    B = _rhs(64, 2, 1)
    with pytest.raises(ValueError, match="must have shape"):
        cg_multi(A, B[:, 0])
    with pytest.raises(ValueError, match="matching shapes"):
        cg_multi(A, B, torch.zeros(64, 3, dtype=torch.float64, device=DEV))
    with pytest.raises(RuntimeError, match="size mismatch"):
        cg_multi(A, _rhs(63, 2, 1))
    with pytest.raises(ValueError, match="cg_differentiable"):
        cg_multi(A, B.clone().requires_grad_(True))
    from pytorch_sparse_solver.module_a.multi_rhs import _block_solve
    with pytest.raises(RuntimeError, match="size mismatch"):
        _block_solve("cg", A, _rhs(63, 2, 1), None, 1e-5, 0.0, None, None)


# ------------------------------------------------------------------ a special right-hand side between two ordinary ones
def _special_cases():
    import _special_cases as S
    out = []
    for dtn in (S.F64, S.F32):
        for name in ("nan-b", "inf-b", "b-overflow", "b-underflow", "zero-chunk"):
            if name in S.REGIME_NAMES[dtn]:       # 2^520 and 2^-540 are no fp32 numbers
                out.append((dtn, name))
    return out


@pytest.mark.parametrize("jacobi", [False, True], ids=["plain", "jacobi"])
@pytest.mark.parametrize("kind", ["cg", "bicgstab"])
@pytest.mark.parametrize("dtn, name", _special_cases(), ids=[f"{d}-{n}" for d, n in _special_cases()])
def test_multi_neighbours_of_a_special_column(hipk, oracle, kind, jacobi, dtn, name):
    """Three right-hand sides on one matrix of 2049 rows (two reduction chunks), the middle one in a special regime of b
    (tests/_special_cases.py): NaN, inf, <b, b> overflowing or underflowing, a zero chunk.  Every column -- the special one and its
    ordinary neighbours -- is its own single-right-hand-side oracle solve bit for bit (NaNs as one pattern: the sign of a produced
    NaN is the implementation's), with its own info, iterations, matvecs and breakdown."""
    import _special_cases as S
    from _oracle_cases import _band
    from pytorch_sparse_solver import _hipk
    from pytorch_sparse_solver.module_a import JacobiPreconditioner, get_last_stats
    from pytorch_sparse_solver.module_a.multi_rhs import _block_solve
    wdt, ndt = (torch.float64, np.float64) if dtn == S.F64 else (torch.float32, np.float32)
    n = 2049
    Msp = _band(n, (1, 2)) if kind == "cg" else _band(n, (1, 2), sym=False, seed=1)
    A = torch.sparse_csr_tensor(torch.from_numpy(Msp.indptr.astype(np.int64)), torch.from_numpy(Msp.indices.astype(np.int64)),
                                torch.from_numpy(Msp.data.astype(ndt)), size=Msp.shape).to(DEV)
    reg = S.regime(name, dtn)
    Bh = _rhs(n, 3, 40, wdt).cpu().numpy()
    Bh[:, 1] = S.special_b(S.scaled(np.ascontiguousarray(Bh[:, 1]), reg[3]), reg[4])
    B = torch.from_numpy(Bh).to(DEV)
    M = JacobiPreconditioner(A) if jacobi else None
    kw = dict(tol=1e-8 if dtn == S.F64 else 1e-4, atol=0.0, maxiter=S.NAN_MAXITER if name == "nan-b" else S.MAXITER_CAP)
    X, info = _block_solve(kind, A, B, None, kw["tol"], kw["atol"], kw["maxiter"], M)
    st = get_last_stats()
    assert _hipk.last_solve_path() == f"hipk_{kind}_multi launch sequence"
    dinv = None if M is None else M.dinv.to(wdt).cpu().numpy()
    Xh = X.cpu().numpy()

    def canon(a):
        a = np.array(a, copy=True)
        a[np.isnan(a)] = np.nan
        return a.view(np.int64 if a.dtype == np.float64 else np.int32)

    seen = []
    for j in range(3):
        ref = _oracle_solve(oracle, kind, A, dinv, np.ascontiguousarray(Bh[:, j]), None, wdt, kw)
        c = st.columns[j]
        got, want = (int(info[j]), c.iterations, c.matvecs, c.breakdown), (ref.info, ref.iterations, ref.matvecs, ref.breakdown)
        seen.append(want)
        assert got == want, (j, got, want)
        assert np.array_equal(canon(Xh[:, j]), canon(ref.x)), f"column {j} differs from its own oracle solve"
    # the neighbours are ordinary solves, the middle column took a branch of its own
    assert seen[0][1] > 0 and seen[2][1] > 0 and np.isfinite(Xh[:, [0, 2]]).all(), seen
    if name == "nan-b":
        assert seen[1][1] == S.NAN_MAXITER and np.isnan(Xh[:, 1]).all(), seen
    elif name != "zero-chunk":
        assert seen[1][1] == 0 and not Xh[:, 1].any(), seen
