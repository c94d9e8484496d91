"""The case table of gmres_batch (tests/test_gmres_batch_cases.py checks it on the CPU oracle, tests/test_gpu_gmres_batch.py runs every
case through hipk_gm_batch_kernel).

A case: id, dtype ('f64' | 'f32'), pre (Jacobi), restart, method ('batched' | 'incremental'), the pattern (a convection-diffusion
grid, a dense n x n pattern, or `pattern` + `transform` of tests/_batch_patterns.py: general rows of 1 to 32 entries in stored
order), S, the x0 kind ('none' | 'random' | 'exact': the exact solution of system 1, which then runs 0
cycles and 2 operator applications), keyword arguments and the path string the kernel route must report.  S > 4 cycles the four
matrices with fresh seeded right-hand sides.  `special`: system 0 of the 7 x 5 pattern has only a constant diagonal ('diag': happy
breakdown at step 1) or only zeros ('zero': a zero column in H; 'batched' meets a zero Cholesky pivot) with b = ones, next to a partner
that converges normally.  `kernel` False: the case lies outside the kernel's envelope ('auto' loops, 'kernel' raises)."""
import zlib
from dataclasses import dataclass, field

import numpy as np

from _batch_cases import CONVDIFF, MAX_N, MAX_ROW, TOL, _dense_pattern, _np_dtype, jacobi_dinv  # noqa: F401

MAX_RESTART = 31


@dataclass
class Case:
    id: str
    dtype: str
    pre: bool
    restart: int
    method: str
    grid: tuple = None        # (nx, ny), or None for a dense pattern
    dense: int = None         # n of a dense pattern
    pattern: tuple = None     # ('rag31', n) | ('rag32', n) | ('dense32',) | ('empty', n) of tests/_batch_patterns.py
    transform: str = None     # a key of tests/_order_cases.TRANSFORMS, applied to `pattern`
    S: int = 4
    x0: str = "none"
    kwargs: dict = field(default_factory=dict)
    zero_b: int = None        # this system's right-hand side is 0
    special: str = None       # 'diag' | 'zero'
    kernel: bool = True
    solver: str = "gmres"

    @property
    def path(self):
        return "hipk_gm_batch_kernel<%s,%s>" % ("double" if self.dtype == "f64" else "float", "true" if self.pre else "false")

    @property
    def solve_kwargs(self):
        kw = {"tol": TOL[self.dtype], "restart": self.restart, "solve_method": self.method}
        kw.update(self.kwargs)
        return kw


def _c(dtype, pre, grid, restart, method, S=4, x0="none", tag="", **kw):
    name = f"gmres{'-jac' if pre else ''}-{dtype}-{grid[0]}x{grid[1]}-r{restart}-{method[0]}-S{S}-x0{x0}{tag}"
    return Case(id=name, dtype=dtype, pre=pre, restart=restart, method=method, grid=grid, S=S, x0=x0, **kw)


def _d(dtype, pre, n, restart, method):
    return Case(id=f"gmres{'-jac' if pre else ''}-{dtype}-dense{n}-r{restart}-{method[0]}", dtype=dtype, pre=pre, restart=restart,
                method=method, dense=n, S=2)


def _p(dtype, pre, pattern, transform, restart, method, S=4, x0="none", tag="", **kw):
    name = (f"gmres{'-jac' if pre else ''}-{dtype}-{'n'.join(str(v) for v in pattern)}-{transform or 'sorted'}-r{restart}-{method[0]}"
            f"-S{S}-x0{x0}{tag}")
    return Case(id=name, dtype=dtype, pre=pre, restart=restart, method=method, pattern=pattern, transform=transform, S=S, x0=x0, **kw)


B, I = "batched", "incremental"
CASES = [
    # ---- n = 35: one partial tile; restart 1, 2, 5
    _c("f64", False, (7, 5), 5, B), _c("f64", False, (7, 5), 1, I), _c("f64", True, (7, 5), 2, B, S=5, x0="random"),
    _c("f32", False, (7, 5), 5, I, S=2), _c("f64", False, (7, 5), 5, B, S=1),
    _c("f64", False, (7, 5), 5, I, S=1030, x0="random"),                       # more workgroups than are resident
    # ---- 255, 256, 257: the edges of one tile and of one virtual-thread block
    _c("f64", False, (17, 15), 7, I, S=5, x0="exact"), _c("f64", True, (16, 16), 20, I), _c("f32", False, (16, 16), 20, B, x0="exact"),
    _c("f32", True, (257, 1), 8, B, x0="random"), _c("f64", False, (257, 1), 9, I),
    # ---- 1024, 1025: four tiles and one row more
    _c("f64", False, (32, 32), 20, B, S=300), _c("f32", False, (32, 32), 16, I), _c("f64", True, (32, 32), 5, B, x0="random"),
    _c("f32", False, (41, 25), 9, B, x0="random"), _c("f32", True, (41, 25), 30, I), _c("f64", False, (41, 25), 8, I),
    # ---- 2025, 2048, 2049, 2304: the edge of the first reduction chunk
    _c("f64", False, (45, 45), 31, B, x0="random"), _c("f64", True, (64, 32), 16, B), _c("f32", False, (64, 32), 30, B),
    _c("f64", False, (683, 3), 7, B), _c("f32", True, (683, 3), 20, I, x0="exact"),
    _c("f64", True, (48, 48), 31, I, x0="exact"), _c("f32", False, (48, 48), 20, B, S=5),
    # ---- 4096: the envelope's edge
    _c("f64", False, (64, 64), 20, B), _c("f64", True, (64, 64), 30, I, x0="random"), _c("f32", True, (64, 64), 20, B),
    _c("f64", False, (64, 64), 31, I),
    # ---- maxiter, atol, b = 0
    _c("f64", False, (32, 32), 5, B, x0="exact", tag="-maxiter3", kwargs={"maxiter": 3}),
    _c("f64", False, (17, 15), 5, I, tag="-atol", kwargs={"atol": 1e-2}),
    _c("f64", True, (16, 16), 8, B, S=5, tag="-b0", zero_b=2),
    # ---- dense patterns: n = 1, 2, 3; restart 5 > n = 3
    _d("f64", False, 1, 5, B), _d("f64", True, 2, 2, I), _d("f32", False, 3, 5, B), _d("f64", True, 3, 5, I),
    # ---- special systems next to a partner that converges
    _c("f64", False, (7, 5), 5, B, S=2, tag="-diag", special="diag"), _c("f64", False, (7, 5), 5, I, S=2, tag="-diag", special="diag"),
    _c("f64", False, (7, 5), 5, B, S=2, tag="-zero", special="zero"), _c("f64", False, (7, 5), 5, I, S=2, tag="-zero", special="zero"),
    _c("f32", False, (7, 5), 5, B, S=2, tag="-zero", special="zero"),
    # ---- outside the envelope: 'auto' takes the loop, 'kernel' raises
    _c("f64", False, (16, 16), 32, B, S=2, kernel=False),
    _c("f64", False, (17, 241), 5, B, S=2, kernel=False, kwargs={"maxiter": 4}),
    # ---- the pattern axis: rows of 1 .. 32 entries, unsorted, repeated, a stored zero, an empty row (n = 300: two tiles, the second
    # of 44 rows; n = 2049: nine tiles, a second reduction chunk of one row; dense 32: every row at the bound)
    _p("f64", False, ("rag31", 300), "dup_shuf", 10, I), _p("f64", True, ("rag31", 300), "dup_diag", 10, B, x0="random"),
    _p("f32", False, ("rag31", 2049), "shuf", 10, I, S=5), _p("f32", True, ("rag31", 2049), "dup_diag", 10, B),
    _p("f64", False, ("rag31", 2049), "zero", 10, I, x0="exact"),
    _p("f64", True, ("rag31", 2049), "rev", 10, B),                             # nnz odd: the padded copy of `values`
    _p("f64", False, ("rag32", 300), "shuf", 10, B),                            # rows of 1 and of 32 entries in one wavefront
    _p("f64", False, ("dense32",), "rev", 8, I, S=2),
    _p("f64", False, ("empty", 300), None, 5, B, tag="-maxiter2", kwargs={"maxiter": 2}),
    _p("f64", False, ("dense32",), "dup", 5, B, S=2, kernel=False),             # 33 entries per row: 'auto' loops, 'kernel' raises
]
PATTERN_CASES = [c for c in CASES if c.pattern]
BY_ID = {c.id: c for c in CASES}
# the cases that also run with HIPK_BATCH_LAUNCH_ITS = 7 and = 1 (every instantiation, both methods; > 1 launch each)
BUDGET_IDS = ["gmres-f64-7x5-r5-b-S4-x0none", "gmres-f64-7x5-r1-i-S4-x0none", "gmres-jac-f64-7x5-r2-b-S5-x0random",
              "gmres-f32-7x5-r5-i-S2-x0none", "gmres-jac-f64-16x16-r20-i-S4-x0none", "gmres-jac-f32-257x1-r8-b-S4-x0random",
              "gmres-f32-41x25-r9-b-S4-x0random", "gmres-jac-f32-41x25-r30-i-S4-x0none", "gmres-f64-683x3-r7-b-S4-x0none",
              "gmres-f64-64x64-r20-b-S4-x0none", "gmres-jac-f64-16x16-r8-b-S5-x0none-b0",
              # the pattern axis: a Jacobi case with 32-entry rows and a diagonal stored twice, and n = 2049 (the second chunk)
              "gmres-jac-f64-rag31n300-dup_diag-r10-b-S4-x0random", "gmres-f32-rag31n2049-shuf-r10-i-S5-x0none"]


def build(case):
    """-> dict crow, col (int32), vals (S, nnz), B (S, n), X0 ((S, n) or None), all numpy in the case's dtype."""
    dt = _np_dtype(case)
    rng = np.random.default_rng([zlib.crc32(case.id.encode()), 11])
    if case.pattern:
        from _batch_patterns import build_pattern
        crow, col, vals = build_pattern(case.pattern, case.transform, "gmres", case.S, rng)
        n = crow.size - 1
    elif case.dense:
        n = case.dense
        mats = [(3.0 + s) * np.eye(n) + 0.5 * np.ones((n, n)) + 0.25 * np.triu(np.ones((n, n)), 1) for s in range(case.S)]
        crow, col = _dense_pattern(n)
        vals = np.stack([M.reshape(-1) for M in mats])
    else:
        from pytorch_sparse_solver.utils.matrix_utils import create_convdiff_2d_csr
        nx, ny = case.grid
        four = [create_convdiff_2d_csr(nx, ny, g, d) for g, d in CONVDIFF]
        crow = four[0].crow_indices().numpy().astype(np.int32)
        col = four[0].col_indices().numpy().astype(np.int32)
        for A in four[1:]:
            assert np.array_equal(A.crow_indices().numpy(), crow) and np.array_equal(A.col_indices().numpy(), col), case.id
        vals = np.stack([four[s % 4].values().numpy() for s in range(case.S)])
        n = crow.size - 1
    Bm = rng.standard_normal((case.S, n))
    if case.special:
        rows = np.repeat(np.arange(n), np.diff(crow))
        vals[0] = np.where(col == rows, 2.5, 0.0) if case.special == "diag" else 0.0
        Bm[0] = 1.0
    vals = np.ascontiguousarray(vals.astype(dt))
    Bm = np.ascontiguousarray(Bm.astype(dt))
    S = vals.shape[0]
    assert S == case.S, case.id
    if case.zero_b is not None:
        Bm[case.zero_b] = 0
    X0 = None
    if case.x0 == "random":
        X0 = np.ascontiguousarray(rng.standard_normal((S, n)).astype(dt))
    elif case.x0 == "exact":
        from oracle import oracle as O
        X0 = np.ascontiguousarray(rng.standard_normal((S, n)).astype(dt))
        e = 1 % S
        Bm[e] = (O.spmv if case.dtype == "f64" else O.spmv32)(crow, col, vals[e], X0[e])    # then b - A x0 is exactly 0 for system e
    return {"crow": crow, "col": col, "vals": vals, "B": Bm, "X0": X0, "n": n, "nnz": int(col.size)}


def oracle_run(case, data, O, dinv=None):
    """The oracle's result per system (a list of OracleResult); dinv: the (S, n) Jacobi vectors a preconditioned case uses."""
    f32 = case.dtype == "f32"
    if case.pre:
        fn = O.gmres_jacobi32 if f32 else O.gmres_jacobi
        if dinv is None:
            dinv = jacobi_dinv(data)
    else:
        fn = O.gmres32 if f32 else O.gmres
    out = []
    for s in range(case.S):
        x0 = None if data["X0"] is None else data["X0"][s]
        args = (data["crow"], data["col"], data["vals"][s]) + ((dinv[s],) if case.pre else ()) + (data["B"][s], x0)
        out.append(fn(*args, gpu_tolerances=True, **case.solve_kwargs))
    return out


_cache = {}


def reference(case, O):
    """build + oracle_run once per case and process (shared by the tests; never modified)."""
    if case.id not in _cache:
        data = build(case)
        _cache[case.id] = (data, oracle_run(case, data, O))
    return _cache[case.id]
