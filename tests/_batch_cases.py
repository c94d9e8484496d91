"""The case table of cg_batch / bicgstab_batch (tests/test_batch_cases.py checks it on the CPU oracle, tests/test_gpu_batch.py runs
every case through the batch kernels).

A case: id, solver ('cg' | 'bicgstab'), dtype ('f64' | 'f32'), pre (Jacobi), the pattern (a grid of the project's generators, a
dense n x n pattern, or `pattern` + `transform` of tests/_batch_patterns.py: general rows of 1 to 32 entries in stored order), S, the x0 kind ('none' | 'random' | 'exact': the exact solution of system 1, so that system alone runs 0
iterations), keyword arguments, environment and the path string the kernel route must report.  S > 4 cycles the four matrices with
fresh seeded right-hand sides.  `kernel` False: the case lies outside the kernel's envelope ('auto' loops, 'kernel' raises)."""
import json
import os
import zlib
from dataclasses import dataclass, field

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VARDIFF = ((0.5, 0), (1.0, 1), (1.5, 2), (2.0, 3))          # (contrast, seed) of create_variable_diffusion_2d_csr
CONVDIFF = ((0.5, 0.25), (0.2, 0.1), (0.8, 0.4), (0.0, 0.0))  # (gamma, delta) of create_convdiff_2d_csr
TOL = {"f64": 1e-8, "f32": 1e-5}
MAX_N, MAX_ROW = 4096, 32


@dataclass
class Case:
    id: str
    solver: str
    dtype: str
    pre: bool
    grid: tuple = None        # (nx, ny), or None for a dense pattern
    dense: str = None         # 'spd1' | 'spd2' | 'spd3' | 'bd-10' | 'bd-11'
    pattern: tuple = None     # ('rag31', n) | ('rag32', n) | ('dense32',) | ('empty', n) of tests/_batch_patterns.py
    transform: str = None     # a key of tests/_order_cases.TRANSFORMS, applied to `pattern`
    S: int = 4
    x0: str = "none"
    kwargs: dict = field(default_factory=dict)
    env: dict = field(default_factory=dict)
    zero_b: int = None        # this system's right-hand side is 0
    kernel: bool = True

    @property
    def path(self):
        return "hipk_%s_batch_kernel<%s,%s>" % ("cg" if self.solver == "cg" else "bi", "double" if self.dtype == "f64" else "float",
                                                "true" if self.pre else "false")

    @property
    def solve_kwargs(self):
        kw = {"tol": TOL[self.dtype]}
        kw.update(self.kwargs)
        return kw


def _c(solver, dtype, pre, grid, S=4, x0="none", tag="", **kw):
    name = f"{solver}{'-jac' if pre else ''}-{dtype}-{grid[0]}x{grid[1]}-S{S}-x0{x0}{tag}"
    return Case(id=name, solver=solver, dtype=dtype, pre=pre, grid=grid, S=S, x0=x0, **kw)


def _p(solver, dtype, pre, pattern, transform, S=4, x0="none", tag="", **kw):
    name = f"{solver}{'-jac' if pre else ''}-{dtype}-{'n'.join(str(v) for v in pattern)}-{transform or 'sorted'}-S{S}-x0{x0}{tag}"
    return Case(id=name, solver=solver, dtype=dtype, pre=pre, pattern=pattern, transform=transform, S=S, x0=x0, **kw)


def _pattern_cases(solver, tol32=None):
    """The pattern axis for one solver: rows of 1 .. 32 entries, unsorted, repeated, a stored zero, an empty row (n = 300: two tiles,
    the second of 44 rows; n = 2049: nine tiles, a second reduction chunk of one row; dense 32: every row at the bound)."""
    kw32 = {} if tol32 is None else {"kwargs": {"tol": tol32}}
    return [
        _p(solver, "f64", False, ("rag31", 300), "dup_shuf"),
        _p(solver, "f64", True, ("rag31", 300), "dup_diag", x0="random"),
        _p(solver, "f32", False, ("rag31", 2049), "shuf", S=5, **kw32),
        _p(solver, "f32", True, ("rag31", 2049), "dup_diag", **kw32),
        _p(solver, "f64", False, ("rag31", 2049), "zero", x0="exact"),
        _p(solver, "f64", True, ("rag31", 2049), "rev"),                    # nnz odd: the padded copy of `values`
        _p(solver, "f64", False, ("rag32", 300), "shuf"),                   # rows of 1 and of 32 entries in one wavefront
        _p(solver, "f64", False, ("dense32",), "rev", S=2),
        _p(solver, "f64", False, ("empty", 300), None, tag="-maxiter4", kwargs={"maxiter": 4}),
        _p(solver, "f64", False, ("dense32",), "dup", S=2, kernel=False),   # 33 entries per row: 'auto' loops, 'kernel' raises
    ]


CASES = [
    # ---- CG and Jacobi PCG on variable diffusion
    _c("cg", "f64", False, (7, 5)), _c("cg", "f64", True, (7, 5), x0="random"), _c("cg", "f32", False, (7, 5), S=5),
    _c("cg", "f64", False, (7, 5), S=1), _c("cg", "f64", False, (7, 5), S=2, x0="exact"),
    _c("cg", "f64", False, (7, 5), S=1030, x0="random"),                      # more workgroups than are resident at four per CU
    _c("cg", "f64", False, (17, 15), S=5, x0="exact"), _c("cg", "f64", True, (16, 16)), _c("cg", "f32", True, (257, 1), x0="random"),
    _c("cg", "f64", False, (257, 1)), _c("cg", "f32", False, (16, 16), x0="exact"),
    _c("cg", "f64", False, (32, 32), S=300), _c("cg", "f32", False, (32, 32)), _c("cg", "f64", True, (32, 32), x0="random"),
    _c("cg", "f32", False, (41, 25), x0="random"), _c("cg", "f32", True, (41, 25)), _c("cg", "f64", False, (41, 25)),
    _c("cg", "f64", False, (45, 45), x0="random"), _c("cg", "f64", True, (64, 32)), _c("cg", "f64", False, (683, 3)),
    _c("cg", "f32", True, (683, 3), x0="exact"), _c("cg", "f32", False, (64, 32)),
    _c("cg", "f64", True, (48, 48), x0="exact"), _c("cg", "f32", False, (48, 48), S=5),
    _c("cg", "f64", False, (64, 64)), _c("cg", "f64", True, (64, 64), x0="random"), _c("cg", "f32", True, (64, 64)),
    _c("cg", "f64", False, (32, 32), x0="exact", tag="-maxiter5", kwargs={"maxiter": 5}),
    _c("cg", "f64", False, (17, 15), tag="-atol", kwargs={"atol": 1e-2}),
    _c("cg", "f64", True, (16, 16), S=5, tag="-b0", zero_b=2),
    # ---- BiCGStab and Jacobi BiCGStab on convection-diffusion
    _c("bicgstab", "f64", False, (7, 5)), _c("bicgstab", "f64", True, (7, 5), S=5, x0="random"), _c("bicgstab", "f32", False, (7, 5), S=2),
    _c("bicgstab", "f64", False, (7, 5), S=1), _c("bicgstab", "f64", False, (7, 5), S=1030),
    _c("bicgstab", "f64", False, (17, 15), x0="exact"), _c("bicgstab", "f32", True, (16, 16)), _c("bicgstab", "f64", True, (257, 1), x0="random"),
    _c("bicgstab", "f64", False, (32, 32), S=300, x0="random"), _c("bicgstab", "f32", False, (32, 32)), _c("bicgstab", "f64", True, (32, 32)),
    _c("bicgstab", "f32", False, (41, 25), x0="random"), _c("bicgstab", "f64", True, (41, 25)),
    _c("bicgstab", "f64", False, (45, 45)), _c("bicgstab", "f32", True, (64, 32), x0="random"), _c("bicgstab", "f64", False, (683, 3), S=5),
    _c("bicgstab", "f64", True, (48, 48)), _c("bicgstab", "f32", False, (48, 48), x0="exact"),
    _c("bicgstab", "f64", False, (64, 64)), _c("bicgstab", "f64", True, (64, 64), x0="random"), _c("bicgstab", "f32", False, (64, 64)),
    _c("bicgstab", "f64", False, (32, 32), x0="exact", tag="-maxiter5", kwargs={"maxiter": 5}),
    _c("bicgstab", "f64", True, (17, 15), tag="-atol", kwargs={"atol": 1e-2}),
    _c("bicgstab", "f64", False, (16, 16), S=5, tag="-b0", zero_b=0),
    # ---- dense patterns: n = 1, 2, 3, and the breakdown fixtures next to a partner that converges
    Case(id="cg-f64-dense1", solver="cg", dtype="f64", pre=False, dense="spd1", S=2),
    Case(id="cg-jac-f64-dense2", solver="cg", dtype="f64", pre=True, dense="spd2", S=2),
    Case(id="cg-f32-dense3", solver="cg", dtype="f32", pre=False, dense="spd3", S=2),
    Case(id="bicgstab-f64-dense1", solver="bicgstab", dtype="f64", pre=False, dense="spd1", S=2),
    Case(id="bicgstab-jac-f64-dense3", solver="bicgstab", dtype="f64", pre=True, dense="spd3", S=2),
    Case(id="bicgstab-f64-bd-10", solver="bicgstab", dtype="f64", pre=False, dense="bd-10", S=2),
    Case(id="bicgstab-f64-bd-11", solver="bicgstab", dtype="f64", pre=False, dense="bd-11", S=2),
    # ---- outside the envelope: 'auto' takes the loop, 'kernel' raises
    _c("cg", "f64", False, (17, 241), S=2, kernel=False, kwargs={"maxiter": 20}),
]
# fp32 BiCGStab on rag31(2049) stagnates above TOL['f32'] on the oracle (relative residuals 1.4e-5 .. 2.8e-5, breakdown -11, info -1);
# at 1e-4 every system of both fp32 cases ends with info 0 and no breakdown (tests/test_batch_cases.py asserts it)
PATTERN_TOL32 = {"cg": None, "bicgstab": 1e-4}
CASES += _pattern_cases("cg", PATTERN_TOL32["cg"]) + _pattern_cases("bicgstab", PATTERN_TOL32["bicgstab"])
PATTERN_CASES = [c for c in CASES if c.pattern]
BY_ID = {c.id: c for c in CASES}
# the cases that also run with HIPK_BATCH_LAUNCH_ITS = 7 and = 1 (every instantiation's save / resume path; > 1 launch each)
BUDGET_IDS = ["cg-f64-7x5-S4-x0none", "cg-jac-f64-16x16-S4-x0none", "cg-f32-41x25-S4-x0random", "cg-jac-f32-41x25-S4-x0none",
              "cg-f64-45x45-S4-x0random", "bicgstab-f64-7x5-S4-x0none", "bicgstab-jac-f64-7x5-S5-x0random",
              "bicgstab-f32-41x25-S4-x0random", "bicgstab-jac-f32-16x16-S4-x0none", "bicgstab-jac-f64-41x25-S4-x0none",
              "bicgstab-f64-16x16-S5-x0none-b0", "cg-f32-48x48-S5-x0none", "bicgstab-jac-f32-64x32-S4-x0random",
              # the pattern axis: a Jacobi case with 32-entry rows and a diagonal stored twice, and n = 2049 (the second chunk)
              "cg-jac-f64-rag31n300-dup_diag-S4-x0random", "cg-f32-rag31n2049-shuf-S5-x0none",
              "bicgstab-jac-f64-rag31n300-dup_diag-S4-x0random", "bicgstab-f32-rag31n2049-shuf-S5-x0none"]


def _np_dtype(case):
    return np.float64 if case.dtype == "f64" else np.float32


def _dense_pattern(n):
    crow = np.arange(0, n * n + 1, n, dtype=np.int32)
    col = np.tile(np.arange(n, dtype=np.int32), n)
    return crow, col


def _partner(n):
    A = 4.0 * np.eye(n) + 0.5 * np.ones((n, n))
    if n > 1:
        A[0, 1] += 0.25
    return A


def build(case):
    """-> dict crow, col (int32), vals (S, nnz), B (S, n), X0 ((S, n) or None), all numpy in the case's dtype."""
    dt = _np_dtype(case)
    rng = np.random.default_rng([zlib.crc32(case.id.encode()), 7])
    if case.pattern:
        from _batch_patterns import build_pattern
        crow, col, vals = build_pattern(case.pattern, case.transform, case.solver, case.S, rng)
        n = crow.size - 1
        B = rng.standard_normal((case.S, n))
    elif case.dense:
        if case.dense.startswith("bd"):
            d = json.load(open(os.path.join(GOLDEN, "bicgstab_breakdown.json")))[case.dense[2:]]
            M0 = np.array(d["A"], dtype=np.float64)
            n = M0.shape[0]
            mats = [M0, _partner(n)]
            B = np.stack([np.array(d["b"], dtype=np.float64), np.arange(1, n + 1, dtype=np.float64)])
        else:
            n = int(case.dense[-1])
            mats = [(3.0 + s) * np.eye(n) + 0.5 * np.ones((n, n)) for s in range(case.S)]
            B = rng.standard_normal((case.S, n))
        crow, col = _dense_pattern(n)
        vals = np.stack([M.reshape(-1) for M in mats])
    else:
        from pytorch_sparse_solver.utils.matrix_utils import create_convdiff_2d_csr, create_variable_diffusion_2d_csr
        nx, ny = case.grid
        if case.solver == "cg":
            four = [create_variable_diffusion_2d_csr(nx, ny, contrast=c, seed=s) for c, s in VARDIFF]
        else:
            four = [create_convdiff_2d_csr(nx, ny, g, d) for g, d in CONVDIFF]
        crow = four[0].crow_indices().numpy().astype(np.int32)
        col = four[0].col_indices().numpy().astype(np.int32)
        for A in four[1:]:
            assert np.array_equal(A.crow_indices().numpy(), crow) and np.array_equal(A.col_indices().numpy(), col), case.id
        vals = np.stack([four[s % 4].values().numpy() for s in range(case.S)])
        n = crow.size - 1
        B = rng.standard_normal((case.S, n))
    vals = np.ascontiguousarray(vals.astype(dt))
    B = np.ascontiguousarray(B.astype(dt))
    S = vals.shape[0]
    assert S == case.S, case.id
    if case.zero_b is not None:
        B[case.zero_b] = 0
    X0 = None
    if case.x0 == "random":
        X0 = np.ascontiguousarray(rng.standard_normal((S, n)).astype(dt))
    elif case.x0 == "exact":
        from oracle import oracle as O
        X0 = np.ascontiguousarray(rng.standard_normal((S, n)).astype(dt))
        e = 1 % S
        B[e] = (O.spmv if case.dtype == "f64" else O.spmv32)(crow, col, vals[e], X0[e])    # then b - A x0 is exactly 0 for system e
    return {"crow": crow, "col": col, "vals": vals, "B": B, "X0": X0, "n": n, "nnz": int(col.size)}


def jacobi_dinv(data):
    """(S, n): reciprocal diagonals in the data's dtype (duplicates add)."""
    crow, col, vals = data["crow"], data["col"], data["vals"]
    n = data["n"]
    rows = np.repeat(np.arange(n), np.diff(crow))
    on = col == rows
    d = np.zeros((vals.shape[0], n), dtype=vals.dtype)
    np.add.at(d, (slice(None), rows[on]), vals[:, on])
    return np.reciprocal(d)


def oracle_run(case, data, O, dinv=None):
    """The oracle's result per system (a list of OracleResult); dinv: the (S, n) Jacobi vectors a preconditioned case uses."""
    f32 = case.dtype == "f32"
    if case.pre:
        fn = {("cg", False): O.pcg_jacobi, ("cg", True): O.pcg_jacobi32, ("bicgstab", False): O.bicgstab_jacobi,
              ("bicgstab", True): O.bicgstab_jacobi32}[(case.solver, f32)]
        if dinv is None:
            dinv = jacobi_dinv(data)
    else:
        fn = {("cg", False): O.cg, ("cg", True): O.cg32, ("bicgstab", False): O.bicgstab, ("bicgstab", True): O.bicgstab32}[(case.solver, f32)]
    out = []
    for s in range(case.S):
        x0 = None if data["X0"] is None else data["X0"][s]
        args = (data["crow"], data["col"], data["vals"][s]) + ((dinv[s],) if case.pre else ()) + (data["B"][s], x0)
        out.append(fn(*args, **case.solve_kwargs))
    return out


_cache = {}


def reference(case, O):
    """build + oracle_run once per case and process (shared by the tests; never modified)."""
    if case.id not in _cache:
        data = build(case)
        _cache[case.id] = (data, oracle_run(case, data, O))
    return _cache[case.id]
