"""The regimes of tests/test_special_cases.py (no GPU), tests/test_gpu_solve_special.py and tests/test_gpu_spmv_special.py: operands
scaled by exact powers of two until a product overflows, underflows or goes subnormal, and right-hand sides that carry a NaN, an
infinity or a chunk of zeros.  The CPU oracle takes one BRANCH per (regime, solver); the branch is written here as a name with a
predicate on an OracleResult, tests/test_special_cases.py checks that the oracle reaches it on every row the GPU test runs, and the
GPU test then asks the kernels for the oracle's bits -- so no GPU case can be vacuous.

This module imports neither torch nor anything that opens a GPU.

Scales are powers of two only: A -> 2^ea A, b -> 2^eb b, x0 -> 2^(eb - ea) x0 are exact (no entry of the tables' matrices or
vectors is so small that 2^-40 .. 2^-400 rounds it, and where a scale does reach the subnormal range that is the point of the
regime).  The Jacobi forms take dinv = 1 / diag of the SCALED matrix, as a caller would."""
import re

import numpy as np

F64, F32 = "f64", "f32"
CH, TILE = 2048, 256
MAXITER_CAP = 12          # CG, BiCGStab: iterations; GMRES: two restart cycles
GMRES_CYCLE_CAP = 2
NAN_MAXITER = 6           # the NaN regime runs into maxiter: keep it short

# ---------------------------------------------------------------------------------------------- branches
# name: predicate(res, plain, x0s, maxiter, k) -- res: the OracleResult of the regime; plain: that of the unscaled run with the
# same cap (None unless the branch compares with it); x0s: the scaled start (zeros when the row has none); k: eb - ea


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else np.int32)


def _same_bits(a, b):
    return a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _multiple(res, plain, x0s, maxiter, k):
    """x is bitwise 2^k times the plain solve's (finite, not all zero) and every count is the plain solve's."""
    want = np.ldexp(plain.x, k).astype(plain.x.dtype)
    return (np.isfinite(res.x).all() and np.any(res.x != 0) and _same_bits(res.x, want) and plain.iterations > 0 and
            (res.iterations, res.matvecs, res.info, res.breakdown) == (plain.iterations, plain.matvecs, plain.info, plain.breakdown))


def _it0(res, plain, x0s, maxiter, k):
    """The stop test held before the first iteration: x is the start, info 0, no breakdown."""
    return res.iterations == 0 and res.info == 0 and res.breakdown == 0 and _same_bits(res.x, x0s)


def _it0_rho(res, plain, x0s, maxiter, k):
    """BiCGStab's absolute rho test fired in the first iteration: breakdown -10, x is the start."""
    return res.iterations == 0 and res.breakdown == -10 and _same_bits(res.x, x0s)


def _nan_maxiter(res, plain, x0s, maxiter, k):
    """No comparison with a NaN holds: the loop runs to maxiter, every entry of x is NaN, info -1."""
    return res.iterations == maxiter and res.info == -1 and np.isnan(res.x).all()


def _nan_gmres(res, plain, x0s, maxiter, k):
    """GMRES: the first Arnoldi step overflows; breakdown 1 after one iteration, every entry of x is NaN."""
    return res.iterations == 1 and res.breakdown == 1 and np.isnan(res.x).all()


def _ordinary(res, plain, x0s, maxiter, k):
    """An ordinary solve: iterations ran, everything finite, x not the start."""
    return res.iterations > 0 and np.isfinite(res.x).all() and not _same_bits(res.x, x0s) and res.breakdown == 0


def _multiple_x(res, plain, x0s, maxiter, k):
    """x is bitwise 2^k times the plain solve's and the iteration and matvec counts are equal; info may differ."""
    want = np.ldexp(plain.x, k).astype(plain.x.dtype)
    return (np.isfinite(res.x).all() and np.any(res.x != 0) and _same_bits(res.x, want) and plain.iterations > 0 and
            (res.iterations, res.matvecs, res.breakdown) == (plain.iterations, plain.matvecs, plain.breakdown))


def _it0_fail(res, plain, x0s, maxiter, k):
    """The stop test held before the first iteration, yet the final residual test fails (dinv is +inf): info -1."""
    return res.iterations == 0 and res.info == -1 and res.breakdown == 0 and _same_bits(res.x, x0s)


BRANCHES = {"multiple": _multiple, "multiple-x": _multiple_x, "it0-info-1": _it0_fail, "it0": _it0, "it0-rho": _it0_rho, "nan-maxiter": _nan_maxiter, "nan-gmres": _nan_gmres,
            "ordinary": _ordinary}
NEEDS_PLAIN = frozenset(["multiple", "multiple-x"])
KINDS = ("cg", "pcg", "bicgstab", "pbicgstab", "gmres", "pgmres")


def B(cg, bi, gm, pcg, pbi, pgm):
    return {"cg": cg, "bicgstab": bi, "gmres": gm, "pcg": pcg, "pbicgstab": pbi, "pgmres": pgm}


MU, MX, I0, RHO, I0F, NANM, NANG, ORD = "multiple", "multiple-x", "it0", "it0-rho", "it0-info-1", "nan-maxiter", "nan-gmres", "ordinary"
# (name, storage type, log2 scale of A, log2 scale of b (x0: the difference), special entries of b, branch per solver)
# special: None | "nan" (one NaN) | "inf" (one +inf) | "zero-chunk" (b zero over the first reduction chunk, or over its first
# half where that is all there is, one of the zeros negative)
#
# Why the Jacobi forms differ from their plain solvers: dinv = 1 / diag(2^ea A) undoes A's scale inside the iteration, so nothing
# overflows in "ap-overflow"; their `info` compares ||M (b - A x)|| with tol ||b||, which is not invariant under a scale of A
# ("multiple-x": the bits of x and the counts, not info); with subnormal diagonals dinv is +inf.
REGIMES = [
    #                                             cg    bicgstab gmres pcg   pbicgstab pgmres
    ("up", F64, -400, 400, None,                B(MU,   MU,   MU,   MU,   MU,   MU)),
    ("down", F64, 40, -70, None,                B(MU,   RHO,  I0,   MX,   RHO,  I0)),
    ("tiny", F64, -300, -300, None,             B(MU,   RHO,  I0,   MU,   RHO,  ORD)),
    ("b-overflow", F64, 0, 520, None,           B(I0,   I0,   I0,   I0,   I0,   I0)),
    ("b-underflow", F64, 0, -540, None,         B(I0,   I0,   I0,   I0,   I0,   I0)),
    ("subnormal", F64, -1040, -1040, None,      B(I0,   I0,   I0,   I0F,  I0F,  NANG)),
    ("ap-overflow", F64, 700, 400, None,        B(NANM, NANM, NANG, MX,   MX,   I0)),
    ("nan-b", F64, 0, 0, "nan",                 B(NANM, NANM, I0,   NANM, NANM, I0)),
    ("inf-b", F64, 0, 0, "inf",                 B(I0,   I0,   I0,   I0,   I0,   I0)),
    ("zero-chunk", F64, 0, 0, "zero-chunk",     B(ORD,  ORD,  ORD,  ORD,  ORD,  ORD)),
    ("up", F32, -40, 40, None,                  B(MU,   MU,   MU,   MU,   MU,   MU)),
    ("subnormal", F32, -140, -140, None,        B(NANM, RHO,  I0,   NANM, RHO,  I0)),
    ("ap-overflow", F32, 70, 60, None,          B(NANM, NANM, MU,   MX,   NANM, I0)),
    ("nan-b", F32, 0, 0, "nan",                 B(NANM, NANM, I0,   NANM, NANM, I0)),
    ("inf-b", F32, 0, 0, "inf",                 B(I0,   I0,   I0,   I0,   I0,   I0)),
    ("zero-chunk", F32, 0, 0, "zero-chunk",     B(ORD,  ORD,  ORD,  ORD,  ORD,  ORD)),
]
# a solver's own exponents where the table's cannot reach the branch: {(solver, regime, storage type): (ea, eb, why)}
_GM_UP = ("GMRES zeroes ||A v||, the Gram-Schmidt coefficients and ||q|| below eps ABSOLUTELY (the reference's _safe_normalize): "
          "with A at 2^-400 (2^-40) the second Gram-Schmidt pass runs where the plain solve skips it; b alone is scaled")
_PRE_UP = "z = dinv r is 2^(eb - ea) r: <r, z> overflows at 2^1200 (fp32 storage: z itself at 2^120 r is fine, info is not invariant); b alone is scaled"
SOLVER_EXPONENTS = {
    ("gmres", "up", F64): (0, 400, _GM_UP), ("gmres", "up", F32): (0, 40, _GM_UP),
    ("pgmres", "up", F64): (0, 400, _GM_UP), ("pgmres", "up", F32): (0, 40, _GM_UP),
    ("pcg", "up", F64): (0, 400, _PRE_UP), ("pcg", "up", F32): (0, 40, _PRE_UP),
    ("pbicgstab", "up", F32): (0, 40, _PRE_UP),
}
REGIME_NAMES = {F64: [r[0] for r in REGIMES if r[1] == F64], F32: [r[0] for r in REGIMES if r[1] == F32]}


def regime(name, dtn):
    for r in REGIMES:
        if r[0] == name and r[1] == dtn:
            return r
    raise KeyError((name, dtn))


# ---------------------------------------------------------------------------------------------- operands of a (row, regime)
def scaled(a, e):
    """2^e a in a's type (exact unless the result leaves the normal range)."""
    return np.ldexp(a, e).astype(a.dtype)


def special_b(b, special):
    """b with the regime's special entries; positions depend on n alone."""
    b = b.copy()
    n = b.size
    if special == "nan":
        b[(2 * n) // 3] = np.nan
    elif special == "inf":
        b[n // 3] = np.inf
    elif special == "zero-chunk":
        m = CH if n > CH else max(1, n // 2)
        b[:m] = 0.0
        b[m // 2] = -0.0
    else:
        assert special is None, special
    return b


def operands(M, b, x0, dinv_wanted, reg, ea=None, eb=None):
    """(values of the scaled matrix, b, x0 or None, dinv or None) of one regime on a row's own M, b, x0 (numpy, the row's storage
    type).  ea / eb: a row's own exponents where the table's do not reach the branch on its matrix."""
    name, dtn, ea0, eb0, special, _ = reg
    ea, eb = ea0 if ea is None else ea, eb0 if eb is None else eb
    vals = scaled(M.data, ea)
    bs = special_b(scaled(b, eb), special)
    x0s = None if x0 is None else scaled(x0, eb - ea)
    dinv = None
    if dinv_wanted:
        diag = scaled(M.diagonal().astype(M.data.dtype), ea).astype(np.float64)
        with np.errstate(divide="ignore", over="ignore"):
            dinv = (1.0 / diag).astype(M.data.dtype)
    return vals, bs, x0s, dinv


def capped(solver, kw):
    """The row's own options with maxiter capped (GMRES: restart cycles)."""
    kw = dict(kw)
    kw["maxiter"] = min(kw["maxiter"], GMRES_CYCLE_CAP if solver in ("gmres", "pgmres") else MAXITER_CAP)
    return kw


def regime_kw(solver, kw, reg):
    kw = capped(solver, kw)
    if reg[0] == "nan-b" and solver not in ("gmres", "pgmres"):
        kw["maxiter"] = min(kw["maxiter"], NAN_MAXITER)
    return kw


ORACLE = {"cg": "cg", "pcg": "pcg_jacobi", "bicgstab": "bicgstab", "pbicgstab": "bicgstab_jacobi", "gmres": "gmres",
          "pgmres": "gmres_jacobi"}


def oracle_solve(oracle, solver, M, vals, dinv, b, x0, kw):
    """The oracle's solve of one (row, regime), as the table tests call it (GMRES with the device's tolerances)."""
    f32 = vals.dtype == np.float32
    fn = getattr(oracle, ORACLE[solver] + ("32" if f32 else ""))
    args = (M.indptr, M.indices, vals) + ((dinv,) if dinv is not None else ()) + (b,)
    okw = dict(x0=x0, tol=kw["tol"], atol=0.0, maxiter=kw["maxiter"])
    if solver in ("gmres", "pgmres"):
        okw.update({k: v for k, v in kw.items() if k in ("restart", "solve_method")}, gpu_tolerances=True)
    n = M.shape[0]
    oracle.set_threads(16 if n >= 100_000 else 4 if n >= 10_000 else 1)   # (the bits do not depend on it)
    try:
        return fn(*args, **okw)
    finally:
        oracle.set_threads(1)


def row_vectors(cid, n, dt, x0kind):
    """b and x0 of a table row as tests/_solve_runner.build_case draws them (x0kind None | "rand")."""
    import zlib
    assert x0kind in (None, "rand"), (cid, x0kind)
    rng = np.random.default_rng(zlib.crc32(cid.encode()))
    x0 = rng.standard_normal(n).astype(dt) if x0kind == "rand" else None
    return rng.standard_normal(n).astype(dt), x0


# ---------------------------------------------------------------------------------------------- rows: the first of every form
MID_KEEP = ("up", "subnormal", "ap-overflow", "nan-b")
ROW_SKIPS = {}   # regimes a row does not run: {(cid, regime): why}, filled by form_rows and below
def family(form):
    """The row of the form table a form belongs to: template arguments stripped (the two-launch CG forms are one)."""
    return re.sub(r"<.*$", "", form)


def form_rows(form_cases, mid_cases):
    """[(cid, solver, matrix key, table, dtype, kw, env, x0kind, path, form)]: for every distinct form of tests/_form_cases.CASES
    and of the mid table (a mid kernel's form is its path), the first row that reports it."""
    seen, rows = set(), []
    for cid, solver, key, dtn, kw, env, x0kind, path, form in form_cases:
        if form not in seen:
            seen.add(form)
            rows.append((cid, solver, key, "form", dtn, kw, env, x0kind, path, form))
    for cid, key, dtn, kw, env, x0kind, path in mid_cases:
        if "_mid_kernel<" in path and " -> " not in path and path not in seen:
            seen.add(path)
            rows.append((cid, cid.split("-")[0], key, "mid", dtn, kw, env, x0kind, path, path))
    # the time budget: the mid table's matrices are the largest (92 k to 524 k rows), and a mid family has up to ten forms per
    # storage type.  The first row of every (solver, family, storage type) runs every regime; the further mid rows of the
    # family keep the regimes in which a NaN meets the loop's own stop and breakdown tests, and the exact multiple
    first = set()
    for r in rows:
        fam = (r[1], family(r[9]), r[4])
        if fam in first and r[3] == "mid":
            for name in REGIME_NAMES[r[4]]:
                if name not in MID_KEEP:
                    ROW_SKIPS[(r[0], name)] = "a further mid row of its family: the first row of the family runs this regime"
        first.add(fam)
    return rows


# a row's own exponents where the table's do not reach the branch on its matrix: {(cid, regime): (ea, eb, why)}
ROW_EXPONENTS = {
    ("pbicgstab-lds-n35-f64", "b-underflow"): (0, -550, "a start is given: r0 = b - A x0 has entries near 2^4, so at 2^-540 <r0, r0> is a "
                                                "nonzero subnormal above atol^2 = 0 and the rho test fires instead; 2^-550 takes it to 0"),
}
# Every regime stays on at least one row of each family of its solver (tests/test_special_cases.py).


def row_regimes(row):
    """[(regime row, ea, eb)] the GPU test runs on `row`."""
    cid, solver, dtn = row[0], row[1], row[4]
    out = []
    for name in REGIME_NAMES[dtn]:
        if (cid, name) in ROW_SKIPS:
            continue
        reg = regime(name, dtn)
        ea, eb = ROW_EXPONENTS.get((cid, name), SOLVER_EXPONENTS.get((solver, name, dtn), (reg[2], reg[3], "")))[:2]
        out.append((reg, ea, eb))
    return out


# ---------------------------------------------------------------------------------------------- SpMV: who a column poisons
def poison(crow, col, columns, n=None, chunk=CH):
    """From the host CSR arrays alone: (rows that store an entry in one of `columns`, the 256-row tiles that hold such rows, the
    reduction chunks of `chunk` rows that hold such rows), each a sorted int64 array."""
    crow, col = np.asarray(crow, dtype=np.int64), np.asarray(col)
    n = len(crow) - 1 if n is None else n
    hit = np.isin(col, np.asarray(list(columns)))
    counts = np.add.reduceat(np.concatenate([hit.astype(np.int64), [0]]), np.minimum(crow[:-1], hit.size))
    counts[np.diff(crow) == 0] = 0
    rows = np.flatnonzero(counts > 0).astype(np.int64)
    return rows, np.unique(rows // TILE), np.unique(rows // chunk)


def poison_columns(n, uniform_tile=None):
    """The columns of step 2 of tests/test_gpu_spmv_special.py: 0, n - 1, the middle of a full tile served from a uniform-tile
    word (uniform_tile: such a tile, or None), the first column of a tile, the last column of the last full tile."""
    full = n // TILE                      # full tiles; the ragged one follows
    cols = [0, n - 1, (full // 3) * TILE, full * TILE - 1]
    if uniform_tile is not None:
        cols.insert(2, uniform_tile * TILE + TILE // 2)
    return cols


BIG_N = 1_000_000


def spmv_poisons(n, uniform_tile):
    """[(column, values)] of one matrix.  The time budget: above a million rows (the 2.2 M-row matrices of the chunk walks) the
    ragged last tile's column n - 1 and the uniform tile's column, with +inf and NaN; every column and -inf on the 70 001-row
    matrices, which reach every kernel family but the chunk walks."""
    cols = poison_columns(n, uniform_tile)
    if n > BIG_N:
        return [(cols[1], ("+inf", "nan")), (cols[2], ("+inf", "nan"))]
    return [(c, ("+inf", "-inf", "nan")) for c in cols]


def spmv_rows(spmv_cases):
    """The cases of tests/_spmv_cases.CASES that tests/test_gpu_spmv_special.py runs: every in-process one (the switches a process
    reads once stay with tests/test_gpu_spmv_instantiations.py), cases of one (matrix, storage type) next to each other."""
    return sorted(n for n, c in spmv_cases.items() if c["fresh"] is None)


def gmres_idle_form(n, kw, env):
    """GMRES tests its start on the host: where the stop test holds at iteration 0 (or cannot fail: a NaN in b) no cycle kernel
    runs, and the solve reports the launch sequence it would have used (the rule of tests/test_form_cases.py, read from
    hipk_gm_path_choose).  Returns that form."""
    g, m = (n + CH - 1) // CH, int(kw.get("restart", 20))
    small = g <= 8 and m <= 31 and "HIPK_GMRES_NO_SMALL" not in env
    wide = small and "HIPK_GMRES_NO_WIDE" not in env
    split = not small and env.get("HIPK_GM_SPLIT_NORM", "0" if g < 1536 else "1") != "0"
    form = ("gmres small + wide" if wide else "gmres small + 256-thread" if small else "gmres restart > 31" if m > 31 else
            "gmres large, first kernels" if "HIPK_GMRES_NO_STREAM" in env else "gmres large, streaming")
    return form + (" + split norm" if split else "") + (", callback M" if kw.get("callback") else "")
