"""The regime table of tests/_special_cases.py checked without a GPU, so that no case of tests/test_gpu_solve_special.py or
tests/test_gpu_spmv_special.py can be vacuous:

  * on every (row, regime) the GPU test runs, the oracle alone reaches the branch the regime is for (its predicate holds);
  * every solver has every regime of a storage type on a row of each of its form families, every form of the library
    (hipk_solve_form_name) has a row with regimes -- the two forms beyond 384 MiB of vectors excepted, as in
    tests/test_form_cases.py -- and every in-process SpMV case has a row; removing a row is noticed;
  * the oracle takes the REFERENCE's branch in every regime: tests/golden/special_values.json (oracle/gen_golden_special.py ran the
    reference's cg, bicgstab and gmres on the two 35-row band systems) -- same info, operator applications, NaN mask and zero mask
    of x, finite x to the tolerances of tests/test_oracle_golden.py;
  * poison() against a dense restatement."""
import json
import os

import numpy as np
import pytest
import scipy.sparse as sp

import _form_cases as FC
import _special_cases as S
import _spmv_cases as SC
from conftest import GOLDEN


def _mid_table():
    import test_gpu_mid_oracle as MO
    MO._n_cu = FC._n_cu          # 256 compute units where there is no device (the table checks of tests/test_form_cases.py)
    return MO


def _rows():
    return S.form_rows(FC.CASES, _mid_table().CASES)


_mats = {}


def _matrix(table, key):
    if (table, key) not in _mats:
        _mats[(table, key)] = (FC.MATRICES if table == "form" else _mid_table().MATRICES)[key]()
    return _mats[(table, key)]


# ---------------------------------------------------------------------------------------------- every (row, regime) reaches its branch
@pytest.mark.parametrize("row", _rows(), ids=[r[0] for r in _rows()])
def test_oracle_reaches_the_branch_of_every_regime_on_this_row(oracle, row):
    cid, solver, key, table, dtn, kw, env, x0kind, path, form = row
    dt = np.float64 if dtn == S.F64 else np.float32
    M = _matrix(table, key).copy()
    M.data = M.data.astype(dt)
    n = M.shape[0]
    b, x0 = S.row_vectors(cid, n, dt, x0kind)
    pre = solver in ("pcg", "pbicgstab", "pgmres")
    d0 = (1.0 / M.diagonal().astype(np.float64)).astype(dt) if pre else None
    plain = S.oracle_solve(oracle, solver, M, M.data, d0, b, x0, S.capped(solver, kw))
    regimes = S.row_regimes(row)
    assert regimes, cid
    missed = []
    for reg, ea, eb in regimes:
        kwr = S.regime_kw(solver, kw, reg)
        vals, bs, x0s, dinv = S.operands(M, b, x0, pre, reg, ea, eb)
        res = S.oracle_solve(oracle, solver, M, vals, dinv, bs, x0s, kwr)
        start = np.zeros(n, dt) if x0s is None else x0s
        if not S.BRANCHES[reg[5][solver]](res, plain, start, kwr["maxiter"], eb - ea):
            missed.append((reg[0], reg[5][solver], res.iterations, res.matvecs, res.info, res.breakdown, int(np.isnan(res.x).sum())))
    assert not missed, (cid, missed)


# ---------------------------------------------------------------------------------------------- completeness
def _forms():
    import torch  # noqa: F401  (HIP runtime first)
    from pytorch_sparse_solver import _hipk
    return _hipk.solve_forms()


def _missing(rows, skips=None):
    """What the tables lack: forms without a row that runs regimes, and (solver, family, regime) triples without a row."""
    skips = S.ROW_SKIPS if skips is None else skips
    ran = {}
    for r in rows:
        names = [n for n in S.REGIME_NAMES[r[4]] if (r[0], n) not in skips]
        ran.setdefault(r[9], []).extend(names)
    no_row = [f for f in _forms() if not ran.get(f) and f not in FC.UNREACHABLE]
    have = set()
    for r in rows:
        for n in S.REGIME_NAMES[r[4]]:
            if (r[0], n) not in skips:
                have.add((r[1], S.family(r[9]), r[4], n))
    want = set()
    for r in _rows():           # the families of the FULL table: a removed row cannot take its family with it
        for dtn in (S.F64, S.F32):
            if any(q[1] == r[1] and S.family(q[9]) == S.family(r[9]) and q[4] == dtn for q in _rows()):
                want.update((r[1], S.family(r[9]), dtn, n) for n in S.REGIME_NAMES[dtn])
    return no_row, sorted(want - have)


def test_every_form_and_every_family_has_every_regime():
    rows = _rows()
    assert len({r[0] for r in rows}) == len(rows) == len({r[9] for r in rows})
    assert all(r[7] in (None, "rand") for r in rows), [r[0] for r in rows if r[7] not in (None, "rand")]
    assert _missing(rows) == ([], [])
    assert set(FC.UNREACHABLE) <= {"cg three-launch, streams", "cg three-launch, streams + flat direction"}
    # every family of a solver runs the regimes of BOTH storage types where it has kernels of both
    fams = {}
    for r in rows:
        fams.setdefault((r[1], S.family(r[9])), set()).add(r[4])
    kernels = {k: v for k, v in fams.items() if k[1].startswith("hipk_")}
    assert kernels and all(v == {S.F64, S.F32} for v in kernels.values()), {k: v for k, v in kernels.items() if len(v) < 2}
    # overrides name rows and regimes that exist, and say why
    ids = {r[0]: r for r in rows}
    for (cid, name), v in list(S.ROW_EXPONENTS.items()) + list(S.ROW_SKIPS.items()):
        assert cid in ids and name in S.REGIME_NAMES[ids[cid][4]] and (v if isinstance(v, str) else v[2]), (cid, name)
    for (solver, name, dtn), v in S.SOLVER_EXPONENTS.items():
        assert solver in S.KINDS and name in S.REGIME_NAMES[dtn] and v[2]
    for reg in S.REGIMES:
        assert set(reg[5]) == set(S.KINDS) and set(reg[5].values()) <= set(S.BRANCHES), reg[0]


def test_removing_a_row_or_skipping_a_regime_is_noticed():
    rows = _rows()
    for i in (0, len(rows) // 2, len(rows) - 1):
        no_row, no_regime = _missing(rows[:i] + rows[i + 1:])
        assert no_row == [rows[i][9]], rows[i][0]
    # a regime dropped from the only row of a family
    sole = [r for r in rows if sum(1 for q in rows if (q[1], S.family(q[9]), q[4]) == (r[1], S.family(r[9]), r[4])) == 1]
    assert sole
    r = sole[0]
    name = S.REGIME_NAMES[r[4]][0]
    assert _missing(rows, {(r[0], name): "test"})[1] == [(r[1], S.family(r[9]), r[4], name)]


def test_every_in_process_spmv_case_has_a_row():
    import test_gpu_spmv_instantiations as TI          # its own list of the in-process cases, written independently
    rows = S.spmv_rows(SC.CASES)
    want = sorted(TI.IN_PROCESS)
    assert rows == want and len(rows) >= 100
    cut = {n: c for n, c in SC.CASES.items() if n != want[3]}
    assert sorted(set(want) - set(S.spmv_rows(cut))) == [want[3]]
    import test_gpu_spmv_special as TS                 # and the GPU test parametrises from exactly these rows
    assert sorted(TS.IN_PROCESS) == rows
    for n in (SC.N_SMALL, SC.N_BIG):
        ps = S.spmv_poisons(n, (n // S.TILE) // 2)
        assert {c for c, _ in ps} >= {n - 1, ((n // S.TILE) // 2) * S.TILE + S.TILE // 2} and all("+inf" in v and "nan" in v for _, v in ps)
        assert n > S.BIG_N or (len(ps) == 5 and all("-inf" in v for _, v in ps))
    for name in rows:
        n = SC.MATRICES[SC.CASES[name]["matrix"]][0]
        cols = S.poison_columns(n, uniform_tile=5)
        assert len(set(cols)) == 5 and cols[0] == 0 and cols[1] == n - 1 and all(0 <= c < n for c in cols)
        assert cols[3] % S.TILE == 0 and (cols[4] + 1) % S.TILE == 0 and cols[4] + 1 + S.TILE > n - n % S.TILE


# ---------------------------------------------------------------------------------------------- poison()
def test_poison_against_a_dense_restatement():
    rng = np.random.default_rng(5)
    n = 3 * S.TILE + 17
    M = sp.random(n, n, density=0.01, random_state=7, format="csr")
    M = (M + sp.diags(np.ones(n))).tolil()
    M[40, :] = 0            # an empty row
    M = M.tocsr()
    M.eliminate_zeros()
    M.sort_indices()
    D = M.toarray() != 0
    for cols in ([0], [n - 1], [S.TILE], [5, 2 * S.TILE + 3], list(rng.integers(0, n, 4))):
        rows, tiles, chunks = S.poison(M.indptr, M.indices, cols, chunk=512)
        want = np.flatnonzero(D[:, cols].any(axis=1))
        assert np.array_equal(rows, want) and 40 not in rows
        assert np.array_equal(tiles, np.unique(want // S.TILE)) and np.array_equal(chunks, np.unique(want // 512))
    # applied twice: the rows within two stencil reaches
    r1, _, _ = S.poison(M.indptr, M.indices, [7])
    r2, _, _ = S.poison(M.indptr, M.indices, r1)
    assert np.array_equal(r2, np.flatnonzero((D.astype(int) @ D.astype(int))[:, 7] > 0))


# ---------------------------------------------------------------------------------------------- the oracle against the reference
def _golden():
    with open(os.path.join(GOLDEN, "special_values.json")) as f:
        return json.load(f)


def _unhex(a):
    return np.array([float.fromhex(v) for v in a], dtype=np.float64)


def _golden_id(r):
    return f"{r['tag']}-{r['system']}-{r['regime']}"


@pytest.mark.parametrize("r", _golden()["runs"], ids=_golden_id)
def test_oracle_takes_the_reference_branch(oracle, r):
    g = _golden()
    sysd = g["systems"][r["system"]]
    M = sp.csr_matrix((_unhex(sysd["val"]), np.array(sysd["col"]), np.array(sysd["crow"])), shape=(35, 35))
    reg = ("plain", S.F64, 0, 0, None, None) if r["regime"] == "plain" else S.regime(r["regime"], r["dtype"])
    assert r["dtype"] == S.F64 and r["special"] == reg[4]
    vals, b, _, _ = S.operands(M, _unhex(sysd["b"]), None, False, reg, r["ea"], r["eb"])
    res = getattr(oracle, r["solver"])(M.indptr, M.indices, vals, b, **r["kwargs"])     # (the reference ran on the CPU: its tolerances)
    x_ref = _unhex(r["x"])
    assert (res.info, res.matvecs) == (r["info"], r["matvecs"]), (res.info, res.matvecs, r["info"], r["matvecs"])
    assert np.flatnonzero(np.isnan(res.x)).tolist() == r["nan"] == np.flatnonzero(np.isnan(x_ref)).tolist()
    assert np.flatnonzero(res.x == 0).tolist() == r["zero"]
    fin = np.isfinite(x_ref)
    assert np.array_equal(np.isfinite(res.x), fin)
    if fin.any() and np.any(x_ref[fin] != 0):
        k = r["eb"] - r["ea"]           # compare at the plain solve's scale: the norms of x at 2^800 overflow
        a, w = np.ldexp(res.x[fin], -k), np.ldexp(x_ref[fin], -k)
        rel = np.linalg.norm(a - w) / np.linalg.norm(w)
        assert rel < (1e-3 if r["solver"] == "bicgstab" else 1e-8), rel
    # the regime's branch as the table names it, on the reference's own numbers where they suffice (the incremental method stops
    # inside the first cycle of "ap-overflow" with a finite x; the rows of the solve tables are checked one by one above)
    if r["regime"] != "plain" and r["tag"] != "gmres_incremental":
        branch = reg[5][r["solver"]]
        if branch in ("it0", "it0-rho", "it0-info-1"):
            assert r["matvecs"] == 2 and len(r["zero"]) == 35
        elif branch in ("nan-maxiter", "nan-gmres"):
            assert len(r["nan"]) == 35 and r["info"] == -1


def test_the_reference_refuses_fp32_storage():
    """fp32 storage is this project's extension: the reference promotes b to fp64 and refuses an fp32 A, so the fixture
    holds no fp32 run and the fp32 oracle's branches are pinned by the GPU == oracle32 tests alone."""
    g = _golden()
    assert {r["dtype"] for r in g["runs"]} == {S.F64}
    assert g["refused"][S.F32]["runs"] > 0 and g["refused"][S.F32]["errors"]
    names = {(r["tag"], r["system"]) for r in g["runs"]}
    for key in names:
        assert {r["regime"] for r in g["runs"] if (r["tag"], r["system"]) == key} == set(["plain"] + S.REGIME_NAMES[S.F64])
