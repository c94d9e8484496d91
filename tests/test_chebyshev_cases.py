"""The case table of tests/test_gpu_chebyshev_kernels.py (tests/_cheb_cases.py) is what it claims, checked without a GPU: for
every generated matrix, what the dispatch of csrc/hipk_api.hip keys on -- longest row, entries per 256-row tile (against 1280 and
2048), distinct (offset, value) pairs, tile widths (hipk_sell_units) and the pad-to-largest rule, the share of uniform tiles --
recomputed in numpy and compared with the kernel family each case names.  And what makes the bitwise comparisons of those tests
meaningful: on every stand-alone input an evaluation that contracts d = c1 d + c2 res into one rounding differs from the mirror in
at least 10 % of the entries, and |z| stays below 10."""

import numpy as np
import pytest

import _cheb_cases as C
from _cheb_mirror import mirror


def _check_family(k, case):
    want = case["keys"]
    assert (k["max_row"], k["max_tile"], k["widths"], k["common"]) == (want["max_row"], want["max_tile"], want["widths"], want["common"]), k
    assert k["pairs"] <= 9                                                   # <= 256: the CODED path
    # the two-rows-per-lane kernel: a common width of 4, 5 or 8 and at least half of the tiles uniform
    wide = k["common"] in (4, 5, 8) and k["uniform"] >= 0.5
    assert wide == (case["wide"] is not None), k
    if wide:
        for s in (0, 1):
            assert case["wide"][s] == f"hipk_spmv_sell_wide_kernel<{k['common']},28,{s}>"
            assert C.two_launches(case["wide"][s]) == f"hipk_spmv_sell_wide_kernel<{k['common']},-1,{s}>" + C.STEP64
    # the plain tile kernel's Chebyshev twins: rows of at most 32 entries, at most 1280 / 2048 entries per tile
    cap = 1280 if k["max_tile"] <= 1280 else 2048 if k["max_tile"] <= 2048 else None
    if cap is None:
        assert case["plain"] == C.two_launches(case["plain"]) == "hipk_spmv_kernel<double,1280,false>" + C.STEP64
    else:
        assert case["plain"] == f"hipk_spmv_cheb_kernel<double,{cap}>"
        assert C.two_launches(case["plain"]) == f"hipk_spmv_kernel<double,{cap},true>" + C.STEP64


def _contracted(oracle, crow, col, val, M, r, dtype=np.float64):
    """The mirror with d = c1 * d + c2 * res rounded ONCE (what an fma or a contracted expression gives): evaluated in
    np.longdouble for fp64, in float64 for fp32 (where the two products are exact), then rounded to the working type."""
    f, L = dtype, (np.longdouble if dtype == np.float64 else np.float64)
    spmv = oracle.spmv if dtype == np.float64 else oracle.spmv32
    dinv = M.dinv.numpy()
    d = f(M.c0) * (dinv * r)
    z = d
    for k in range(M.degree):
        res = dinv * spmv(crow, col, val, z, bsub=r)
        d = (L(f(M.c1[k])) * d.astype(L) + L(f(M.c2[k])) * res.astype(L)).astype(f)
        z = z + d
    return f(M.scale) * z


def _check_sensitive(oracle, cid, crow, col, val, diag, dtype=np.float64):
    """On this input a contracted step differs from the mirror in at least 10 % of the entries, and |z| stays below 10."""
    dinv, r = C.apply_inputs(len(crow) - 1, diag, dtype)
    val = val.astype(dtype)
    for degree in C.DEGREES:
        M, _ = C.apply_coefficients(degree, dinv)
        z = mirror(oracle, crow, col, val, M, r, dtype=dtype)
        zc = _contracted(oracle, crow, col, val, M, r, dtype)
        assert z.dtype == zc.dtype == dtype
        differ = float(np.mean(z != zc))
        print(f"{cid} degree {degree}: max |z| {np.abs(z).max():.3g}, a contracted step differs in {100 * differ:.1f} % of the entries")
        assert np.isfinite(z).all() and np.abs(z).max() < 10.0
        assert differ >= 0.10


@pytest.mark.parametrize("name", sorted(C.BANDS))
def test_band_cases_name_the_family_the_dispatch_takes(oracle, name):
    assert np.finfo(np.longdouble).nmant > 60
    case = C.BANDS[name]
    crow, col, val, diag = C.band(C.N_BIG, case["offsets"])
    k = C.dispatch_keys(crow, col, val)
    print(name, k)
    assert k["ntiles"] == 8595 and C.N_BIG - 256 * 8594 == 13 and oracle.chunk_geom(C.N_BIG) == (2048, 1075)
    _check_family(k, case)
    assert k["uniform"] >= 0.99                                              # all but the tiles at the band's ends
    assert k["masked"] == 0      # a band's short rows lack entries OUTSIDE the matrix: HIPK_SPMV_MASKED finds nothing here (GRIDS)
    # (the oracle's thread count is left alone: setting it sets the OpenMP thread count of the whole process, torch's included)
    _check_sensitive(oracle, name, crow, col, val, diag)
    if name == "band5":          # the fp32 input of the plain tile kernel
        _check_sensitive(oracle, name + " f32", crow, col, val, diag, dtype=np.float32)


@pytest.mark.parametrize("name", sorted(C.GRIDS))
def test_grid_cases_have_masked_tiles(oracle, name):
    """The matrices of the HIPK_SPMV_MASKED=1 runs: line ends inside the matrix, so tiles that are not uniform but whose rows are
    subsequences of one pattern exist; the count computed here is what the GPU test reads back from the handle's byte count."""
    nx, ny, steps, diag, notes, width = C.GRIDS[name]
    crow, col, val, _ = C.grid(name)
    k = C.dispatch_keys(crow, col, val)
    print(name, k)
    assert k["pairs"] == len(steps) and k["max_row"] == len(steps) <= 7 and k["common"] == width
    assert k["uniform"] >= 0.5 and k["masked"] >= 0.1 * k["ntiles"]
    ch, chunks = oracle.chunk_geom(nx * ny)
    assert ch == 2048 and 512 <= chunks <= 2048                  # a workgroup per chunk by default (walk 0)
    assert notes == tuple(f"hipk_spmv_sell_wide_kernel<{width},28,{s}>" for s in (0, 1))
    _check_sensitive(oracle, name, crow, col, val, diag)


@pytest.mark.parametrize("n", (C.SMALL_N_WIDE,) + C.SMALL_NS)
def test_small_cases(oracle, n):
    crow, col, val, diag = C.band(n, C.SMALL_OFFSETS)
    k = C.dispatch_keys(crow, col, val)
    print(n, k)
    assert k["pairs"] <= 5 and k["max_row"] <= 5 and k["max_tile"] <= 1280
    if n == C.SMALL_N_WIDE:                       # the two-rows-per-lane kernel when the grouped walk is forced
        _check_sensitive(oracle, f"n={n}", crow, col, val, diag)
        assert (k["ntiles"], n - 273 * 256) == (274, 113)
        assert (k["max_tile"], k["widths"], k["common"]) == (1280, {5}, 5) and k["uniform"] >= 0.99
        assert C.SMALL_WIDE == "hipk_spmv_sell_wide_kernel<5,28,1>" and C.two_launches(C.SMALL_WIDE) == "hipk_spmv_sell_wide_kernel<5,-1,1>" + C.STEP64
    elif n == 1023:
        assert (k["max_tile"], k["widths"], k["common"], k["uniform"]) == (1280, {5}, 5, 0.5)
    elif n == 257:
        assert (k["max_tile"], k["widths"], k["common"], k["uniform"]) == (1200, {4, 5}, 5, 0.0)
    else:                                         # one tile, not uniform: the issue of which kernel runs is left to the library
        assert k["ntiles"] == 1 and k["uniform"] == 0.0


@pytest.mark.parametrize("name", sorted(C.SOLVE_KEYS))
def test_solve_matrices(oracle, name):
    A = C.solve_matrix(name)
    want = C.SOLVE_KEYS[name]
    k = C.dispatch_keys(A.crow_indices().numpy(), A.col_indices().numpy(), A.values().numpy())
    print(name, k)
    assert (k["max_row"], k["max_tile"], k["widths"], k["common"]) == (want["max_row"], want["max_tile"], want["widths"], want["common"]), k
    assert (k["pairs"] <= 256) == want["coded"]
    if want["uniform"] is not None:
        assert k["uniform"] >= want["uniform"]
    for cid, (matrix, dtype, solver, degree, kw, plain, note) in C.SOLVES.items():
        if matrix != name:
            continue
        if plain:      # the tile kernel's twin: fp64 by entries per tile, fp32 always <float,2048>
            t, cap = ("double", 1280 if k["max_tile"] <= 1280 else 2048) if "f32" not in cid else ("float", 2048)
            assert k["max_tile"] <= 2048 and note == f"hipk_spmv_cheb_kernel<{t},{cap}>", cid
        else:          # a workgroup per chunk of 2048 rows: between a quarter of 256 x 8 workgroup slots and all of them
            ch, chunks = oracle.chunk_geom(A.shape[0])
            assert ch == 2048 and 512 <= chunks <= 2048, cid
            assert k["uniform"] >= 0.5 and note == f"hipk_spmv_sell_wide_kernel<{k['common']},28,0>", cid
