"""Case table of the Chebyshev epilogue tests, shared by tests/test_gpu_chebyshev_kernels.py (the device runs) and
tests/test_chebyshev_cases.py (the same table checked without a GPU): seeded matrices, the inputs of a stand-alone
hipk_cheb_apply, and per case the kernel notes the dispatch of csrc/hipk_api.hip (hipk_launch_spmv) must report, written out
literally."""
import ctypes
import types

import numpy as np
import torch

from _cheb_mirror import coefficients
from test_gpu_coded import banded

N_BIG = 2_200_077     # 8595 tiles of 256 rows, the last of 13 rows; 1075 reduction chunks of 2048 rows, the last ragged
DEGREES = (1, 3, 32)
LMAX, LMIN, SCALE = 2.0, 2.0 / 30, 0.37
STEP64 = " + hipk_cheb_step_kernel<double>"
STEP32 = " + hipk_cheb_step_kernel<float>"

def two_launches(note):
    """The note of the same handle with HIPK_CHEB_FUSED=0: the SpMV's residual form, then hipk_cheb_step_kernel."""
    if note.startswith("hipk_spmv_sell_wide_kernel<"):
        return note.replace(",28,", ",-1,") + STEP64
    if note.startswith("hipk_spmv_cheb_kernel<"):
        t = note[len("hipk_spmv_cheb_kernel<"):].split(",")[0]
        return note.replace("hipk_spmv_cheb_kernel<", "hipk_spmv_kernel<").replace(">", ",true>") + (STEP64 if t == "double" else STEP32)
    return note    # no epilogue: the note is the two-launch form already


# name: offsets; `wide`: the one-launch note of the coded path for the walks (HIPK_SPMV_SELL_STRIDED =) 0 and 1 -- None: the tile
# width is none of 4, 5, 8, the coded path has no epilogue; `plain`: the note with the plain tile kernels
# (set_path(plain_only=True)); with HIPK_CHEB_FUSED=0 the notes are two_launches() of these; `keys`: what the dispatch keys on --
# longest row, largest entry count of a 256-row tile, tile widths before padding, the common width after it
BANDS = {
    "band3": dict(offsets=[-1, 0, 1],
                  wide=("hipk_spmv_sell_wide_kernel<4,28,0>", "hipk_spmv_sell_wide_kernel<4,28,1>"),
                  plain="hipk_spmv_cheb_kernel<double,1280>",
                  keys=dict(max_row=3, max_tile=768, widths={4}, common=4)),
    "band4": dict(offsets=[-1500, -1, 0, 1],
                  wide=("hipk_spmv_sell_wide_kernel<4,28,0>", "hipk_spmv_sell_wide_kernel<4,28,1>"),
                  plain="hipk_spmv_cheb_kernel<double,1280>",
                  keys=dict(max_row=4, max_tile=1024, widths={4}, common=4)),
    "band5": dict(offsets=[-1500, -1, 0, 1, 1500],
                  wide=("hipk_spmv_sell_wide_kernel<5,28,0>", "hipk_spmv_sell_wide_kernel<5,28,1>"),
                  plain="hipk_spmv_cheb_kernel<double,1280>",
                  keys=dict(max_row=5, max_tile=1280, widths={4, 5}, common=5)),
    "band6": dict(offsets=[-1500, -2, -1, 0, 1, 1500],
                  wide=None,
                  plain="hipk_spmv_cheb_kernel<double,2048>",
                  keys=dict(max_row=6, max_tile=1536, widths={5, 6}, common=6)),
    "band7": dict(offsets=[-9000, -1500, -1, 0, 1, 1500, 9000],
                  wide=("hipk_spmv_sell_wide_kernel<8,28,0>", "hipk_spmv_sell_wide_kernel<8,28,1>"),
                  plain="hipk_spmv_cheb_kernel<double,2048>",
                  keys=dict(max_row=7, max_tile=1792, widths={5, 6, 8}, common=8)),
    "band8": dict(offsets=[-9000, -1500, -2, -1, 0, 1, 1500, 9000],
                  wide=("hipk_spmv_sell_wide_kernel<8,28,0>", "hipk_spmv_sell_wide_kernel<8,28,1>"),
                  plain="hipk_spmv_cheb_kernel<double,2048>",                        # 2048 entries per tile: the inclusive edge
                  keys=dict(max_row=8, max_tile=2048, widths={6, 8}, common=8)),
    "band9": dict(offsets=[-9000, -1500, -2, -1, 0, 1, 2, 1500, 9000],
                  wide=None,
                  plain="hipk_spmv_kernel<double,1280,false> + hipk_cheb_step_kernel<double>",   # 2304 per tile: no epilogue
                  keys=dict(max_row=9, max_tile=2304, widths={8, 9}, common=9)),
}

# Masked tiles (HIPK_SPMV_MASKED=1: hipk_tile_masked_kernel) exist only where a row lacks an entry whose column is INSIDE the matrix,
# i.e. at the line ends of a grid; a band has none (its short rows are those whose column falls outside).  Grid stencils, row
# j * nx + i, off-diagonals -1: name: (nx, ny, neighbours (di, dj) in ascending column order, diagonal, notes by walk, tile width)
GRIDS = {
    "grid4_2000x1100": (2000, 1100, [(-1, 0), (0, 0), (1, 0), (0, 1)], 3.5,
                        ("hipk_spmv_sell_wide_kernel<4,28,0>", "hipk_spmv_sell_wide_kernel<4,28,1>"), 4),
    "poisson2000": (2000, 2000, [(0, -1), (-1, 0), (0, 0), (1, 0), (0, 1)], 4.0,
                    ("hipk_spmv_sell_wide_kernel<5,28,0>", "hipk_spmv_sell_wide_kernel<5,28,1>"), 5),
    "tri2048x1152": (2048, 1152, [(-1, -1), (0, -1), (-1, 0), (0, 0), (1, 0), (0, 1), (1, 1)], 6.5,
                     ("hipk_spmv_sell_wide_kernel<8,28,0>", "hipk_spmv_sell_wide_kernel<8,28,1>"), 8),
}

SMALL_OFFSETS = [-40, -1, 0, 1, 40]
SMALL_N_WIDE = 70_001      # 274 tiles, the last of 113 rows; HIPK_SPMV_SELL_STRIDED=1 takes the two-rows-per-lane kernel
SMALL_WIDE = "hipk_spmv_sell_wide_kernel<5,28,1>"
SMALL_NS = (1, 2, 3, 5, 255, 257, 1023)    # no or exactly half of the tiles uniform: bits only

# the README's sizes (profiles/cheb_probe.txt recorded these notes and their two-launch forms)
POISSON_SIZES = {2000: "hipk_spmv_sell_wide_kernel<5,28,0>", 4000: "hipk_spmv_sell_wide_kernel<5,28,1>",
                 8000: "hipk_spmv_sell_wide_kernel<5,28,1>"}

# whole solves: name: (matrix, dtype, solver, degree, keyword arguments, plain CSR kernels only, the step kernel of M(b))
SOLVES = {
    "poisson2000_cg": ("poisson2000", torch.float64, "cg", 3, dict(tol=1e-10, maxiter=40), False,
                       "hipk_spmv_sell_wide_kernel<5,28,0>"),
    "convdiff1500_bicgstab": ("convdiff1500", torch.float64, "bicgstab", 2, dict(maxiter=15), False,
                              "hipk_spmv_sell_wide_kernel<5,28,0>"),
    "convdiff1500_gmres": ("convdiff1500", torch.float64, "gmres", 2, dict(restart=10, maxiter=2), False,
                           "hipk_spmv_sell_wide_kernel<5,28,0>"),
    "tri2048x1152_cg": ("tri2048x1152", torch.float64, "cg", 3, dict(maxiter=30), False,
                        "hipk_spmv_sell_wide_kernel<8,28,0>"),
    "vardiff1200_plain_cg": ("vardiff1200", torch.float64, "cg", 3, dict(maxiter=30), True,
                             "hipk_spmv_cheb_kernel<double,1280>"),
    "poisson1200_f32_plain_cg": ("poisson1200", torch.float32, "cg", 3, dict(tol=1e-4, maxiter=30), True,
                                 "hipk_spmv_cheb_kernel<float,2048>"),
}
# what the dispatch keys on, per solve matrix (uniform: the least share of tiles whose rows all carry one pattern)
SOLVE_KEYS = {
    "poisson2000": dict(max_row=5, max_tile=1280, widths={4, 5}, common=5, coded=True, uniform=0.5),
    "convdiff1500": dict(max_row=5, max_tile=1280, widths={4, 5}, common=5, coded=True, uniform=0.5),
    "tri2048x1152": dict(max_row=7, max_tile=1792, widths={5, 8}, common=8, coded=True, uniform=0.5),
    "vardiff1200": dict(max_row=5, max_tile=1280, widths={4, 5}, common=5, coded=False, uniform=None),
    "poisson1200": dict(max_row=5, max_tile=1280, widths={4, 5}, common=5, coded=True, uniform=None),
}


def band(n, offsets):
    """(crow, col, val, diagonal) of the banded matrix whose k-th off-diagonal is the constant -(1 + 0.25 k) and whose diagonal
    is the constant sum |off-diagonals| + 0.5: at most 9 (offset, value) pairs, first and last rows lacking entries."""
    offsets = sorted(offsets)
    off = [o for o in offsets if o != 0]
    w = {o: -(1.0 + 0.25 * k) for k, o in enumerate(off)}
    diag = sum(-v for v in w.values()) + 0.5
    vals = np.array([diag if o == 0 else w[o] for o in offsets])
    crow, col, val = banded(n, offsets, lambda r, k: vals[k])
    return crow, col, val, diag


def apply_inputs(n, diag, dtype=np.float64):
    """(dinv, r): dinv = u / diag with u uniform in [0.5, 1] -- varying per row, unrelated to 1 / diag --, r standard normal."""
    rng = np.random.default_rng(n)
    dinv = (rng.uniform(0.5, 1.0, n) / diag).astype(dtype)
    r = rng.standard_normal(n).astype(dtype)
    return dinv, r


def apply_coefficients(degree, dinv):
    """(M, coef): the object tests/_cheb_mirror.py: mirror reads and the ctypes array hipk_cheb_apply takes; scale is not 1."""
    c0, c1, c2 = coefficients(LMAX, LMIN, degree)
    M = types.SimpleNamespace(c0=c0, c1=c1, c2=c2, scale=SCALE, degree=degree, dinv=torch.from_numpy(dinv))
    coef = (ctypes.c_double * (2 * degree + 2))(c0, *c1, *c2, SCALE)
    return M, coef


def grid_stencil(nx, ny, steps, diag):
    """(crow, col, val) of a stencil on an nx x ny grid, row j * nx + i: an entry -1 for every neighbour (i + di, j + dj) of `steps`
    (ascending column order) inside the grid, `diag` for (0, 0)."""
    i, j = np.tile(np.arange(nx), ny), np.repeat(np.arange(ny), nx)
    cols = np.stack([(j + dj) * nx + (i + di) for di, dj in steps], axis=1)
    keep = np.stack([(i + di >= 0) & (i + di < nx) & (j + dj >= 0) & (j + dj < ny) for di, dj in steps], axis=1)
    vals = np.broadcast_to(np.array([diag if s == (0, 0) else -1.0 for s in steps]), cols.shape)
    crow = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int64)
    return crow, cols[keep].astype(np.int64), vals[keep].copy()


def grid(name):
    nx, ny, steps, diag, _, _ = GRIDS[name]
    return grid_stencil(nx, ny, steps, diag) + (diag,)


def triangulated(nx, ny):
    """7-point Laplacian of a triangulated nx x ny grid as a torch CSR matrix: the five-point neighbours plus (i - 1, j - 1) and
    (i + 1, j + 1), off-diagonals -1, diagonal 6.5."""
    crow, col, val = grid_stencil(nx, ny, GRIDS["tri2048x1152"][2], 6.5)
    return torch.sparse_csr_tensor(torch.from_numpy(crow), torch.from_numpy(col), torch.from_numpy(val), size=(nx * ny, nx * ny))


def solve_matrix(name):
    from pytorch_sparse_solver.utils import matrix_utils as mu
    return {"poisson2000": lambda: mu.create_poisson_2d_csr(2000, 2000),
            "convdiff1500": lambda: mu.create_convdiff_2d_csr(1500, 1500),
            "tri2048x1152": lambda: triangulated(2048, 1152),
            "vardiff1200": lambda: mu.create_variable_diffusion_2d_csr(1200, 1200, seed=3),
            "poisson1200": lambda: mu.create_poisson_2d_csr(1200, 1200)}[name]()


def dispatch_keys(crow, col, val):
    """What hipk_launch_spmv and the handle's structure analysis key on, recomputed in numpy: the longest row, the largest entry
    count of a 256-row tile, the number of distinct (col - row, value) pairs, every tile's width (hipk_sell_units of its longest
    row), the width all tiles share after the pad-to-largest rule (None: they keep different widths), and the share of tiles whose
    256 rows all carry the same (offset, value) pattern."""
    n = len(crow) - 1
    lens = np.diff(crow)
    ntiles = (n + 255) // 256
    starts = np.arange(ntiles) * 256
    tile_nnz = np.add.reduceat(lens, starts)
    w = np.maximum.reduceat(lens, starts)
    units = 4 * (w // 4 + (w % 4 == 3)) + np.where(w % 4 == 3, 0, w % 4)
    planes, wmax = int(units.sum()), int(units.max())
    common = wmax if (units.min() == wmax or ntiles * wmax <= planes + planes // 50 + 8) else None
    rows = np.repeat(np.arange(n), lens)
    uo, oi = np.unique(col - rows, return_inverse=True)
    uv, vi = np.unique(np.ascontiguousarray(val, dtype=np.float64).view(np.int64), return_inverse=True)   # bit patterns
    uniq, ids = np.unique(oi.reshape(-1).astype(np.int64) * len(uv) + vi.reshape(-1), return_inverse=True)
    # a row's pattern as one number: its pair ids in order, base 257 (exact below 2^64 up to 7 entries, a hash beyond)
    pos = np.arange(len(col)) - np.repeat(crow[:-1], lens)
    term = (ids.reshape(-1).astype(np.uint64) + np.uint64(1)) * np.power(np.uint64(257), pos.astype(np.uint64))
    sig = np.add.reduceat(term, crow[:-1])
    full = n // 256
    uniform = masked = 0
    if full:
        s = sig[:full * 256].reshape(full, 256)
        is_uniform = s.min(axis=1) == s.max(axis=1)
        uniform = int(is_uniform.sum())
        # masked tiles (hipk_tile_masked_kernel): a full tile that is not uniform, whose longest row has at most 7 entries, every row
        # a subsequence of that row's pattern, and every load of the pattern in range for all 256 rows
        if len(uniq) <= 62:
            bits = np.bitwise_or.reduceat(np.uint64(1) << ids.reshape(-1).astype(np.uint64), crow[:-1])[:full * 256].reshape(full, 256)
            ln = lens[:full * 256].reshape(full, 256)
            who = ln.argmax(axis=1)
            pat = bits[np.arange(full), who]
            subset = ((bits & ~pat[:, None]) == 0).all(axis=1)
            off = (col - rows).astype(np.int64)
            omin = np.minimum.reduceat(off, crow[:-1])[:full * 256].reshape(full, 256)[np.arange(full), who]
            omax = np.maximum.reduceat(off, crow[:-1])[:full * 256].reshape(full, 256)[np.arange(full), who]
            t0 = np.arange(full) * 256
            in_range = (t0 + omin >= 0) & (t0 + 255 + omax <= n - 1)
            masked = int((~is_uniform & subset & in_range & (ln.max(axis=1) <= 7)).sum())
    return dict(max_row=int(lens.max()), max_tile=int(tile_nnz.max()), pairs=len(uniq), widths=set(int(u) for u in np.unique(units)),
                common=common, uniform=uniform / ntiles, masked=masked, ntiles=ntiles)
