"""General sparsity patterns for the batch case tables (tests/_batch_cases.py, tests/_gmres_batch_cases.py): rows of 1 to 32 stored
entries side by side, an empty row, descents, repeated columns, a stored zero, a diagonal stored twice.

A case names a pattern -- ('rag31', n) | ('rag32', n) | ('dense32',) | ('empty', n) -- and a transformation of
tests/_order_cases.TRANSFORMS (or None).  The transformation is applied with one seed to every system's values; it reads only
(crow, col, seed), so all S systems keep one pattern and their values are permuted or split identically.  The transformed arrays
ARE the matrices under test.

  rag31(n)   _oracle_cases._band(n, 1..15) (31 entries in an interior row), its upper triangle thinned with a seeded per-row
             probability p = u^2: the pair (i, j) stays with probability 1.2 min(p_i, p_j); rows and columns 5, n // 2 and n - 1 stay
             in full; mirrored.  Row lengths 1 .. 31, some rows hold the diagonal only.  dup_diag, dup_shuf and zero take the full
             rows from 31 to exactly 32.
  rag32(n)   rag31(n) and the pair (n // 2, n // 2 + 16): the full interior row holds 32 entries untransformed, in one wavefront
             with rows that hold the diagonal only.
  dense32    every row 32 entries; 'dup' makes them 33 (outside the envelope).
  empty      rag31(n) with two rows stripped of every stored entry, the diagonal included (symmetric: their columns as well).

Values of rag31 / empty, system s: seeded uniform in [-1, -0.1] (symmetric, or independent upper and lower), diagonal = the row's
absolute off-diagonal sum x (1 + 0.02 s) + 0.05 (s + 1): one pattern, S different conditionings.

This module imports neither torch nor anything that opens a GPU."""
import numpy as np

from _oracle_cases import _band
from _order_cases import TRANSFORMS

FULL_OFFS = range(1, 16)
EMPTY_ROWS = (40, 261)          # one in each 256-row tile of n = 300; neither is a full row


def full_rows(n):
    return (5, n // 2, n - 1)


def rag31(n, seed=31, extra=False):
    """-> (iu, ju): the kept strictly-upper pairs of the symmetric pattern, sorted by (iu, ju); extra: and (n // 2, n // 2 + 16)."""
    U = _band(n, FULL_OFFS).tocoo()
    up = U.row < U.col
    iu, ju = U.row[up].astype(np.int64), U.col[up].astype(np.int64)
    rng = np.random.default_rng([seed, n])
    p = rng.random(n) ** 2
    keep = rng.random(iu.size) < 1.2 * np.minimum(p[iu], p[ju])
    for f in full_rows(n):
        keep |= (iu == f) | (ju == f)
    iu, ju = iu[keep], ju[keep]
    if extra:
        iu, ju = np.append(iu, n // 2), np.append(ju, n // 2 + 16)
    order = np.lexsort((ju, iu))
    return iu[order], ju[order]


def _assemble(n, iu, ju, S, symmetric, rng, no_rows=()):
    """crow, col (sorted rows) and vals (S, nnz) in fp64 of the pattern {(i, j), (j, i), (i, i)} without the rows `no_rows` (and,
    when symmetric, without their columns)."""
    gone = np.zeros(n, dtype=bool)
    gone[list(no_rows)] = True
    if symmetric:
        ok = ~(gone[iu] | gone[ju])
        iu, ju = iu[ok], ju[ok]
    d = np.flatnonzero(~gone)
    r = np.concatenate([iu, ju, d])
    c = np.concatenate([ju, iu, d])
    npair = iu.size
    vals = np.empty((S, r.size))
    for s in range(S):
        up = rng.uniform(-1.0, -0.1, npair)
        lo = up if symmetric else rng.uniform(-1.0, -0.1, npair)
        vals[s, :npair], vals[s, npair:2 * npair] = up, lo
    if not symmetric:
        ok = ~gone[r]
        r, c, vals = r[ok], c[ok], vals[:, ok]
    off = r != c
    for s in range(S):
        rowsum = np.bincount(r[off], weights=np.abs(vals[s, off]), minlength=n)
        vals[s, ~off] = rowsum[r[~off]] * (1.0 + 0.02 * s) + 0.05 * (s + 1)
    order = np.lexsort((c, r))
    crow = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=n))])
    return crow, c[order], np.ascontiguousarray(vals[:, order])


def dense32(solver, S):
    """The dense 32 x 32 pattern: SPD values of the 'spdN' kind for CG, the nonsymmetric dense recipe of gmres_batch otherwise."""
    n = 32
    E = np.ones((n, n))
    skew = 0.0 if solver == "cg" else 0.25 * np.triu(E, 1)
    mats = [(3.0 + s) * np.eye(n) + 0.5 * E + skew for s in range(S)]
    crow = np.arange(0, n * n + 1, n)
    return crow, np.tile(np.arange(n), n), np.stack([M.reshape(-1) for M in mats])


def build_pattern(pattern, transform, solver, S, rng):
    """-> crow, col (int32), vals (S, nnz) fp64: the pattern with the solver's kind of values, transformed."""
    kind = pattern[0]
    if kind == "dense32":
        crow, col, vals = dense32(solver, S)
    else:
        n = pattern[1]
        crow, col, vals = _assemble(n, *rag31(n, extra=kind == "rag32"), S, solver == "cg", rng,
                                    no_rows=EMPTY_ROWS if kind == "empty" else ())
    crow, col = crow.astype(np.int64), col.astype(np.int64)
    if transform is not None:
        out = [TRANSFORMS[transform](crow, col, vals[s], seed=len(kind)) for s in range(S)]
        for c2, j2, _ in out[1:]:
            assert np.array_equal(c2, out[0][0]) and np.array_equal(j2, out[0][1]), (pattern, transform)
        crow, col, vals = out[0][0], out[0][1], np.stack([o[2] for o in out])
    return crow.astype(np.int32), col.astype(np.int32), np.ascontiguousarray(vals)


def sorted_rows(crow, col, vals):
    """The same stored entries with every row in ascending column order (stable: repeated columns keep their order)."""
    rows = np.repeat(np.arange(len(crow) - 1), np.diff(crow))
    order = np.lexsort((np.arange(len(col)), col, rows))
    return crow, np.ascontiguousarray(col[order]), np.ascontiguousarray(vals[:, order])
