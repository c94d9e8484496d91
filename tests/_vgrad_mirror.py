"""The matrix gradient of a solve, written out: for every stored entry k of a CSR matrix, in row r and column col[k],

    G[k] = -(lam[r] * x[col[k]])

one multiplication in the dtype of the matrix values (lam and x are cast to it first), then a negation.  `grad_values` is the scalar
loop over rows and their entries in numpy scalars of that dtype; it knows nothing of the product's torch expression
(module_a/matrix_grad.py) or kernel (csrc/hipk_vgrad.hip).  `grad_values_rows` is the same formula with the inner loop as one numpy
slice per non-empty run of rows, for the cases whose millions of entries the scalar loop would take minutes over;
tests/test_matrix_grad.py pins it to the scalar loop bit for bit.

This module imports neither torch nor anything that opens a GPU."""
import numpy as np


def grad_values(crow, col, lam, x, dtype):
    """crow (n + 1,), col (nnz,) integers; lam (n_rows,), x (n_cols,) any float arrays -> G (nnz,) of `dtype`."""
    dt = np.dtype(dtype).type
    crow, col = np.asarray(crow), np.asarray(col)
    out = np.empty(len(col), dtype=dtype)
    with np.errstate(invalid="ignore", over="ignore"):        # inf * 0 and NaN operands are cases, not mistakes
        for r in range(len(crow) - 1):
            lr = dt(lam[r])
            for k in range(int(crow[r]), int(crow[r + 1])):
                p = lr * dt(x[int(col[k])])
                out[k] = -p
    return out


def grad_values_rows(crow, col, lam, x, dtype):
    """The same values: every entry's row taken from the row lengths, the product and the negation as array operations in `dtype`."""
    crow, col = np.asarray(crow).astype(np.int64), np.asarray(col).astype(np.int64)
    lam, x = np.asarray(lam).astype(dtype), np.asarray(x).astype(dtype)
    rows = np.repeat(np.arange(len(crow) - 1), np.diff(crow))
    with np.errstate(invalid="ignore", over="ignore"):
        p = lam[rows] * x[col]
    return np.negative(p)


def batch_grad_values(crow, col, Lam, X, dtype, fast=False):
    """(S, nnz): the formula for every system of a batch on one pattern."""
    f = grad_values_rows if fast else grad_values
    return np.stack([f(crow, col, Lam[s], X[s], dtype) for s in range(len(Lam))])
