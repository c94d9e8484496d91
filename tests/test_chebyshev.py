"""ChebyshevPreconditioner on CPU tensors: coefficients, errors, the apply bit for bit against a numpy mirror, the operator's
spectrum, the generic solver path against the reference's own runs (tests/golden/cheb_*.npz, tools/gen_golden_cheb.py: the
reference's cg / bicgstab / gmres with M = a torch closure of the documented apply), and the iteration counts it buys."""
import math

import numpy as np
import pytest
import torch

from conftest import BICGSTAB_MATVEC_BAND, load_case
from _cheb_mirror import coefficients, csr, mirror, rid, runs, scale_of

CASES = sorted({r["case"] for r in runs()})


def _gershgorin(d):
    crow, val = d["crow"].astype(np.int64), d["val"]
    return float((np.add.reduceat(np.abs(val), crow[:-1]) * d["dinv"]).max()), float(d["dinv"].max())


# ---------------------------------------------------------------------------------------------- 1. coefficients and errors
@pytest.mark.parametrize("degree", [1, 3, 6, 32])
@pytest.mark.parametrize("case", ["cheb_poisson_17x13", "cheb_vardiff_nx32"])
def test_coefficients_follow_the_recurrence(case, degree):
    from pytorch_sparse_solver.module_a import ChebyshevPreconditioner
    d = load_case(case)
    A = csr(d)
    M = ChebyshevPreconditioner(A, degree=degree)
    bound, dinv_max = _gershgorin(d)
    assert M.lmax == pytest.approx(bound, rel=1e-14) and M.lmin == M.lmax / 30.0
    assert np.array_equal(M.dinv.numpy(), 1.0 / np.diag(A.to_dense().numpy()))
    c0, c1, c2 = coefficients(M.lmax, M.lmin, degree)
    assert M.c0 == c0 and list(M.c1) == c1 and list(M.c2) == c2 and len(M.c1) == len(M.c2) == degree
    assert M.scale == scale_of(M.lmax, M.lmin, degree, dinv_max) and 0.0 < M.scale < 1.0
    raw = ChebyshevPreconditioner(A, degree=degree, lmax=3.0, lmin=0.5, normalize=False)
    assert raw.scale == 1.0 and (raw.lmax, raw.lmin) == (3.0, 0.5)
    assert (raw.c0, list(raw.c1), list(raw.c2)) == coefficients(3.0, 0.5, degree)
    assert ChebyshevPreconditioner(A, ratio=10.0).lmin == M.lmax / 10.0


def test_poisson_gershgorin_bound_is_two():
    from pytorch_sparse_solver.module_a import ChebyshevPreconditioner
    from pytorch_sparse_solver.utils.matrix_utils import create_poisson_2d_csr, create_poisson_2d_sparse_coo
    for A in (create_poisson_2d_csr(9, 7), create_poisson_2d_sparse_coo(9, 7), create_poisson_2d_csr(9, 7).to_dense()):
        M = ChebyshevPreconditioner(A)
        assert M.lmax == 2.0 and M.degree == 3 and M.shape == (63, 63) and M.applies == 0 and M.spmvs == 0


def test_errors():
    from pytorch_sparse_solver.module_a import ChebyshevPreconditioner
    from pytorch_sparse_solver.utils.matrix_utils import create_poisson_2d_csr
    A = create_poisson_2d_csr(6, 5)
    for degree in (0, 33):
        with pytest.raises(ValueError, match="degree"):
            ChebyshevPreconditioner(A, degree=degree)
    for lmin, lmax in ((2.0, 2.0), (3.0, 2.0), (0.0, 2.0), (-1.0, 2.0)):
        with pytest.raises(ValueError, match="lmin"):
            ChebyshevPreconditioner(A, lmin=lmin, lmax=lmax)
    D = A.to_dense().clone()
    for bad in (0.0, -4.0):
        D[3, 3] = bad
        with pytest.raises(ValueError, match="diagonal"):
            ChebyshevPreconditioner(D)
    with pytest.raises(ValueError, match="square"):
        ChebyshevPreconditioner(torch.zeros(3, 4, dtype=torch.float64))
    M = ChebyshevPreconditioner(A)
    for v in (torch.zeros(29, dtype=torch.float64), torch.zeros(30, 1, dtype=torch.float64), torch.zeros(31, dtype=torch.float64)):
        with pytest.raises(ValueError, match="shape"):
            M(v)
    assert M.applies == 0

    class FakeRowBlock:                      # what distributed.RowBlockCSR announces itself with
        _hipk_row_block = True
        shape = (30, 30)
    with pytest.raises(ValueError, match="RowBlockCSR"):
        ChebyshevPreconditioner(FakeRowBlock())


def test_row_block_csr_is_refused():
    from pytorch_sparse_solver.distributed import RowBlockCSR
    from pytorch_sparse_solver.module_a import ChebyshevPreconditioner
    assert RowBlockCSR._hipk_row_block is True
    with pytest.raises(ValueError, match="RowBlockCSR"):
        ChebyshevPreconditioner(object.__new__(RowBlockCSR))


# ---------------------------------------------------------------------------------------------- 2. CPU apply == mirror
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("degree", [1, 3, 6])
@pytest.mark.parametrize("case", CASES)
def test_cpu_apply_equals_numpy_mirror_bitwise(oracle, case, degree, normalize):
    from pytorch_sparse_solver.module_a import ChebyshevPreconditioner
    d = load_case(case)
    M = ChebyshevPreconditioner(csr(d), degree=degree, normalize=normalize)
    for r in (d["b"], np.random.default_rng(degree).standard_normal(int(d["n"]))):
        z = M(torch.from_numpy(r)).numpy()
        assert np.array_equal(z, mirror(oracle, d["crow"], d["col"], d["val"], M, r))
    assert (M.applies, M.spmvs) == (2, 2 * degree)


def test_cpu_apply_long_rows_and_fp32(oracle):
    """A dense SPD matrix (rows of 100 > 32 entries: the strided long-row summation) and fp32 arithmetic."""
    from pytorch_sparse_solver.module_a import ChebyshevPreconditioner
    rng = np.random.default_rng(7)
    G = rng.standard_normal((100, 100))
    Ad = G @ G.T + 100 * np.eye(100)
    A = torch.from_numpy(Ad)
    S = A.to_sparse_csr()
    crow, col, val = S.crow_indices().numpy(), S.col_indices().numpy(), S.values().numpy()
    r = rng.standard_normal(100)
    M = ChebyshevPreconditioner(A, degree=4)
    assert np.array_equal(M(torch.from_numpy(r)).numpy(), mirror(oracle, crow, col, val, M, r))
    M32 = ChebyshevPreconditioner(A.to(torch.float32), degree=4)
    z32 = M32(torch.from_numpy(r.astype(np.float32)))
    assert z32.dtype == torch.float32
    assert np.array_equal(z32.numpy(), mirror(oracle, crow, col, val.astype(np.float32), M32, r, dtype=np.float32))


# ---------------------------------------------------------------------------------------------- 3. the operator is what it claims
@pytest.mark.parametrize("degree", [1, 3, 6])
def test_operator_is_spd_bounded_and_clusters_the_spectrum(degree):
    from pytorch_sparse_solver.module_a import ChebyshevPreconditioner
    d = load_case("cheb_poisson_17x13")
    A = csr(d)
    Ad = A.to_dense().numpy()
    n = Ad.shape[0]

    def matrix_of(M):
        return np.stack([M(torch.from_numpy(e)).numpy() for e in np.eye(n)], axis=1)

    Mn = matrix_of(ChebyshevPreconditioner(A, degree=degree))
    assert np.abs(Mn - Mn.T).max() <= 1e-12 * np.abs(Mn).max()
    ev = np.linalg.eigvalsh((Mn + Mn.T) / 2)
    assert ev.min() > 0.0 and ev.max() <= 1.0 + 1e-12
    s = 1.0 / np.sqrt(np.diag(Ad))
    lam = np.linalg.eigvalsh(s[:, None] * Ad * s[None, :])
    lmin, lmax = float(lam[0]), float(lam[-1])
    Mr = matrix_of(ChebyshevPreconditioner(A, degree=degree, lmin=lmin, lmax=lmax, normalize=False))
    assert np.abs(Mr - Mr.T).max() <= 1e-12 * np.abs(Mr).max() and np.linalg.eigvalsh((Mr + Mr.T) / 2).min() > 0.0
    mu = np.linalg.eigvals(Mr @ Ad)          # similar to a symmetric matrix: real
    assert np.abs(mu.imag).max() <= 1e-10
    eps = 1.0 / math.cosh(degree * math.acosh((lmax + lmin) / (lmax - lmin)))
    assert mu.real.min() >= 1.0 - eps - 1e-10 and mu.real.max() <= 1.0 + eps + 1e-10


# ---------------------------------------------------------------------------------------------- 4. generic path vs the reference
@pytest.mark.parametrize("r", runs(), ids=rid)
def test_generic_path_matches_reference(r):
    from pytorch_sparse_solver.module_a import ChebyshevPreconditioner, bicgstab, cg, get_last_stats, gmres
    d = load_case(r["case"])
    A = csr(d)
    M = ChebyshevPreconditioner(A, degree=r["degree"], normalize=r["normalize"])
    assert M.lmax == pytest.approx(r["lmax"], rel=1e-14)
    assert np.allclose([M.c0, *M.c1, *M.c2, M.scale], [r["c0"], *r["c1"], *r["c2"], r["scale"]], rtol=1e-13, atol=0.0)
    x0 = torch.from_numpy(d["x0"]) if r["has_x0"] else None
    x, info = {"cg": cg, "bicgstab": bicgstab, "gmres": gmres}[r["solver"]](A, torch.from_numpy(d["b"]), x0=x0, M=M, **r["kwargs"])
    st = get_last_stats()
    x_ref = d[r["tag"] + "_x"]
    assert info == r["info"]
    if r["solver"] == "bicgstab":
        assert abs(st.matvecs - r["matvecs"]) <= max(2, BICGSTAB_MATVEC_BAND * r["matvecs"])
        assert np.linalg.norm(x.numpy() - x_ref) <= 1e-5 * np.linalg.norm(x_ref)
    else:
        assert st.matvecs == r["matvecs"]
        assert np.linalg.norm(x.numpy() - x_ref) <= 1e-8 * np.linalg.norm(x_ref)
    assert M.spmvs == r["degree"] * M.applies and M.applies > 0


def test_fixtures_hold_a_converged_solve_the_reference_calls_failed():
    """normalize=False reproduces the reference's rule: info = -1 although the true residual is below tol ||b||."""
    hit = [r for r in runs() if r["solver"] == "cg" and not r["normalize"] and r["info"] == -1 and r["relres"] <= r["kwargs"]["tol"]]
    assert hit, "no unscaled run with the reference's info = -1 at a converged true residual"


# ---------------------------------------------------------------------------------------------- 5. it lowers the iteration count
def _counts(A, tol=1e-6):
    from pytorch_sparse_solver.module_a import ChebyshevPreconditioner, JacobiPreconditioner, cg, get_last_stats
    b = torch.ones(A.shape[0], dtype=torch.float64)
    _, info_j = cg(A, b, tol=tol, M=JacobiPreconditioner(A))
    its_j = get_last_stats().iterations
    M = ChebyshevPreconditioner(A)
    x, info = cg(A, b, tol=tol, M=M)
    its = get_last_stats().iterations
    Mr = ChebyshevPreconditioner(A, normalize=False)
    xr, info_r = cg(A, b, tol=tol, M=Mr)
    its_r = get_last_stats().iterations
    relres = lambda v: float(torch.linalg.norm(b - torch.mv(A.to_dense(), v)) / torch.linalg.norm(b))   # noqa: E731
    print(f"jacobi {its_j} its (info {info_j}) | chebyshev(3) {its} its (info {info}, relres {relres(x):.3e}) | "
          f"unscaled {its_r} its (info {info_r}, relres {relres(xr):.3e})")
    assert info_j == 0 and info == 0
    assert its <= 0.35 * its_j
    assert (M.degree + 1) * its <= 1.25 * its_j
    assert abs(its_r - its) <= 1 and relres(xr) <= tol and relres(x) <= tol
    return its_j, its, info_r


def test_iteration_count_poisson_200():
    from pytorch_sparse_solver.utils.matrix_utils import create_poisson_2d_csr
    _counts(create_poisson_2d_csr(200, 200))


def test_iteration_count_variable_diffusion_128():
    from pytorch_sparse_solver.utils.matrix_utils import create_variable_diffusion_2d_csr
    _counts(create_variable_diffusion_2d_csr(128, 128))
