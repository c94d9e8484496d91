"""ChebyshevPreconditioner on the device: hipk_cheb_apply bit for bit against the numpy mirror (tests/_cheb_mirror.py) in both of
its forms -- one launch per step (the SpMV kernels' Chebyshev epilogue) and SpMV + hipk_cheb_step_kernel -- with the form that ran
asserted from the kernel note; whole cg / bicgstab / gmres solves against the reference's runs (tests/golden/cheb_*.npz); one
large solve for the stop logic.  The epilogue kernels one by one -- every instantiation at ragged sizes, the README's sizes, whole
solves in which an epilogue kernel runs -- are in tests/test_gpu_chebyshev_kernels.py."""
import numpy as np
import pytest
import torch

from conftest import BICGSTAB_MATVEC_BAND, load_case
from _cheb_mirror import csr, mirror, rid, runs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DEGREES = [1, 3, 6, 32]
STEP = "hipk_cheb_step_kernel"


def _poisson(nx, ny):
    from pytorch_sparse_solver.utils.matrix_utils import create_poisson_2d_csr
    return create_poisson_2d_csr(nx, ny)


def _vardiff(nx, ny):
    from pytorch_sparse_solver.utils.matrix_utils import create_variable_diffusion_2d_csr
    return create_variable_diffusion_2d_csr(nx, ny, seed=3)


def _arrow(nx):
    """Poisson with a first row / column of 100 entries: one row beyond the 32 a lane sums (the tile kernel's general path)."""
    A = _poisson(nx, nx).to_dense()
    A[0, 3:100] = -0.01
    A[3:100, 0] = -0.01
    return A.to_sparse_csr()


def _dense_spd(n):
    g = torch.Generator().manual_seed(n)
    G = torch.randn(n, n, dtype=torch.float64, generator=g)
    return (G @ G.T + n * torch.eye(n, dtype=torch.float64)).to_sparse_csr()


# name: (builder, dtype, plain CSR kernels only, HIPK_SPMV_SELL_STRIDED or None, the kernel note of the one-launch form -- None: this
# SpMV family has no Chebyshev epilogue and both settings of HIPK_CHEB_FUSED run SpMV + hipk_cheb_step_kernel)
CONFIGS = {
    "poisson1024_wide": (lambda: _poisson(1024, 1024), torch.float64, False, None, "hipk_spmv_sell_wide_kernel<5,28,0>"),
    "poisson1024_wide_groups": (lambda: _poisson(1024, 1024), torch.float64, False, "1", "hipk_spmv_sell_wide_kernel<5,28,1>"),
    "poisson1024_plain": (lambda: _poisson(1024, 1024), torch.float64, True, None, "hipk_spmv_cheb_kernel<double,1280>"),
    "poisson1000x1003_ragged": (lambda: _poisson(1000, 1003), torch.float64, True, None, "hipk_spmv_cheb_kernel<double,1280>"),
    "vardiff300_offset_coded": (lambda: _vardiff(300, 300), torch.float64, False, None, None),
    "vardiff300_plain": (lambda: _vardiff(300, 300), torch.float64, True, None, "hipk_spmv_cheb_kernel<double,1280>"),
    "arrow40_long_row": (lambda: _arrow(40), torch.float64, False, None, None),
    "dense200_rowwave": (lambda: _dense_spd(200), torch.float64, False, None, None),
    "poisson300x200_f32_coded": (lambda: _poisson(300, 200), torch.float32, False, None, None),
    "poisson300x200_f32_plain": (lambda: _poisson(300, 200), torch.float32, True, None, "hipk_spmv_cheb_kernel<float,2048>"),
    "vardiff131_f32_plain": (lambda: _vardiff(131, 131), torch.float32, True, None, "hipk_spmv_cheb_kernel<float,2048>"),
}


def _check_apply(hipk, oracle, monkeypatch, A, dtype, plain, strided, fused_note, degrees=DEGREES):
    from pytorch_sparse_solver.module_a import ChebyshevPreconditioner
    if strided is not None:
        monkeypatch.setenv("HIPK_SPMV_SELL_STRIDED", strided)
    A = A.to(dtype)
    n = A.shape[0]
    crow, col, val = A.crow_indices().numpy(), A.col_indices().numpy(), A.values().numpy()
    Ad = A.to(DEV)
    h = hipk.CsrHandle(Ad.crow_indices(), Ad.col_indices(), Ad.values(), A.shape)   # a handle of its own: set_path, plan cache
    h.set_path(plain_only=plain)
    npdt = np.float64 if dtype == torch.float64 else np.float32
    r = np.random.default_rng(n).standard_normal(n).astype(npdt)
    rd = torch.from_numpy(r).to(DEV)
    for degree in degrees:
        for normalize in ((True, False) if degree == 3 else (True,)):
            M = ChebyshevPreconditioner(A, degree=degree, normalize=normalize)       # coefficients and dinv
            ref = mirror(oracle, crow, col, val, M, r, dtype=npdt)
            dinv = M.dinv.to(DEV)
            for fused in ("1", "0"):
                monkeypatch.setenv("HIPK_CHEB_FUSED", fused)
                z = hipk.cheb_apply(h, degree, dinv, M._coef, rd)
                note = hipk.CsrHandle.last_spmv_kernel()
                if fused == "1" and fused_note is not None:
                    assert note == fused_note, note
                else:
                    assert note.endswith(f" + {STEP}<{'double' if dtype == torch.float64 else 'float'}>"), note
                assert torch.equal(rd, torch.from_numpy(r).to(DEV))                  # the input is left alone
                assert np.array_equal(z.cpu().numpy(), ref), (degree, normalize, fused, note)
    h.close()


# ---------------------------------------------------------------------------------------------- 7. the apply, both forms
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_cheb_apply_bitwise_mirror(hipk, oracle, monkeypatch, name):
    build, dtype, plain, strided, fused_note = CONFIGS[name]
    _check_apply(hipk, oracle, monkeypatch, build(), dtype, plain, strided, fused_note)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("plain", [False, True], ids=["auto", "plain"])
@pytest.mark.parametrize("case", sorted({r["case"] for r in runs()}))
def test_cheb_apply_bitwise_mirror_fixture_matrices(hipk, oracle, monkeypatch, case, plain, dtype):
    """Every fixture matrix (n <= 2304, 17 x 13 = 221 rows among them).  With the plain CSR kernels these short-rowed matrices
    take the tile kernel's FAST instantiations, which have the epilogue; the coded forms of such small systems do not reach the
    two-rows-per-lane kernel."""
    A = csr(load_case(case))
    t = "double" if dtype == torch.float64 else "float"
    cap = 1280 if dtype == torch.float64 else 2048
    _check_apply(hipk, oracle, monkeypatch, A, dtype, plain, None, f"hipk_spmv_cheb_kernel<{t},{cap}>" if plain else None)


def test_cheb_apply_rejects_what_it_cannot_run(hipk):
    from pytorch_sparse_solver.module_a import ChebyshevPreconditioner
    A = _poisson(20, 20)
    M = ChebyshevPreconditioner(A, degree=2)
    v = torch.ones(400, dtype=torch.float64, device=DEV)
    op = hipk.OpHandle(lambda x: x, 400, torch.float64, torch.device(DEV))
    z, work = torch.empty_like(v), torch.empty(800, dtype=torch.float64, device=DEV)
    rc = hipk.lib().hipk_cheb_apply(op.ptr, 2, M.dinv.to(DEV).data_ptr(), M._coef, v.data_ptr(), z.data_ptr(), work.data_ptr(), None)
    assert rc != 0 and "matrix-free" in hipk.lib().hipk_last_error().decode()
    op.close()
    Ad = A.to(DEV)
    h = hipk.handle_for(Ad)
    for degree in (0, 33):
        rc = hipk.lib().hipk_cheb_apply(h.ptr, degree, M.dinv.to(DEV).data_ptr(), M._coef, v.data_ptr(), z.data_ptr(), work.data_ptr(), None)
        assert rc != 0
    with pytest.raises(ValueError, match="shape"):
        ChebyshevPreconditioner(Ad)(torch.ones(399, dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError, match="float32"):
        ChebyshevPreconditioner(Ad)(torch.ones(400, dtype=torch.float32, device=DEV))


# ---------------------------------------------------------------------------------------------- 8. whole solves
@pytest.mark.parametrize("r", runs(), ids=rid)
def test_gpu_solvers_with_chebyshev(hipk, r):
    from pytorch_sparse_solver.module_a import ChebyshevPreconditioner, bicgstab, cg, get_last_stats, gmres
    d = load_case(r["case"])
    A = csr(d, DEV)
    b = torch.from_numpy(d["b"]).to(DEV)
    x0 = torch.from_numpy(d["x0"]).to(DEV) if r["has_x0"] else None
    solve = {"cg": cg, "bicgstab": bicgstab, "gmres": gmres}[r["solver"]]
    out = []
    for _ in range(2):
        M = ChebyshevPreconditioner(A, degree=r["degree"], normalize=r["normalize"])
        path_before = hipk.last_solve_path()
        M(b)                                                              # an apply outside a solve leaves the solve path alone
        assert hipk.last_solve_path() == path_before and (M.applies, M.spmvs) == (1, r["degree"])
        x, info = solve(A, b, x0=x0, M=M, **r["kwargs"])
        st = get_last_stats()
        assert type(st).__name__ == "SolveStats" and "callable_M" in st.method    # the HIP path, not the generic one
        assert M.spmvs == r["degree"] * M.applies and M.applies > 1
        out.append((x.cpu().numpy(), info, st.matvecs, st.iterations))
    (xs, info, matvecs, _), again = out
    assert np.array_equal(xs, again[0]) and (info, matvecs) == again[1:3]           # run-to-run: the same bits
    x_ref = d[r["tag"] + "_x"]
    err = np.linalg.norm(xs - x_ref) / np.linalg.norm(x_ref)
    print(f"{rid(r)}: info {info} (reference {r['info']}), matvecs {matvecs} (reference {r['matvecs']}), |x - x_ref| / |x_ref| = {err:.3e}")
    assert info == r["info"]
    if r["solver"] == "cg":
        assert matvecs == r["matvecs"]
        assert err <= 1e-8
    elif r["solver"] == "bicgstab":
        assert abs(matvecs - r["matvecs"]) <= max(2, BICGSTAB_MATVEC_BAND * r["matvecs"])
        assert err <= 1e-5
    else:
        assert err <= 1e-8


# ---------------------------------------------------------------------------------------------- 9. one large case
def test_large_poisson_stop_logic(hipk):
    from pytorch_sparse_solver.module_a import ChebyshevPreconditioner, cg, get_last_stats
    A = _poisson(1000, 1000).to(DEV)
    n = A.shape[0]
    b = torch.ones(n, dtype=torch.float64, device=DEV)
    _, info_plain = cg(A, b, tol=1e-6)
    its_plain = get_last_stats().iterations
    M = ChebyshevPreconditioner(A, degree=3)
    x, info = cg(A, b, tol=1e-6, M=M)
    st = get_last_stats()
    y = hipk.spmv(hipk.handle_for(A), x)
    relres = float(torch.linalg.vector_norm(b - y) / torch.linalg.vector_norm(b))
    print(f"N = 1000^2: plain cg {its_plain} iterations (info {info_plain}); chebyshev(3) {st.iterations} iterations, info {info}, "
          f"true relres {relres:.3e}, {M.applies} applies, {st.solve_ms:.1f} ms")
    assert info_plain == 0 and info == 0 and "callable_M" in st.method
    assert st.iterations <= 0.35 * its_plain
    assert relres <= 1e-6
    assert M.spmvs == 3 * M.applies
