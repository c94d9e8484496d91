"""The three-launch CG sequence with the x update deferred (csrc/hipk_cg.hip: hipk_cg_pdir_kernel, hipk_cg_xdir_kernel,
hipk_cg_xflush_kernel): p ping-pongs between two buffers, x is brought up to date every second iteration for two iterations at
once -- x = (x + alpha_{k-1} p_{k-1}) + alpha_k p_k, each product and sum rounded on its own -- and a flush after the loop adds
the last term when an odd number of iterations ran.  Every case compares x, iterations, info, the true and the recurrence
residual BIT FOR BIT with HIPK_CG_DEFER_X=0 (hipk_cg_direction_kernel every iteration) and with the CPU oracle, and every arm
asserts the form it ran; one test shows through the C ABI that the second p buffer is really written (without it the comparisons
would pass vacuously whenever a gate left both arms on the old kernels), one reads the compiler's resource report of the two
per-chunk kernels (no GPU needed).

Main system: the 5-point Poisson matrix on a 137 x 135 grid -- n = 18 495: 10 reduction chunks, a ragged last chunk of 63
elements, n odd (fp64 vector tail 1) and n % 4 = 3 (fp32 tail); HIPK_CG_NO_LDS_LOOP keeps it on the launch sequence."""
import ctypes
import functools

import numpy as np
import pytest
import torch

DEV = "cuda:0"
NX, NY = 137, 135
FORM = "cg three-launch"


@functools.lru_cache(maxsize=None)
def _system(nx, ny, dt):
    """(device CSR tensor, numpy crow, col, val) of the Poisson matrix."""
    from pytorch_sparse_solver.utils.matrix_utils import create_poisson_2d_csr
    A = create_poisson_2d_csr(nx, ny, device=DEV)
    if dt == torch.float32:
        A = torch.sparse_csr_tensor(A.crow_indices(), A.col_indices(), A.values().float(), size=A.shape)
    return (A, A.crow_indices().cpu().numpy().astype(np.int32), A.col_indices().cpu().numpy().astype(np.int32),
            A.values().cpu().numpy())


def _solve(hipk, monkeypatch, A, b, x0, env, kw):
    for k in ("HIPK_CG_DEFER_X", "HIPK_CG_NO_LDS_LOOP", "HIPK_TEST_LDS_NOT_RESIDENT", "HIPK_NO_LDS_SPREAD", "HIPK_CG_LAUNCH_ITS",
              "HIPK_HOST_SIGNAL", "HIPK_PACE_WINDOW"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    x = torch.zeros_like(b) if x0 is None else x0.clone()
    st = hipk.solve("cg", hipk.handle_for(A), b, x, atol=0.0, **{"maxiter": None, **kw})
    assert hipk.last_solve_form() == FORM, (env, kw, hipk.last_solve_form())
    return x.cpu().numpy(), (st.iterations, st.info, st.residual_norm, st.recurrence_rs)


def _check(hipk, oracle, monkeypatch, grid, dt, b, x0, env, kw, path_suffix=None):
    """Both arms and the oracle on one case; returns the iteration count."""
    A, crow, col, val = _system(grid[0], grid[1], dt)
    bd = torch.from_numpy(b).to(DEV)
    x0d = None if x0 is None else torch.from_numpy(x0).to(DEV)
    new = _solve(hipk, monkeypatch, A, bd, x0d, env, kw)
    if path_suffix:
        assert hipk.last_solve_path().endswith(path_suffix), hipk.last_solve_path()
    old = _solve(hipk, monkeypatch, A, bd, x0d, {**env, "HIPK_CG_DEFER_X": "0"}, kw)
    ref = (oracle.cg if dt == torch.float64 else oracle.cg32)(crow, col, val, b, x0=x0, **kw)
    refs = (ref.iterations, ref.info, ref.residual_norm, ref.recurrence_rs)
    what = (grid, dt, env, kw)
    assert new[1] == old[1], (what, new[1], old[1])
    assert np.array_equal(new[0].view(np.uint8), old[0].view(np.uint8)), what
    assert new[1] == refs, (what, new[1], refs)
    assert np.array_equal(new[0].view(np.uint8), ref.x.astype(new[0].dtype).view(np.uint8)), what
    return new[1][0]


def _np_dt(dt):
    return np.float64 if dt == torch.float64 else np.float32


SEQ = {"HIPK_CG_NO_LDS_LOOP": "1"}


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_cutoffs_of_both_parities_and_one_stop(hipk, oracle, monkeypatch, dt):
    """maxiter 0 .. 5 with tol = 0: K even and odd, the flush idle and working; then one stop by the tolerance."""
    b = np.ones(NX * NY, dtype=_np_dt(dt))
    for m in range(6):
        assert _check(hipk, oracle, monkeypatch, (NX, NY), dt, b, None, SEQ, dict(tol=0.0, maxiter=m)) == m
    _check(hipk, oracle, monkeypatch, (NX, NY), dt, b, None, SEQ, dict(tol=1e-3))


@pytest.mark.gpu
def test_stops_of_both_parities(hipk, oracle, monkeypatch):
    b = np.ones(NX * NY)
    its = [_check(hipk, oracle, monkeypatch, (NX, NY), torch.float64, b, None, SEQ, dict(tol=t)) for t in (1e-1, 1e-2, 1e-3, 1e-6)]
    assert any(k & 1 for k in its) and any(not k & 1 for k in its), its   # (the oracle's counts: _check compared them)


@pytest.mark.gpu
def test_start_states(hipk, oracle, monkeypatch):
    """A random warm start; x0 = the exact solution: the stop at iteration 0."""
    rng = np.random.default_rng(7)
    n = NX * NY
    b, x0 = rng.standard_normal(n), rng.standard_normal(n)
    assert _check(hipk, oracle, monkeypatch, (NX, NY), torch.float64, b, x0, SEQ, dict(tol=1e-5)) > 0
    A = _system(NX, NY, torch.float64)[0]
    b_exact = hipk.spmv(hipk.handle_for(A), torch.from_numpy(x0).to(DEV)).cpu().numpy()
    assert _check(hipk, oracle, monkeypatch, (NX, NY), torch.float64, b_exact, x0, SEQ, dict(tol=0.5)) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("launch_its", [7, 6])
def test_entry_after_a_hand_back(hipk, oracle, monkeypatch, launch_its):
    """The mid loop runs `launch_its` iterations, its second launch reports "not co-resident": the sequence starts at an odd and
    at an even iteration, with p where the loop left it."""
    b = np.ones(NX * NY)
    env = {"HIPK_TEST_LDS_NOT_RESIDENT": "2", "HIPK_NO_LDS_SPREAD": "1", "HIPK_CG_LAUNCH_ITS": str(launch_its)}
    for kw in (dict(tol=1e-6), dict(tol=0.0, maxiter=launch_its + 3), dict(tol=0.0, maxiter=launch_its + 4)):
        assert _check(hipk, oracle, monkeypatch, (NX, NY), torch.float64, b, None, env, kw, path_suffix="launch sequence") > launch_its


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{"HIPK_HOST_SIGNAL": "0"}, {"HIPK_PACE_WINDOW": "1"}], ids=["stream-polling", "window1"])
def test_pacing(hipk, oracle, monkeypatch, env):
    _check(hipk, oracle, monkeypatch, (NX, NY), torch.float64, np.ones(NX * NY), None, {**SEQ, **env}, dict(tol=1e-2))


@pytest.mark.gpu
def test_the_size_the_dispatch_takes_by_itself(hipk, oracle, monkeypatch):
    """1100 x 1000: 538 chunks, beyond the mid loop -- no switch set."""
    b = np.random.default_rng(11).standard_normal(1100 * 1000)
    for m in (25, 26):
        assert _check(hipk, oracle, monkeypatch, (1100, 1000), torch.float64, b, None, {}, dict(tol=0.0, maxiter=m)) == m


@pytest.mark.gpu
def test_the_second_p_buffer_is_written_only_by_the_deferred_sequence(hipk, monkeypatch):
    """hipk_cg_solve through the C ABI on a workspace pre-filled with a sentinel: the fourth vector (behind Ap) is written by
    default and untouched with HIPK_CG_DEFER_X=0."""
    A = _system(NX, NY, torch.float64)[0]
    h, L, n = hipk.handle_for(A), hipk.lib(), NX * NY
    wb = int(L.hipk_cg_work_bytes(n, hipk.HIPK_F64))
    vec = (n * 8 + 255) // 256 * 256
    off = 256 + int(L.hipk_scratch_bytes()) + 3 * vec
    assert off + vec <= wb
    b = torch.ones(n, dtype=torch.float64, device=DEV)
    monkeypatch.setenv("HIPK_CG_NO_LDS_LOOP", "1")
    touched = {}
    for defer in ("1", "0"):
        monkeypatch.setenv("HIPK_CG_DEFER_X", defer)
        work = torch.full((wb,), 0xA5, dtype=torch.uint8, device=DEV)
        x = torch.zeros_like(b)
        prm, st = hipk.Params(), hipk.Stats()
        prm.tol, prm.atol, prm.maxiter, prm.gpu_tolerances = 1e-6, 0.0, -1, 1
        with torch.cuda.device(h.device):
            rc = L.hipk_cg_solve(h.ptr, b.data_ptr(), x.data_ptr(), work.data_ptr(), wb, ctypes.byref(prm), ctypes.byref(st),
                                 torch.cuda.current_stream().cuda_stream)
        assert rc == 0 and st.info == 0 and hipk.last_solve_form() == FORM, (defer, rc, st.info, hipk.last_solve_form())
        touched[defer] = bool((work[off:off + n * 8] != 0xA5).any().item())
    assert touched == {"1": True, "0": False}, touched


def test_the_deferred_kernels_keep_eight_workgroups_per_cu():
    """<= 64 VGPRs, <= 80 SGPRs, no scratch for the fp64 instantiations (one round of workgroups at n = 4 M), from the compiler's
    resource report as tests/test_kernel_resources.py reads it."""
    import os
    import shutil
    import test_kernel_resources as kr
    if not os.path.exists(kr.HIPCC) or shutil.which("c++filt") is None:
        pytest.skip("hipcc / c++filt not installed")
    got = kr._vgprs("hipk_cg.hip")
    for k in ("void hipk_cg_pdir_kernel<double>", "void hipk_cg_xdir_kernel<double>"):
        assert k in got, (k, sorted(got)[:60])
        assert got[k] <= 64 and kr._vgprs.sgprs[k] <= 80 and kr._vgprs.scratch[k] == 0, (k, got[k], kr._vgprs.sgprs[k], kr._vgprs.scratch[k])
