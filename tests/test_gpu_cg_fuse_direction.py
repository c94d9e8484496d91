"""The CG direction step as the tail of the fused SpMV + update launch (csrc/hipk_cg_fuse.h, steps 6-9): <r,r> crosses the
workgroups through a second hand-off inside the launch, p_{k+1} = r_{k+1} + beta p_k is formed from the registers that hold
r_{k+1}, and on every second iteration the deferred x update runs in front of that hand-off -- one launch per iteration.

Every case compares x, iterations, info, the true and the recurrence residual BIT FOR BIT with the HIPK_CG_FUSE_DIRECTION=0 arm
(the fused launch followed by hipk_cg_pdir_kernel / hipk_cg_xdir_kernel) and with the CPU oracle, and asserts
hipk_last_cg_fused_directions(): the iteration count in the new arm, 0 in the other -- a gate that silently left both arms on
the same launches would fail there.  The kernel note, the form and the path are those of the fused sequence in both arms.

Sizes, matrices and helpers are those of tests/test_gpu_cg_fuse_update.py (the envelope is the same: 512 < chunks <= 2048); tol = 0
and maxiter <= 9 keep every case at a few launches."""
import json

import numpy as np
import pytest
import torch

import test_gpu_cg_fuse_update as fu
from test_gpu_cg_fuse_update import DEV, FORM, FUSED5, _band, _fresh_handle, _poisson, _reference, _same, _separate

OWN = ("HIPK_CG_FUSE_DIRECTION", "HIPK_TEST_CG_FUSE_DIR_GIVE_UP")


def _solve(hipk, monkeypatch, h, b, x0, env, kw, work=None):
    """fu._solve with this file's switches cleared as well; appends hipk_last_cg_fused_directions()."""
    for k in OWN:
        monkeypatch.delenv(k, raising=False)
    got = fu._solve(hipk, monkeypatch, h, b, x0, env, kw, work=work)
    return got + (hipk.last_cg_fused_directions(),)


def _refs(ref):
    return ref.x, (ref.iterations, ref.info, ref.residual_norm, ref.recurrence_rs)


def _check(hipk, oracle, monkeypatch, system, b, x0, kw, units=5):
    """The tail arm, the HIPK_CG_FUSE_DIRECTION=0 arm and the oracle on one case; returns the iteration count."""
    A = system[0]
    h = hipk.handle_for(A)
    bd = torch.from_numpy(b).to(DEV)
    x0d = None if x0 is None else torch.from_numpy(x0).to(DEV)
    new = _solve(hipk, monkeypatch, h, bd, x0d, {}, kw)
    old = _solve(hipk, monkeypatch, h, bd, x0d, {"HIPK_CG_FUSE_DIRECTION": "0"}, kw)
    what = (A.shape, kw)
    note = f"hipk_cg_fuse_update_kernel<{units}>"
    assert new[2] == old[2] == note and new[3] == old[3] == FORM, (what, new[2:], old[2:])
    assert hipk.last_solve_path() == "launch sequence", (what, hipk.last_solve_path())
    ref = _refs(_reference(oracle, system, b, x0, kw))
    assert new[1] == old[1] == ref[1], (what, new[1], old[1], ref[1])
    assert np.array_equal(new[0].view(np.uint8), old[0].view(np.uint8)), what
    assert np.array_equal(new[0].view(np.uint8), ref[0].view(np.uint8)), what
    assert new[4] == new[1][0] and old[4] == 0, (what, new[4], old[4], new[1][0])
    return new[1][0]


@pytest.mark.gpu
def test_one_row_in_the_last_chunk_cutoffs_of_both_parities_and_one_stop(hipk, oracle, monkeypatch):
    """1025 x 1025 (514 chunks, the last of ONE row, n odd), b = ones: maxiter 0 .. 5 with tol = 0 (the x flush idle and working,
    the stop on the first pass), then the recorded stop by the tolerance: 1301 iterations, decided by the tail's collector."""
    sysm = _poisson(1025, 1025)
    b = np.ones(1025 * 1025)
    for m in range(6):
        assert _check(hipk, oracle, monkeypatch, sysm, b, None, dict(tol=0.0, maxiter=m)) == m
    with open(fu.TOL_STOP) as f:
        want = json.load(f)
    assert want["n"] == b.size and want["tol"] == 1e-3 and want["iterations"] == 1301
    bd = torch.from_numpy(b).to(DEV)
    h = hipk.handle_for(sysm[0])
    new = _solve(hipk, monkeypatch, h, bd, None, {}, dict(tol=1e-3))
    old = _solve(hipk, monkeypatch, h, bd, None, {"HIPK_CG_FUSE_DIRECTION": "0"}, dict(tol=1e-3))
    assert new[2] == old[2] == FUSED5 and new[3] == old[3] == FORM, (new[2:], old[2:])
    assert _same(new, old), (new[1], old[1])
    assert fu._digest(new[0], new[1]) == {k: want[k] for k in fu._digest(new[0], new[1])}, (new[1], want)
    assert new[4] == want["iterations"] and old[4] == 0, (new[4], old[4])


@pytest.mark.gpu
def test_random_right_hand_side_and_warm_start(hipk, oracle, monkeypatch):
    rng = np.random.default_rng(5)
    n = 1025 * 1025
    b, x0 = rng.standard_normal(n), rng.standard_normal(n)
    sysm = _poisson(1025, 1025)
    for m in (4, 5):
        assert _check(hipk, oracle, monkeypatch, sysm, b, None, dict(tol=0.0, maxiter=m)) == m
        assert _check(hipk, oracle, monkeypatch, sysm, b, x0, dict(tol=0.0, maxiter=m)) == m


@pytest.mark.gpu
@pytest.mark.parametrize("nx,ny,seed", [(1024, 1026, 6), (2048, 2048, 8)], ids=["513-full-chunks", "2048-chunks-every-slot"])
def test_the_edges_of_the_envelope(hipk, oracle, monkeypatch, nx, ny, seed):
    b = np.random.default_rng(seed).standard_normal(nx * ny)
    for m in (4, 5):
        assert _check(hipk, oracle, monkeypatch, _poisson(nx, ny), b, None, dict(tol=0.0, maxiter=m)) == m


@pytest.mark.gpu
@pytest.mark.parametrize("width,units", [(7, 8), (4, 4)])
def test_wider_and_narrower_stencils(hipk, oracle, monkeypatch, width, units):
    """The UNITS = 8 and UNITS = 4 instantiations, 514 chunks, a ragged last chunk of 77 rows."""
    sysm = _band(width)
    b = np.random.default_rng(width).standard_normal(sysm[0].shape[0])
    for m in (3, 4):
        assert _check(hipk, oracle, monkeypatch, sysm, b, None, dict(tol=0.0, maxiter=m), units=units) == m


@pytest.mark.gpu
def test_the_collector_of_either_hand_off_gives_up(hipk, oracle, monkeypatch):
    """HIPK_TEST_CG_FUSE_DIR_GIVE_UP = 0, 1, 4 (a p-only iteration, an x iteration, a later p-only one): iteration k is finished
    by hipk_cg_pdir_kernel, the solve goes on with the separate kernels and gives the same bits; k iterations ran their direction
    step in the fused launch; the handle does not try the fused form again, a fresh handle does.  HIPK_TEST_CG_FUSE_GIVE_UP = 1, 4
    with the tail on: the first hand-off's give-up, the same bits."""
    sysm = _poisson(1025, 1025)
    b = np.random.default_rng(9).standard_normal(1025 * 1025)
    bd = torch.from_numpy(b).to(DEV)
    kw = dict(tol=0.0, maxiter=9)
    ref = _refs(_reference(oracle, sysm, b, None, kw))
    assert ref[1][0] == 9
    for switch, ks in (("HIPK_TEST_CG_FUSE_DIR_GIVE_UP", (0, 1, 4)), ("HIPK_TEST_CG_FUSE_GIVE_UP", (1, 4))):
        for k in ks:
            h = _fresh_handle(hipk, sysm)
            got = _solve(hipk, monkeypatch, h, bd, None, {switch: str(k)}, kw)
            assert _same(got, ref) and _separate(got[2]) and got[3] == FORM, (switch, k, got[1:], ref[1])
            assert got[4] == k, (switch, k, got[4])
            again = _solve(hipk, monkeypatch, h, bd, None, {}, kw)   # no hook: the latch of the handle keeps the fused form off
            assert _same(again, ref) and _separate(again[2]) and again[4] == 0, (switch, k, again[1:])
            h.close()
    fresh = _fresh_handle(hipk, sysm)
    got = _solve(hipk, monkeypatch, fresh, bd, None, {}, kw)
    assert _same(got, ref) and got[2] == FUSED5 and got[4] == 9, got[1:]
    fresh.close()


@pytest.mark.gpu
def test_workspace_of_exactly_work_bytes_in_every_state(hipk, oracle, monkeypatch):
    """`work` of exactly hipk_cg_work_bytes between guards, filled with 0x00, 0xFF, 0x5A and not refilled: the same solve."""
    from _solve_runner import run_solve_case
    for k in fu.SWITCHES + OWN:
        monkeypatch.delenv(k, raising=False)
    A, crow, col, val = _poisson(1025, 1025)
    b = np.random.default_rng(10).standard_normal(1025 * 1025)
    kw = dict(tol=0.0, maxiter=5)
    st, x, _ = run_solve_case(hipk, "cg fused direction 1025x1025", "cg", hipk.handle_for(A), b, None, None, kw, "launch sequence", FORM)
    assert hipk.CsrHandle.last_spmv_kernel() == FUSED5 and hipk.last_cg_fused_directions() == 5
    ref = oracle.cg(crow, col, val, b, **kw)
    assert (st.iterations, st.info, st.residual_norm, st.recurrence_rs) == (ref.iterations, ref.info, ref.residual_norm, ref.recurrence_rs)
    assert np.array_equal(x.view(np.uint8), ref.x.view(np.uint8))


@pytest.mark.gpu
def test_two_right_hand_sides_back_to_back_on_one_workspace(hipk, oracle, monkeypatch):
    """The second solve finds the first one's flagged words (sequence numbers 1 .. 6, then 1 .. 5 again) in BOTH word regions."""
    A, crow, col, val = _poisson(1025, 1025)
    n = 1025 * 1025
    h = hipk.handle_for(A)
    wb = int(hipk.lib().hipk_cg_work_bytes(n, hipk.HIPK_F64))
    work = torch.empty(wb + 256, dtype=torch.uint8, device=DEV)
    work = work[(-work.data_ptr()) % 256:][:wb]
    rng = np.random.default_rng(12)
    for m in (6, 5):
        b = rng.standard_normal(n)
        got = _solve(hipk, monkeypatch, h, torch.from_numpy(b).to(DEV), None, {}, dict(tol=0.0, maxiter=m), work=work)
        ref = _refs(oracle.cg(crow, col, val, b, tol=0.0, maxiter=m))
        assert got[2] == FUSED5 and got[1] == ref[1] and got[4] == m, (m, got[1:])
        assert np.array_equal(got[0].view(np.uint8), ref[0].view(np.uint8)), m


@pytest.mark.gpu
def test_x_every_iteration_does_not_take_the_tail(hipk, oracle, monkeypatch):
    """HIPK_CG_DEFER_X=0: the fused launch and hipk_cg_direction_kernel, whatever HIPK_CG_FUSE_DIRECTION says."""
    sysm = _poisson(1025, 1025)
    b = np.random.default_rng(5).standard_normal(1025 * 1025)
    bd = torch.from_numpy(b).to(DEV)
    kw = dict(tol=0.0, maxiter=4)
    ref = _refs(_reference(oracle, sysm, b, None, kw))
    for env in ({"HIPK_CG_DEFER_X": "0"}, {"HIPK_CG_DEFER_X": "0", "HIPK_CG_FUSE_DIRECTION": "1"}):
        got = _solve(hipk, monkeypatch, hipk.handle_for(sysm[0]), bd, None, env, kw)
        assert _same(got, ref) and got[2] == FUSED5 and got[3] == FORM and got[4] == 0, (env, got[1:])


def test_the_fused_kernel_with_its_tail_keeps_eight_workgroups_per_cu(monkeypatch):
    """<= 64 VGPRs, <= 80 SGPRs, no scratch, <= 20 480 bytes of static LDS for the three instantiations: the compiler's report,
    read by the existing check."""
    fu.test_the_fused_kernel_keeps_eight_workgroups_per_cu(monkeypatch)
