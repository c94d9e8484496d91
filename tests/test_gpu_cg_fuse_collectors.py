"""Both hand-offs of the fused CG launch run through EIGHT collector workgroups (csrc/hipk_cg_fuse.h, steps 4 and 8): collector s
polls one flagged word per thread -- residue class s of the spec's fold -- and hands its class sum out in slot s of eight lines;
every workgroup folds the eight slots of its line.  tests/test_cg_fuse_fold.py shows on the CPU that the split keeps the spec's
bits; here the kernel shows it at the sizes where the classes differ in length, for the three stencil widths, and when ONE
collector gives up.

Every case compares x, iterations, info, the true and the recurrence residual BIT FOR BIT with the HIPK_CG_FUSE_UPDATE=0 arm
(separate kernels) and with the CPU oracle, and asserts hipk_last_cg_fused_directions() and hipk_last_cg_fused_kept_p(): the
iterations run.  The systems are the smallest the form takes (512 < chunks <= 2048); tol = 0 and maxiter 5 and 6 keep every
case at a few launches and run both parities of the deferred x update."""
import numpy as np
import pytest
import torch

import test_gpu_cg_fuse_direction as fd
import test_gpu_cg_fuse_keep_p as fk
from test_gpu_cg_fuse_update import DEV, FORM, _band, _fresh_handle, _poisson, _reference, _same, _separate

WHO = "HIPK_TEST_CG_FUSE_GIVE_UP_WHO"


def _solve(hipk, monkeypatch, h, b, env, kw):
    """fk._solve (x, stats, note, form, fused directions, kept p) with this file's switch cleared as well."""
    monkeypatch.delenv(WHO, raising=False)
    return fk._solve(hipk, monkeypatch, h, b, None, env, kw)


def _check(hipk, oracle, monkeypatch, system, seed, units=5):
    A = system[0]
    n = A.shape[0]
    b = np.random.default_rng(seed).standard_normal(n)
    bd = torch.from_numpy(b).to(DEV)
    h = hipk.handle_for(A)
    note = f"hipk_cg_fuse_update_kernel<{units}>"
    for m in (5, 6):
        kw = dict(tol=0.0, maxiter=m)
        new = _solve(hipk, monkeypatch, h, bd, {}, kw)
        old = _solve(hipk, monkeypatch, h, bd, {"HIPK_CG_FUSE_UPDATE": "0"}, kw)
        ref = fd._refs(_reference(oracle, system, b, None, kw))
        what = (A.shape, m)
        assert new[2] == note and _separate(old[2], units) and new[3] == old[3] == FORM, (what, new[2:], old[2:])
        assert new[1] == old[1] == ref[1] and new[1][0] == m, (what, new[1], old[1], ref[1])
        assert np.array_equal(new[0].view(np.uint8), old[0].view(np.uint8)), what
        assert np.array_equal(new[0].view(np.uint8), ref[0].view(np.uint8)), what
        assert new[4] == m and new[5] == m and old[4] == 0 and old[5] == 0, (what, new[4:], old[4:])


@pytest.mark.gpu
@pytest.mark.parametrize("nx,ny,g,last,seed", [(1025, 1024, 513, 1024, 21), (707, 1515, 524, 1, 22), (2048, 2048, 2048, 2048, 8)],
                         ids=["513-chunks-the-minimum", "524-chunks-4-mod-8-one-row-last", "2048-chunks-every-slot-of-every-class"])
def test_the_edges_of_the_envelope(hipk, oracle, monkeypatch, nx, ny, g, last, seed):
    """g = 513: class 0 has 65 words, the others 64.  g = 524 = 4 mod 8: classes 0 .. 3 one word longer than 4 .. 7, and the last
    chunk holds one row.  g = 2048: every thread of every collector has a word."""
    n = nx * ny
    assert (n + 2047) // 2048 == g and n - (g - 1) * 2048 == last
    _check(hipk, oracle, monkeypatch, _poisson(nx, ny), seed)


@pytest.mark.gpu
@pytest.mark.parametrize("width,units", [(7, 8), (4, 4)])
def test_wider_and_narrower_stencils(hipk, oracle, monkeypatch, width, units):
    """The UNITS = 8 and UNITS = 4 instantiations at 514 chunks (classes 0 and 1 one word longer), a ragged last chunk of 77 rows."""
    _check(hipk, oracle, monkeypatch, _band(width), 30 + width, units=units)


@pytest.mark.gpu
@pytest.mark.parametrize("who", [0, 3, 7])
def test_one_collector_gives_up(hipk, oracle, monkeypatch, who):
    """HIPK_TEST_CG_FUSE_GIVE_UP_WHO = s: collector s alone behaves as if its poll had run out -- at the first hand-off of iteration
    1, at the second hand-off of iterations 0 and 1 (a p-only and an x iteration) -- while the other seven hand out their sums.
    Every workgroup finds the mark in slot s of its line and stores nothing of that step: the solve goes on with the separate
    kernels and gives the oracle's bits, k iterations ran in the fused launch, the handle keeps the fused form off afterwards and
    a fresh handle takes it again."""
    sysm = _poisson(1025, 1024)
    b = np.random.default_rng(21).standard_normal(1025 * 1024)
    bd = torch.from_numpy(b).to(DEV)
    kw = dict(tol=0.0, maxiter=5)
    ref = fd._refs(_reference(oracle, sysm, b, None, kw))
    assert ref[1][0] == 5
    for switch, ks in (("HIPK_TEST_CG_FUSE_GIVE_UP", (1,)), ("HIPK_TEST_CG_FUSE_DIR_GIVE_UP", (0, 1))):
        for k in ks:
            h = _fresh_handle(hipk, sysm)
            got = _solve(hipk, monkeypatch, h, bd, {switch: str(k), WHO: str(who)}, kw)
            assert _same(got, ref) and _separate(got[2]) and got[3] == FORM, (switch, k, who, got[1:], ref[1])
            assert got[4] == k and got[5] == k, (switch, k, who, got[4:])
            again = _solve(hipk, monkeypatch, h, bd, {}, kw)   # no hook: the latch of the handle keeps the fused form off
            assert _same(again, ref) and _separate(again[2]) and again[4] == 0, (switch, k, who, again[1:])
            h.close()
    fresh = _fresh_handle(hipk, sysm)
    got = _solve(hipk, monkeypatch, fresh, bd, {}, kw)
    assert _same(got, ref) and got[2] == fk.FUSED5 and got[4] == 5 and got[5] == 5, got[1:]
    fresh.close()
