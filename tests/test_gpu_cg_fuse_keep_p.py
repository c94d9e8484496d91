"""The fused CG launch keeps p_k on chip between its SpMV walk and its direction tail (csrc/hipk_cg_fuse.h, step 7; `keep` of
hipk_sell_wide_walk in csrc/hipk_coded.h): the thread that formed two rows of a uniform tile holds p_k of exactly the elements
it owns in the tail, so only the steps of tiles with a grid-line end are loaded again.

Every case compares x, iterations, info, the true and the recurrence residual BIT FOR BIT with the HIPK_CG_FUSE_KEEP_P=0 arm (the
tail loads all of p_k, as before) and with the CPU oracle, and asserts hipk_last_cg_fused_kept_p(): the iteration count in the new
arm, 0 in the other -- a switch that silently left both arms on the same loads would fail there.  Both arms run the fused launch
with its tail (the kernel note and hipk_last_cg_fused_directions() say so).

Sizes, matrices, helpers and right-hand sides are those of tests/test_gpu_cg_fuse_update.py and test_gpu_cg_fuse_direction.py (the
envelope is the same: 512 < chunks <= 2048, and the oracle's solves are shared through their cache); tol = 0 and maxiter <= 5 keep
every case at a few launches."""
import numpy as np
import pytest
import torch

import test_gpu_cg_fuse_direction as fd
import test_gpu_cg_fuse_update as fu
from test_gpu_cg_fuse_update import DEV, FORM, FUSED5, _band, _fresh_handle, _poisson, _reference, _same, _separate

OWN = ("HIPK_CG_FUSE_KEEP_P", "HIPK_TEST_CG_FUSE_GIVE_UP", "HIPK_SPMV_MASKED")
TPC = 8   # tiles of 256 rows per chunk of 2048


def _solve(hipk, monkeypatch, h, b, x0, env, kw):
    """fd._solve with this file's switches cleared as well; appends hipk_last_cg_fused_kept_p()."""
    for k in OWN:
        monkeypatch.delenv(k, raising=False)
    got = fd._solve(hipk, monkeypatch, h, b, x0, env, kw)
    return got + (hipk.last_cg_fused_kept_p(),)


def _check(hipk, oracle, monkeypatch, system, b, x0, kw, units=5, handle=None):
    """The keep-p arm, the HIPK_CG_FUSE_KEEP_P=0 arm and the oracle on one case; returns the iteration count."""
    A = system[0]
    h = hipk.handle_for(A) if handle is None else handle
    bd = torch.from_numpy(b).to(DEV)
    x0d = None if x0 is None else torch.from_numpy(x0).to(DEV)
    new = _solve(hipk, monkeypatch, h, bd, x0d, {}, kw)
    old = _solve(hipk, monkeypatch, h, bd, x0d, {"HIPK_CG_FUSE_KEEP_P": "0"}, kw)
    what = (A.shape, kw)
    note = f"hipk_cg_fuse_update_kernel<{units}>"
    assert new[2] == old[2] == note and new[3] == old[3] == FORM, (what, new[2:], old[2:])
    assert hipk.last_solve_path() == "launch sequence", (what, hipk.last_solve_path())
    ref = fd._refs(_reference(oracle, system, b, x0, kw))
    assert new[1] == old[1] == ref[1], (what, new[1], old[1], ref[1])
    assert np.array_equal(new[0].view(np.uint8), old[0].view(np.uint8)), what
    assert np.array_equal(new[0].view(np.uint8), ref[0].view(np.uint8)), what
    its = new[1][0]
    assert new[4] == old[4] == its, (what, new[4], old[4], its)      # both arms took the tail
    assert new[5] == its and old[5] == 0, (what, new[5], old[5], its)
    return its


def _non_uniform_tiles(crow, col, val):
    """Which tiles of 256 rows hipk_tile_uniform_kernel finds NOT uniform, from the CSR: a tile is uniform when it is whole and all
    its rows carry the same (column - row, value) list."""
    n = crow.size - 1
    lens = np.diff(crow)
    w = int(lens.max())
    slot = np.arange(w)
    have = slot[None, :] < lens[:, None]
    idx = np.minimum(crow[:-1, None] + slot[None, :], col.size - 1)
    off = np.where(have, col[idx] - np.arange(n)[:, None], np.iinfo(np.int64).min)
    v = np.where(have, val[idx], 0.0)
    whole = n // 256
    ntiles = (n + 255) // 256
    differ = np.ones(ntiles, dtype=bool)   # a last tile of fewer rows is never uniform
    o3, v3 = off[:whole * 256].reshape(whole, 256, w), v[:whole * 256].reshape(whole, 256, w)
    differ[:whole] = ~((o3 == o3[:, :1]).all(axis=(1, 2)) & (v3 == v3[:, :1]).all(axis=(1, 2)))
    return differ


def test_the_1025_grid_mixes_kept_and_loaded_steps_in_both_thread_halves():
    """No GPU: on the 1025 x 1025 grid every whole chunk has two or three non-uniform tiles, and they fall on odd and on even
    local indices (local tile i belongs to thread half i & 1, step i >> 1) -- so the tail mixes kept and loaded
    steps in both halves.  On 1024 x 1026 the line ends fall on tile boundaries: still non-uniform tiles, in every chunk."""
    from pytorch_sparse_solver.utils.matrix_utils import create_poisson_2d_csr
    for nx, ny in ((1025, 1025), (1024, 1026)):
        A = create_poisson_2d_csr(nx, ny, device="cpu")
        differ = _non_uniform_tiles(A.crow_indices().numpy().astype(np.int64), A.col_indices().numpy().astype(np.int64), A.values().numpy())
        per_chunk = np.add.reduceat(differ.astype(np.int64), np.arange(0, differ.size, TPC))
        local = np.flatnonzero(differ) % TPC
        if nx == 1025:
            assert 1024 <= differ.sum() <= 2 * 1024 + 1, (differ.sum(), differ.size)   # 1024 line ends inside: one tile or two each
            assert differ.size == 4105 and per_chunk.size == 514 and differ[-1]   # the last chunk: one row, one tile
            assert set(np.unique(per_chunk[:513])) == {2, 3}, np.bincount(per_chunk)   # two line ends per chunk, one of them split
            assert (local % 2 == 1).any() and (local % 2 == 0).any(), np.bincount(local)
            assert set(np.unique(local)) == set(range(TPC)), np.bincount(local)   # every step of both halves is loaded somewhere
        else:
            assert per_chunk.size == 513 and per_chunk.min() >= 1, np.bincount(per_chunk)


@pytest.mark.gpu
def test_one_row_in_the_last_chunk_cutoffs_of_both_parities(hipk, oracle, monkeypatch):
    """1025 x 1025 (514 chunks, the last of ONE row, n odd): b = ones, then a random b without and with a random x0; maxiter 0 .. 5
    (p-only and x iterations, the flush idle and working)."""
    sysm = _poisson(1025, 1025)
    n = 1025 * 1025
    rng = np.random.default_rng(5)
    b, x0 = rng.standard_normal(n), rng.standard_normal(n)
    for m in range(6):
        assert _check(hipk, oracle, monkeypatch, sysm, np.ones(n), None, dict(tol=0.0, maxiter=m)) == m
        assert _check(hipk, oracle, monkeypatch, sysm, b, x0, dict(tol=0.0, maxiter=m)) == m
    assert _check(hipk, oracle, monkeypatch, sysm, b, None, dict(tol=0.0, maxiter=5)) == 5


@pytest.mark.gpu
@pytest.mark.parametrize("nx,ny,seed,ms", [(1024, 1026, 6, (4, 5)), (2048, 2048, 8, (5,))], ids=["513-full-chunks", "2048-chunks-every-slot"])
def test_the_edges_of_the_envelope(hipk, oracle, monkeypatch, nx, ny, seed, ms):
    b = np.random.default_rng(seed).standard_normal(nx * ny)
    for m in ms:
        assert _check(hipk, oracle, monkeypatch, _poisson(nx, ny), b, None, dict(tol=0.0, maxiter=m)) == m


@pytest.mark.gpu
@pytest.mark.parametrize("width,units", [(7, 8), (4, 4)])
def test_wider_and_narrower_stencils(hipk, oracle, monkeypatch, width, units):
    """The UNITS = 8 (one step kept) and UNITS = 4 instantiations, 514 chunks, a ragged last chunk of 77 rows."""
    sysm = _band(width)
    b = np.random.default_rng(width).standard_normal(sysm[0].shape[0])
    for m in (3, 4):
        assert _check(hipk, oracle, monkeypatch, sysm, b, None, dict(tol=0.0, maxiter=m), units=units) == m


@pytest.mark.gpu
def test_uniform_tiles_without_a_diagonal_entry(hipk, oracle, monkeypatch):
    """No entry at offset 0: the walk has no diagonal load to take p_k from and reads the operand w (= p_k) of its rows instead --
    what it keeps is still p_k.  (Not positive definite: five iterations of the recurrence, bit for bit, is all that is asked.)"""
    from test_gpu_coded import banded
    n = 513 * 2048 + 77
    v = np.asarray([-1.0, -1.5, -1.5, -1.0])
    crow, col, val = banded(n, [-1100, -1, 1, 1100], lambda r, k: v[k])
    A = torch.sparse_csr_tensor(torch.from_numpy(crow).to(DEV), torch.from_numpy(col).to(DEV), torch.from_numpy(val).to(DEV), size=(n, n))
    sysm = (A, crow.astype(np.int32), col.astype(np.int32), val)
    b = np.random.default_rng(11).standard_normal(n)
    h = _fresh_handle(hipk, sysm)
    for m in (4, 5):
        assert _check(hipk, oracle, monkeypatch, sysm, b, None, dict(tol=0.0, maxiter=m), units=4, handle=h) == m
    h.close()


@pytest.mark.gpu
def test_masked_tiles_are_kept_too(hipk, oracle, monkeypatch):
    """HIPK_SPMV_MASKED=1 at handle creation: the tiles with a line end go through the two-rows-per-lane path with a presence mask,
    and their rows of p_k are kept like a uniform tile's."""
    sysm = _poisson(1025, 1025)
    b = np.random.default_rng(5).standard_normal(1025 * 1025)
    monkeypatch.setenv("HIPK_SPMV_MASKED", "0")
    plain = _fresh_handle(hipk, sysm)
    plain_bytes = plain.format_bytes()
    plain.close()
    monkeypatch.setenv("HIPK_SPMV_MASKED", "1")
    h = _fresh_handle(hipk, sysm)
    assert h.format_bytes() != plain_bytes, "the handle built no masked tiles"
    assert _check(hipk, oracle, monkeypatch, sysm, b, None, dict(tol=0.0, maxiter=5), handle=h) == 5
    h.close()


@pytest.mark.gpu
def test_the_collector_of_either_hand_off_gives_up_with_p_kept(hipk, oracle, monkeypatch):
    """HIPK_TEST_CG_FUSE_DIR_GIVE_UP and HIPK_TEST_CG_FUSE_GIVE_UP at an even and an odd iteration: the solve goes on with the
    separate kernels and gives the bits of the solve without the hook; k iterations ran in the fused launch, all with p kept."""
    sysm = _poisson(1025, 1025)
    b = np.random.default_rng(5).standard_normal(1025 * 1025)
    bd = torch.from_numpy(b).to(DEV)
    kw = dict(tol=0.0, maxiter=5)
    ref = fd._refs(_reference(oracle, sysm, b, None, kw))
    assert ref[1][0] == 5
    for switch in ("HIPK_TEST_CG_FUSE_DIR_GIVE_UP", "HIPK_TEST_CG_FUSE_GIVE_UP"):
        for k in (2, 3):
            h = _fresh_handle(hipk, sysm)
            got = _solve(hipk, monkeypatch, h, bd, None, {switch: str(k)}, kw)
            assert _same(got, ref) and _separate(got[2]) and got[3] == FORM, (switch, k, got[1:], ref[1])
            assert got[4] == k and got[5] == k, (switch, k, got[4], got[5])
            h.close()
            h = _fresh_handle(hipk, sysm)
            off = _solve(hipk, monkeypatch, h, bd, None, {switch: str(k), "HIPK_CG_FUSE_KEEP_P": "0"}, kw)
            assert _same(off, ref) and off[4] == k and off[5] == 0, (switch, k, off[1:])
            h.close()
    fresh = _fresh_handle(hipk, sysm)
    got = _solve(hipk, monkeypatch, fresh, bd, None, {}, kw)
    assert _same(got, ref) and got[2] == FUSED5 and got[4] == 5 and got[5] == 5, got[1:]
    fresh.close()


def test_the_fused_kernel_that_keeps_p_keeps_eight_workgroups_per_cu(monkeypatch):
    """<= 64 VGPRs, <= 80 SGPRs, no scratch, <= 20 480 bytes of static LDS for UNITS 4, 5 and 8: the compiler's report, read by
    the existing check."""
    fu.test_the_fused_kernel_keeps_eight_workgroups_per_cu(monkeypatch)
