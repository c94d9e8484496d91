"""The CG loop's stencil SpMV and update step in one launch (csrc/hipk_cg_fuse.h: hipk_cg_fuse_update_kernel): Ap stays in LDS, the
chunks' <p,Ap> partials go to one collector workgroup as flagged words and <p,Ap> comes back through eight replicated words.
Every case compares x, iterations, info, the true and the recurrence residual BIT FOR BIT with the HIPK_CG_FUSE_UPDATE=0 arm (SpMV
and hipk_cg_update_kernel as two launches) and with the CPU oracle, and every arm asserts the kernel note it ran under: the fused
arm hipk_cg_fuse_update_kernel<UNITS>, the other arm the two-rows-per-lane SpMV kernel's chunk walk -- a gate that silently left
both arms on the same kernels would fail there.

The sizes are fixed by the dispatch envelope (512 < chunks <= 2048 of 2048 rows), so the iteration counts stay small (tol = 0,
maxiter <= 9).  1025 x 1025: 514 chunks, the last one of ONE row, n odd.  1024 x 1026: 513 full chunks, the lower edge.
2048 x 2048: 2048 chunks, every resident slot of the chip in use.  Wider stencils: a 7-entry band (UNITS = 8) and a 4-entry band
(UNITS = 4) of constant coefficients, 514 chunks with a ragged last one."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest
import torch

DEV = "cuda:0"
FORM = "cg three-launch"
FUSED5 = "hipk_cg_fuse_update_kernel<5>"
SWITCHES = ("HIPK_CG_FUSE_UPDATE", "HIPK_TEST_CG_FUSE_GIVE_UP", "HIPK_CG_DEFER_X")
# The one stop by the tolerance (1025 x 1025, b = ones, tol = 1e-3) takes the oracle 1301 iterations of a million rows: half a minute
# on a CPU, 40 ms on the GPU.  Its result is recorded -- the counts, the two residuals as bit patterns, SHA-256 of x's bytes -- by
# `python tests/test_gpu_cg_fuse_update.py` (oracle.cg on exactly the test's inputs), so the comparison stays bit for bit.
TOL_STOP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cg_fuse_update_tol_stop.json")


def _digest(x, stats):
    it, info, res, rs = stats
    return {"iterations": int(it), "info": int(info), "residual_norm": float(res).hex(), "recurrence_rs": float(rs).hex(),
            "x_sha256": hashlib.sha256(np.ascontiguousarray(x, dtype=np.float64).tobytes()).hexdigest()}


@functools.lru_cache(maxsize=None)
def _poisson(nx, ny):
    """(device CSR tensor, numpy crow, col, val) of the 5-point Poisson matrix."""
    from pytorch_sparse_solver.utils.matrix_utils import create_poisson_2d_csr
    A = create_poisson_2d_csr(nx, ny, device=DEV)
    return (A, A.crow_indices().cpu().numpy().astype(np.int32), A.col_indices().cpu().numpy().astype(np.int32),
            A.values().cpu().numpy())


@functools.lru_cache(maxsize=None)
def _band(width):
    """A constant-coefficient band of 514 chunks (n = 513 * 2048 + 77): 7 entries per row (symmetric, diagonally dominant: UNITS = 8)
    or 4 entries per row (UNITS = 4)."""
    from test_gpu_coded import banded
    n = 513 * 2048 + 77
    offsets, vals = {7: ([-3000, -1100, -1, 0, 1, 1100, 3000], [-0.5, -1.0, -1.0, 8.0, -1.0, -1.0, -0.5]),
                     4: ([-1100, -1, 0, 1], [-1.0, -1.5, 6.0, -1.5])}[width]
    v = np.asarray(vals)
    crow, col, val = banded(n, offsets, lambda r, k: v[k])
    A = torch.sparse_csr_tensor(torch.from_numpy(crow).to(DEV), torch.from_numpy(col).to(DEV), torch.from_numpy(val).to(DEV), size=(n, n))
    return A, crow.astype(np.int32), col.astype(np.int32), val


def _fresh_handle(hipk, system):
    A = system[0]
    return hipk.CsrHandle(A.crow_indices(), A.col_indices(), A.values(), A.shape)


def _solve(hipk, monkeypatch, h, b, x0, env, kw, work=None):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    x = torch.zeros_like(b) if x0 is None else x0.clone()
    st = hipk.solve("cg", h, b, x, atol=0.0, work=work, **{"maxiter": None, **kw})
    note = hipk.CsrHandle.last_spmv_kernel()
    return x.cpu().numpy(), (st.iterations, st.info, st.residual_norm, st.recurrence_rs), note, hipk.last_solve_form()


def _separate(note, units=5):
    """The note of a solve on the separate kernels: its last product is the true residual's, the chunk walk of the wide kernel."""
    return note.startswith(f"hipk_spmv_sell_wide_kernel<{units},") and note.endswith(",0>")


def _same(a, b):
    return a[1] == b[1] and np.array_equal(a[0].view(np.uint8), b[0].view(np.uint8))


_REFS = {}


def _reference(oracle, system, b, x0, kw):
    """The oracle's solve of a case, computed once per (matrix, b, x0, arguments): the two direction forms share it."""
    key = (system[0].shape, len(system[3]), b.tobytes()[:4096], None if x0 is None else x0.tobytes()[:4096], tuple(sorted(kw.items())))
    if key not in _REFS:
        _REFS[key] = oracle.cg(system[1], system[2], system[3], b, x0=x0, **kw)
    return _REFS[key]


def _check(hipk, oracle, monkeypatch, system, b, x0, env, kw, units=5):
    """The fused arm, the HIPK_CG_FUSE_UPDATE=0 arm and the oracle on one case; returns the iteration count."""
    A, crow, col, val = system
    h = hipk.handle_for(A)
    bd = torch.from_numpy(b).to(DEV)
    x0d = None if x0 is None else torch.from_numpy(x0).to(DEV)
    new = _solve(hipk, monkeypatch, h, bd, x0d, env, kw)
    old = _solve(hipk, monkeypatch, h, bd, x0d, {**env, "HIPK_CG_FUSE_UPDATE": "0"}, kw)
    what = (A.shape, env, kw)
    assert new[2] == f"hipk_cg_fuse_update_kernel<{units}>" and new[3] == FORM, (what, new[2], new[3])
    assert _separate(old[2], units) and old[3] == FORM, (what, old[2], old[3])
    ref = _reference(oracle, system, b, x0, kw)
    refs = (ref.iterations, ref.info, ref.residual_norm, ref.recurrence_rs)
    assert new[1] == old[1], (what, new[1], old[1])
    assert np.array_equal(new[0].view(np.uint8), old[0].view(np.uint8)), what
    assert new[1] == refs, (what, new[1], refs)
    assert np.array_equal(new[0].view(np.uint8), ref.x.view(np.uint8)), what
    return new[1][0]


@pytest.mark.gpu
@pytest.mark.parametrize("defer", ["1", "0"], ids=["defer-x", "x-every-iteration"])
def test_one_row_in_the_last_chunk_cutoffs_of_both_parities_and_one_stop(hipk, oracle, monkeypatch, defer):
    """1025 x 1025, b = ones: maxiter 0 .. 5 with tol = 0 (the deferred x's flush idle and working), then a stop by the tolerance."""
    sysm = _poisson(1025, 1025)
    b = np.ones(1025 * 1025)
    env = {} if defer == "1" else {"HIPK_CG_DEFER_X": "0"}
    for m in range(6):
        assert _check(hipk, oracle, monkeypatch, sysm, b, None, env, dict(tol=0.0, maxiter=m)) == m
    with open(TOL_STOP) as f:
        want = json.load(f)
    assert want["n"] == b.size and want["tol"] == 1e-3 and want["iterations"] > 5
    bd = torch.from_numpy(b).to(DEV)
    h = hipk.handle_for(sysm[0])
    new = _solve(hipk, monkeypatch, h, bd, None, env, dict(tol=1e-3))
    old = _solve(hipk, monkeypatch, h, bd, None, {**env, "HIPK_CG_FUSE_UPDATE": "0"}, dict(tol=1e-3))
    assert new[2] == FUSED5 and _separate(old[2]) and new[3] == old[3] == FORM, (new[2:], old[2:])
    assert _same(new, old), (new[1], old[1])
    assert _digest(new[0], new[1]) == {k: want[k] for k in _digest(new[0], new[1])}, (new[1], want)


@pytest.mark.gpu
def test_random_right_hand_side_and_warm_start(hipk, oracle, monkeypatch):
    rng = np.random.default_rng(5)
    n = 1025 * 1025
    b, x0 = rng.standard_normal(n), rng.standard_normal(n)
    sysm = _poisson(1025, 1025)
    for m in (4, 5):
        assert _check(hipk, oracle, monkeypatch, sysm, b, None, {}, dict(tol=0.0, maxiter=m)) == m
    assert _check(hipk, oracle, monkeypatch, sysm, b, x0, {}, dict(tol=0.0, maxiter=5)) == 5
    assert _check(hipk, oracle, monkeypatch, sysm, b, x0, {"HIPK_CG_DEFER_X": "0"}, dict(tol=0.0, maxiter=4)) == 4


@pytest.mark.gpu
def test_the_lower_edge_of_the_envelope(hipk, oracle, monkeypatch):
    """1024 x 1026: 513 full chunks, taken.  1023 x 1025: 512 chunks, the mid loop's size, not taken."""
    b = np.random.default_rng(6).standard_normal(1024 * 1026)
    for m in (4, 5):
        assert _check(hipk, oracle, monkeypatch, _poisson(1024, 1026), b, None, {}, dict(tol=0.0, maxiter=m)) == m
    A = _poisson(1023, 1025)[0]
    assert (1023 * 1025 + 2047) // 2048 == 512
    bd = torch.ones(1023 * 1025, dtype=torch.float64, device=DEV)
    got = _solve(hipk, monkeypatch, hipk.handle_for(A), bd, None, {}, dict(tol=0.0, maxiter=4))
    assert got[1][0] == 4 and "hipk_cg_fuse_update_kernel" not in got[2], got[1:]


@pytest.mark.gpu
def test_every_resident_slot_in_use_and_the_size_beyond(hipk, oracle, monkeypatch):
    """2048 x 2048: 2048 chunks on 2048 slots, the co-residency edge.  2048 x 2049: chunks of 4096 rows, today's kernels."""
    b = np.random.default_rng(8).standard_normal(2048 * 2048)
    for m in (4, 5):
        assert _check(hipk, oracle, monkeypatch, _poisson(2048, 2048), b, None, {}, dict(tol=0.0, maxiter=m)) == m
    A = _poisson(2048, 2049)[0]
    bd = torch.ones(2048 * 2049, dtype=torch.float64, device=DEV)
    got = _solve(hipk, monkeypatch, hipk.handle_for(A), bd, None, {}, dict(tol=0.0, maxiter=4))
    assert got[1][0] == 4 and got[2].startswith("hipk_spmv_sell_wide_kernel<5,") and got[3] == FORM, got[1:]


@pytest.mark.gpu
@pytest.mark.parametrize("width,units", [(7, 8), (4, 4)])
def test_wider_and_narrower_stencils(hipk, oracle, monkeypatch, width, units):
    """Constant-coefficient bands of 7 and of 4 entries per row: the UNITS = 8 and UNITS = 4 instantiations, 514 chunks, a ragged
    last chunk of 77 rows.  (The two-rows-per-lane kernel takes them: _check asserts both notes.)"""
    sysm = _band(width)
    b = np.random.default_rng(width).standard_normal(sysm[0].shape[0])
    for m in (3, 4):
        assert _check(hipk, oracle, monkeypatch, sysm, b, None, {}, dict(tol=0.0, maxiter=m), units=units) == m


@pytest.mark.gpu
@pytest.mark.parametrize("defer", ["1", "0"], ids=["defer-x", "x-every-iteration"])
def test_the_collector_gives_up(hipk, oracle, monkeypatch, defer):
    """HIPK_TEST_CG_FUSE_GIVE_UP = 0, 1, 4 (the deferred x at both parities): the solve goes on with the separate kernels from that
    iteration and gives the same bits; the handle does not try the fused form again, a fresh handle does."""
    sysm = _poisson(1025, 1025)
    A, crow, col, val = sysm
    b = np.random.default_rng(9).standard_normal(1025 * 1025)
    bd = torch.from_numpy(b).to(DEV)
    kw = dict(tol=0.0, maxiter=9)
    env = {} if defer == "1" else {"HIPK_CG_DEFER_X": "0"}
    ref = _reference(oracle, sysm, b, None, kw)
    refs = (ref.x, (ref.iterations, ref.info, ref.residual_norm, ref.recurrence_rs))
    assert ref.iterations == 9
    sep = _solve(hipk, monkeypatch, hipk.handle_for(A), bd, None, {**env, "HIPK_CG_FUSE_UPDATE": "0"}, kw)
    assert _same(sep, refs) and _separate(sep[2])
    for k in (0, 1, 4):
        h = _fresh_handle(hipk, sysm)
        got = _solve(hipk, monkeypatch, h, bd, None, {**env, "HIPK_TEST_CG_FUSE_GIVE_UP": str(k)}, kw)
        assert _same(got, refs) and _separate(got[2]) and got[3] == FORM, (k, got[1:], refs[1])
        again = _solve(hipk, monkeypatch, h, bd, None, env, kw)          # no hook: the latch of the handle keeps it off
        assert _same(again, refs) and _separate(again[2]), (k, again[1:])
        h.close()
    fresh = _fresh_handle(hipk, sysm)
    got = _solve(hipk, monkeypatch, fresh, bd, None, env, kw)
    assert _same(got, refs) and got[2] == FUSED5, got[1:]
    fresh.close()


@pytest.mark.gpu
def test_workspace_of_exactly_work_bytes_in_every_state(hipk, oracle, monkeypatch):
    """`work` of exactly hipk_cg_work_bytes between guards, filled with 0x00, 0xFF, 0x5A and not refilled: the same solve."""
    from _solve_runner import run_solve_case
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    A, crow, col, val = _poisson(1025, 1025)
    b = np.random.default_rng(10).standard_normal(1025 * 1025)
    kw = dict(tol=0.0, maxiter=5)
    st, x, _ = run_solve_case(hipk, "cg fused 1025x1025", "cg", hipk.handle_for(A), b, None, None, kw, "launch sequence", FORM)
    assert hipk.CsrHandle.last_spmv_kernel() == FUSED5
    ref = oracle.cg(crow, col, val, b, **kw)
    assert (st.iterations, st.info, st.residual_norm, st.recurrence_rs) == (ref.iterations, ref.info, ref.residual_norm, ref.recurrence_rs)
    assert np.array_equal(x.view(np.uint8), ref.x.view(np.uint8))


@pytest.mark.gpu
def test_two_right_hand_sides_back_to_back_on_one_workspace(hipk, oracle, monkeypatch):
    """The second solve finds the first one's flagged words (sequence numbers 1 .. 6 and 1 .. 5 again) in the workspace."""
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
        ref = oracle.cg(crow, col, val, b, tol=0.0, maxiter=m)
        assert got[2] == FUSED5 and got[1] == (ref.iterations, ref.info, ref.residual_norm, ref.recurrence_rs), (m, got[1:])
        assert np.array_equal(got[0].view(np.uint8), ref.x.view(np.uint8)), m


def test_the_fused_kernel_keeps_eight_workgroups_per_cu(monkeypatch):
    """<= 64 VGPRs, <= 80 SGPRs, no scratch and <= 20 480 bytes of static LDS for the three instantiations, from the compiler's
    resource report as tests/test_kernel_resources.py reads it (the LDS figure from the same report)."""
    import os
    import re
    import shutil
    import subprocess
    import test_kernel_resources as kr
    if not os.path.exists(kr.HIPCC) or shutil.which("c++filt") is None:
        pytest.skip("hipcc / c++filt not installed")
    reports = []
    real_run = subprocess.run

    def run(cmd, *a, **k):
        p = real_run(cmd, *a, **k)
        if cmd and cmd[0] == kr.HIPCC:
            reports.append(p.stderr)
        return p

    monkeypatch.setattr(kr.subprocess, "run", run)
    got = kr._vgprs("hipk_cg.hip")
    assert len(reports) == 1
    lds = dict(re.findall(r"Function Name: (\S+).*?LDS Size \[bytes/block\]: (\d+)", reports[0], re.S))
    for units in (4, 5, 8):
        k = f"void hipk_cg_fuse_update_kernel<{units}>"
        assert k in got, (k, sorted(got)[:60])
        assert got[k] <= 64 and kr._vgprs.sgprs[k] <= 80 and kr._vgprs.scratch[k] == 0, (k, got[k], kr._vgprs.sgprs[k], kr._vgprs.scratch[k])
        mangled = [m for m in lds if f"hipk_cg_fuse_update_kernelILi{units}E" in m]
        assert len(mangled) == 1 and int(lds[mangled[0]]) <= 20480, (k, mangled, [lds[m] for m in mangled])


if __name__ == "__main__":   # records TOL_STOP with the CPU oracle (no GPU needed)
    import sys
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [ROOT, os.path.join(ROOT, "pytorch-sparse-linalg-torch-amgx.cg.bicg.gmres_amd")]
    from oracle import oracle as O
    from pytorch_sparse_solver.utils.matrix_utils import create_poisson_2d_csr
    O.build()
    A = create_poisson_2d_csr(1025, 1025, device="cpu")
    b = np.ones(1025 * 1025)
    ref = O.cg(A.crow_indices().numpy().astype(np.int32), A.col_indices().numpy().astype(np.int32), A.values().numpy(), b, tol=1e-3)
    rec = {"n": int(b.size), "tol": 1e-3, **_digest(ref.x, (ref.iterations, ref.info, ref.residual_norm, ref.recurrence_rs))}
    with open(TOL_STOP, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(rec)
