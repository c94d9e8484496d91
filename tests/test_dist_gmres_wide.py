"""Row-partitioned GMRES at restart 32 .. 255: `gmres(A_rb, b_loc, restart=m)` with a RowBlockCSR operand runs
hipk_dist_{p,}gmres_wide_solve -- H in the workspace as in the single-device loop beyond restart 31, and one in-place all-gather of
the multi-dot partials per CGS pass whatever the Arnoldi step.  Every rank gets, bit for bit, its slice of the single-device solve.
CPU: the kernels' register budgets, the exported entry points, the work-bytes functions, and the routing of dist_gmres with the
native layer stubbed.  GPU: ranks share cuda:0 with host-staged collectives (or the device mailboxes); real RCCL at world 1."""
import contextlib
import ctypes
import json
import os
import shutil
import socket
import subprocess
import sys
import types

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "pytorch-sparse-linalg-torch-amgx.cg.bicg.gmres_amd")
for _p in (ROOT, PKG, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from test_kernel_resources import HIPCC, _vgprs  # noqa: E402


# ---------------------------------------------------------------------------------------------------------------------- CPU
@pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("c++filt") is None, reason="hipcc / c++filt not installed")
def test_packed_multidot_and_hreduce_keep_eight_workgroups_per_cu():
    got = _vgprs("hipk_gmres.hip")
    for k in ("void hipk_gm_multidot_packed_kernel<double>", "hipk_gm_hreduce_packed_kernel"):
        assert k in got, (k, sorted(got)[:80])
        assert got[k] <= 64, f"{k}: {got[k]} VGPRs"
        assert _vgprs.sgprs[k] <= 80, f"{k}: {_vgprs.sgprs[k]} SGPRs"
        assert _vgprs.scratch[k] == 0, f"{k}: {_vgprs.scratch[k]} bytes of scratch per lane"


WIDE = ("hipk_dist_gmres_wide_work_bytes", "hipk_dist_gmres_wide_solve", "hipk_dist_pgmres_wide_work_bytes",
        "hipk_dist_pgmres_wide_solve")


def _plan(world=2, rank=0, per=3, slab=64):
    from pytorch_sparse_solver import _hipk
    p = _hipk.DistPlan()
    p.rank, p.world, p.per, p.slab = rank, world, per, slab
    p.n_local, p.n_ext, p.n_global = per * 2048, per * 2048 + 96, world * per * 2048
    p.chunk_rows, p.g_red = 2048, world * per
    return p


def test_wide_entry_points_are_exported_and_bound():
    from pytorch_sparse_solver import _hipk
    L = _hipk.lib()
    for name in WIDE:
        assert name in _hipk.SYMBOLS and hasattr(L, name), name
    assert L.hipk_dist_gmres_wide_work_bytes.restype is ctypes.c_size_t
    assert L.hipk_version() == 300


@pytest.mark.parametrize("pre", ["", "p"])
def test_wide_work_bytes_cover_restart_32_to_255_only(pre):
    """Pure host code: > 0 inside [32, 255], 0 outside; the block for H grows with the restart, the narrow workspace is untouched."""
    from pytorch_sparse_solver import _hipk
    L = _hipk.lib()
    wide = getattr(L, f"hipk_dist_{pre}gmres_wide_work_bytes")
    narrow = getattr(L, f"hipk_dist_{pre}gmres_work_bytes")
    plan = ctypes.byref(_plan())
    got = {r: int(wide(plan, r)) for r in (0, 1, 31, 32, 33, 64, 128, 255, 256, 1000)}
    assert all(got[r] == 0 for r in (0, 1, 31, 256, 1000)), got
    assert 0 < got[32] < got[33] < got[64] < got[128] < got[255], got
    # the wide workspace holds at least the narrow layout at that restart (partials of m + 1 columns, m + 2 vectors)
    assert got[32] > int(narrow(plan, 31))
    assert int(wide(None, 64)) == 0


def _stub_native(monkeypatch, calls):
    """dist_gmres on a CPU-only problem with the native layer stubbed: the loop is declared available, the library's entry points
    record their name and succeed, torch.cuda's stream plumbing is a no-op."""
    import pytorch_sparse_solver.distributed as D
    from pytorch_sparse_solver import _hipk
    from pytorch_sparse_solver.distributed import RowPartition
    from dist_cpu_ops import OracleOps

    class FakeLib:
        def __getattr__(self, name):
            def fn(*args):
                calls.append(name)
                return 4096 if name.endswith("work_bytes") else 0
            return fn

    monkeypatch.setattr(_hipk, "lib", lambda: FakeLib())
    monkeypatch.setattr(D, "native_loop_ok", lambda prob: True)
    monkeypatch.setattr(torch.cuda, "device", lambda dev: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "current_stream", lambda dev=None: types.SimpleNamespace(cuda_stream=0))
    part = RowPartition(64, 1, 0)
    none = torch.zeros(0, dtype=torch.int64)
    plan = types.SimpleNamespace(send_splits=[0], recv_splits=[0], send_first=[-1], n_send=0, n_ghost=0, slab=0,
                                 send_idx=none, ghost_src=none, send_off=none, dest_off=none)
    return types.SimpleNamespace(part=part, plan=plan, ops=OracleOps(), n_ext=64, b=torch.ones(64, dtype=torch.float64),
                                 A={"h": None}, coll_struct=lambda: _hipk.Rccl(1, 1, 1, 1, 1, None))


@pytest.mark.parametrize("pre", ["", "p"])
@pytest.mark.parametrize("restart,entry", [(1, "gmres"), (31, "gmres"), (32, "gmres_wide"), (255, "gmres_wide")])
def test_dist_gmres_routes_restart_to_the_narrow_or_wide_loop(monkeypatch, pre, restart, entry):
    from pytorch_sparse_solver.distributed import dist_gmres
    calls = []
    prob = _stub_native(monkeypatch, calls)
    dinv = torch.ones(max(prob.n_ext, 1), dtype=torch.float64) if pre else None
    x, info, st = dist_gmres(prob, restart=restart, maxiter=1, dinv=dinv)
    assert calls == [f"hipk_dist_{pre}{entry}_work_bytes", f"hipk_dist_{pre}{entry}_solve"], calls
    assert info == 0 and x.numel() == 64


@pytest.mark.parametrize("restart", [0, 256, 1000])
def test_dist_gmres_rejects_restart_outside_1_to_255(monkeypatch, restart):
    from pytorch_sparse_solver.distributed import dist_gmres
    calls = []
    prob = _stub_native(monkeypatch, calls)
    with pytest.raises(ValueError, match=r"\[1, 255\]"):
        dist_gmres(prob, restart=restart)
    assert calls == []


# ---------------------------------------------------------------------------------------------------- GPU (ranks share cuda:0)
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run(world, task, args, tmp_path, env_extra=None, timeout=300):
    out = str(tmp_path / f"wide_{task}_{world}_{abs(hash(json.dumps(args, sort_keys=True)))}.json")
    for _attempt in range(3):   # a port found free can be taken before the store binds it (EADDRINUSE): try another one
        port = _free_port()
        procs = []
        for r in range(world):
            env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1",
                       MASTER_PORT=str(port), OMP_NUM_THREADS="1", **(env_extra or {}))
            procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "_dist_gmres_wide_worker.py"), task, out,
                                           json.dumps(args)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
        logs = []
        for p in procs:
            try:
                o, _ = p.communicate(timeout=timeout)
            except subprocess.TimeoutExpired:
                for q in procs:
                    q.kill()
                raise
            logs.append(o.decode(errors="replace"))
        if all(p.returncode == 0 for p in procs) or not any("EADDRINUSE" in lg for lg in logs):
            break
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)
    with open(out) as f:
        return json.load(f)


def _check(r, maxiter=-1):
    keep = json.dumps({k: v for k, v in r.items() if k != "counts"})
    assert r["single_equal"], keep
    for mine in r["ranks"]:
        assert mine == r["single"], keep          # info, cycles, matvecs, residual norm, breakdown: exactly
    if maxiter > 0:
        assert r["single"]["iterations"] == maxiter, keep


@pytest.mark.gpu
@pytest.mark.parametrize("world,halo,kind,nx,ny,restart,method,jacobi,maxiter,extra", [
    (1, "p2p", "vardiff", 96, 64, 32, "batched", False, 1, {"oracle": True}),
    (2, "p2p", "vardiff", 96, 64, 40, "batched", False, 2, {"oracle": True}),
    (3, "allgather", "convdiff", 96, 64, 64, "incremental", False, 3, {}),
    (2, "p2p", "convdiff", 128, 96, 128, "batched", True, 1, {}),
    (3, "allgather", "vardiff", 160, 120, 255, "batched", False, 1, {}),
    (2, "p2p", "vardiff", 200, 150, 255, "incremental", True, 2, {}),
    (3, "allgather", "vardiff", 96, 64, 40, "incremental", True, -1, {}),          # to convergence
    (2, "p2p", "convdiff", 96, 64, 64, "batched", False, -1, {"warm": True}),       # warm start, to convergence
])
def test_wide_gmres_is_the_single_device_solve(world, halo, kind, nx, ny, restart, method, jacobi, maxiter, extra, tmp_path):
    args = dict({"kind": kind, "nx": nx, "ny": ny, "restart": restart, "solve_method": method, "jacobi": jacobi,
                 "maxiter": maxiter, "tol": 1e-8}, **extra)
    r = _run(world, "hip", args, tmp_path, env_extra={"HIPK_DIST_HALO": halo})
    _check(r, maxiter)
    assert len(r["n_local"]) == world and all(v > 0 for v in r["n_local"]), r["n_local"]
    if extra.get("oracle"):
        assert r["oracle_equal"], r["oracle"]
        assert r["oracle"]["iterations"] == r["single"]["iterations"], r["oracle"]
    if maxiter < 0:
        assert r["single"]["info"] == 0, r["single"]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,world,method", [("scaled_identity", 2, "batched"), ("scaled_identity", 3, "incremental"),
                                               ("fewvals", 2, "batched"), ("fewvals", 3, "incremental")])
def test_wide_gmres_happy_breakdown_inside_a_cycle(kind, world, method, tmp_path):
    """Krylov spaces that close long before step 64 of a GMRES(64) cycle (2 I: at the first step; four 2 x 2 Jordan blocks: at step
    8 in exact arithmetic): the breakdown flag, counts and x of the single-device solve."""
    args = {"kind": kind, "nx": 96, "ny": 64, "restart": 64, "solve_method": method, "maxiter": 2, "tol": 1e-10}
    r = _run(world, "hip", args, tmp_path, env_extra={"HIPK_DIST_HALO": "p2p" if world == 2 else "allgather"})
    _check(r)
    if kind == "scaled_identity":
        assert r["single"]["breakdown"] == 1 and r["single"]["matvecs"] == 4 and r["single"]["info"] == 0, r["single"]


def _halo(c, world, halo):
    if world > 1 and halo == "allgather":
        return [["all_gather", c["slab"], False]]
    H = []
    if world > 1:
        for peer, (ns, nr) in enumerate(zip(c["send_counts"], c["recv_counts"])):
            H += ([["send", ns, peer]] if ns else []) + ([["recv", nr, peer]] if nr else [])
    return H


@pytest.mark.gpu
@pytest.mark.parametrize("world,halo", [(2, "p2p"), (3, "allgather")])
def test_wide_gmres_makes_five_all_gathers_per_arnoldi_step(world, halo, tmp_path):
    """Every collective call of the wide loop (plain and Jacobi, restart 40, one and two cycles), in order: per Arnoldi step the
    halo of v_k, then in-place all-gathers of per, (k + 1) per, per, (k + 1) per, per doubles, none of them in a group; after the
    steps the residual's exchange; the set-up and final blocks of the narrow loop."""
    m = 40
    args = {"kind": "vardiff", "nx": 96, "ny": 64, "restart": m, "solve_method": "batched", "maxiter": 1, "tol": 1e-8,
            "count": True}
    r = _run(world, "hip", args, tmp_path, env_extra={"HIPK_DIST_HALO": halo})
    _check(r, 1)
    for c in r["counts"]:
        per, H = c["per"], _halo(c, world, halo)
        alone = ([["group_start"]] + H + [["group_end"]]) if (H and halo == "p2p") else H
        agi = ["all_gather", per, True]
        cycle = []
        for k in range(m):
            blk = ["all_gather", (k + 1) * per, True]
            cycle += alone + [agi, blk, agi, blk, agi]
        cycle += alone + [agi]
        final = alone + [agi, agi]
        setup = {"gmres": [agi] + alone + [agi], "pgmres": [agi] + alone + [agi, agi]}
        for name in ("gmres", "pgmres"):
            for k in (1, 2):
                assert c["traces"][f"{name}_{k}"] == setup[name] + k * cycle + final, (name, k, world, halo)


@pytest.mark.gpu
def test_wide_gmres_on_device_mailboxes_through_the_product_problem(tmp_path):
    """HIPK_DIST_COMM=p2p at world 1 through RowBlockCSR's own DistProblem, restart 255: the mailbox takes the multi-dot block."""
    args = {"kind": "vardiff", "nx": 96, "ny": 64, "restart": 255, "solve_method": "batched", "maxiter": 1, "tol": 1e-8,
            "comm": "product"}
    r = _run(1, "hip", args, tmp_path, env_extra={"HIPK_DIST_COMM": "p2p"})
    _check(r, 1)
    assert r["comm"] == ["p2p-mailbox"], r["comm"]


@pytest.mark.gpu
def test_wide_gmres_on_device_mailboxes_at_world_2(tmp_path):
    args = {"kind": "convdiff", "nx": 96, "ny": 64, "restart": 128, "solve_method": "incremental", "maxiter": 2, "tol": 1e-8,
            "comm": "mailbox"}
    _check(_run(2, "hip", args, tmp_path), 2)


@pytest.mark.gpu
def test_wide_gmres_on_large_row_blocks(tmp_path):
    """Two ranks of 1.15 M rows (1536 x 1500 variable diffusion) sharing cuda:0, GMRES(40), one cycle: bitwise."""
    args = {"kind": "vardiff", "nx": 1536, "ny": 1500, "restart": 40, "solve_method": "batched", "maxiter": 1, "tol": 1e-12}
    r = _run(2, "hip", args, tmp_path, env_extra={"HIPK_DIST_HALO": "p2p"}, timeout=900)
    _check(r, 1)
    assert min(r["n_local"]) >= 1_150_000, r["n_local"]


@pytest.mark.gpu
def test_wide_entry_points_report_errors_at_world_1(tmp_path):
    r = _run(1, "hip_errors", {"nx": 24, "ny": 20, "fail_nth": 4}, tmp_path)
    ARG, HIP, WORKSPACE = -1, -2, -5
    for pre in ("", "p"):
        got = r[pre + "gmres"]
        assert got["nccl"] == [HIP, f"hipk_dist_{pre}gmres_wide_solve: all_gather(partials) failed (ncclResult 7)"], got
        assert got["work"][0] == WORKSPACE and got["work"][1].endswith(": work too small"), got
        for case in ("restart31", "restart256"):
            assert got[case][0] == ARG and got[case][1].endswith("restart must be in [32, 255]"), got
        assert got["bytes"]["31"] == 0 == got["bytes"]["256"] and got["bytes"]["32"] > 0 and got["bytes"]["255"] > 0, got


@pytest.mark.gpu
def test_wide_gmres_nccl_world1_equals_single_gpu(tmp_path):
    """Real RCCL at world size 1: GMRES(64) on the RowBlockCSR through the direct communicator is the single-device solve."""
    code = r'''
import os, sys, json, torch, torch.distributed as dist
sys.path[:0] = [%r, %r]
import pytorch_sparse_solver as pss
from pytorch_sparse_solver.module_a import JacobiPreconditioner, gmres, get_last_stats
from pytorch_sparse_solver.utils.matrix_utils import create_variable_diffusion_2d_csr
dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
A = create_variable_diffusion_2d_csr(96, 64, device="cuda:0")
b = torch.randn(96 * 64, dtype=torch.float64, generator=torch.Generator().manual_seed(3)).to("cuda:0")
Arb = pss.RowBlockCSR.from_global_csr(A)
out = {}
for name, kw in (("plain", {}), ("jacobi", {"M": JacobiPreconditioner(Arb)})):
    x, info = gmres(Arb, b, tol=1e-8, restart=64, **kw)
    st = get_last_stats()
    kr = {"M": JacobiPreconditioner(A)} if kw else {}
    xr, info_r = gmres(A, b, tol=1e-8, restart=64, **kr)
    sr = get_last_stats()
    out[name] = {"equal": bool(torch.equal(x, xr)), "info": [info, info_r], "it": [st.iterations, sr.iterations],
                 "mv": [st.matvecs, sr.matvecs], "res": [st.residual_norm, sr.residual_norm]}
out["comm"] = Arb._prob.comm_kind
print(json.dumps(out))
dist.destroy_process_group()
''' % (ROOT, PKG)
    for _ in range(3):
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
        p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
        if p.returncode == 0 or "EADDRINUSE" not in p.stderr:
            break
    assert p.returncode == 0, p.stdout + p.stderr
    r = json.loads(p.stdout.strip().splitlines()[-1])
    assert r["comm"] == "rccl-direct", r
    for name in ("plain", "jacobi"):
        s = r[name]
        assert s["equal"] and s["info"][0] == s["info"][1] and s["it"][0] == s["it"][1], r
        assert s["mv"][0] == s["mv"][1] and s["res"][0] == s["res"][1], r
