"""Jacobi preconditioning on the row-partitioned operand: `cg / bicgstab / gmres(A_rb, b_loc, M=P)` and
`SparseSolver().solve(A_rb, b_loc, M=P)` with P = JacobiPreconditioner of the RowBlockCSR or of the replicated global matrix.
Every rank calls with its block and gets, bit for bit, the single-device preconditioned solve of the global system.
CPU: gloo world 2 / 3 with the CPU ops double (the preconditioner's set-up and the errors).  GPU: ranks share cuda:0, the
C-driven loops (hipk_dist_pcg_solve, hipk_dist_pbicgstab_solve, hipk_dist_pgmres_solve) with host-staged collectives or the
device mailboxes; real RCCL at world 1."""
import json
import os
import socket
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "pytorch-sparse-linalg-torch-amgx.cg.bicg.gmres_amd")


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run(world, task, args, tmp_path, env_extra=None, timeout=300):
    out = str(tmp_path / f"jacobi_{task}_{world}_{abs(hash(json.dumps(args, sort_keys=True)))}.json")
    for _attempt in range(3):   # a port found free can be taken before the store binds it (EADDRINUSE): try another one
        port = _free_port()
        procs = []
        for r in range(world):
            env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1",
                       MASTER_PORT=str(port), OMP_NUM_THREADS="1", **(env_extra or {}))
            procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "_dist_jacobi_worker.py"), task, out, json.dumps(args)],
                                          env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
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


# ---------------------------------------------------------------------------------------------------- CPU (gloo, ops double)
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("kind,nx,ny", [("vardiff", 40, 37), ("random_spd", 80, 77)])
def test_row_block_jacobi_dinv_is_the_rank_slice_of_the_global_one(world, kind, nx, ny, tmp_path):
    pieces = _run(world, "dinv", {"kind": kind, "nx": nx, "ny": ny}, tmp_path)
    assert all(p["equal"] for p in pieces), pieces
    assert all(p["shape"] == [nx * ny, nx * ny] for p in pieces)
    assert sum(p["n"] for p in pieces) == nx * ny and pieces[0]["rows"][0] == 0 and pieces[-1]["rows"][1] == nx * ny


@pytest.mark.parametrize("world", [2, 3])
def test_zero_diagonal_on_one_rank_raises_on_every_rank(world, tmp_path):
    pieces = _run(world, "zero", {"kind": "vardiff", "nx": 40, "ny": 37}, tmp_path, timeout=120)
    assert all("zero on the diagonal" in p["raised"] for p in pieces), pieces


@pytest.mark.parametrize("world", [2, 3])
def test_row_block_preconditioner_errors(world, tmp_path):
    pieces = _run(world, "errors", {"kind": "vardiff", "nx": 40, "ny": 37}, tmp_path)
    for p in pieces:
        for name in ("callable", "block", "matrix"):
            assert p[name].startswith("ValueError") and "preconditioners" in p[name], p
        assert p["wrong_size"].startswith("ValueError") and "JacobiPreconditioner of shape" in p["wrong_size"], p
        for method in ("cg", "bicgstab", "gmres"):
            assert p["cpu_" + method].startswith("RuntimeError") and "C-driven loop" in p["cpu_" + method], p


def test_row_block_preconditioner_errors_without_a_process_group():
    """One-rank block, no process group: a wrong-size Jacobi raises ValueError before anything else is looked at."""
    import torch
    from pytorch_sparse_solver import RowBlockCSR
    from pytorch_sparse_solver.module_a import JacobiPreconditioner, bicgstab, gmres
    from pytorch_sparse_solver.utils.matrix_utils import create_variable_diffusion_2d_csr
    A = create_variable_diffusion_2d_csr(8, 8)
    Arb = RowBlockCSR.from_global_csr(A)
    b = torch.ones(64, dtype=torch.float64)
    P = JacobiPreconditioner(Arb)
    assert P.shape == (64, 64) and P.row_range == (0, 64) and torch.equal(P.dinv, JacobiPreconditioner(A).dinv)
    with pytest.raises(ValueError, match="JacobiPreconditioner of shape"):
        bicgstab(Arb, b, M=JacobiPreconditioner(create_variable_diffusion_2d_csr(8, 9)))
    with pytest.raises(ValueError, match="preconditioners"):
        gmres(Arb, b, M=lambda v: v)


# ---------------------------------------------------------------------------------------------------- GPU (ranks share cuda:0)
def _check(r, maxiter=-1):
    keep = json.dumps(r)
    assert r["bitwise_equal"], keep
    assert r["single_equal"], keep
    assert set(r["info"]) == {r["ref_info"]} == {r["single_info"]}, keep
    assert set(r["iterations"]) == {r["ref_iterations"]} == {r["single_iterations"]}, keep
    assert set(r["residual_norm"]) == {r["ref_residual_norm"]} == {r["single_residual_norm"]}, keep
    assert r["second_bitwise_equal"] and set(r["second_info"]) == {r["ref2_info"]}, keep
    assert set(r["second_iterations"]) == {r["ref2_iterations"]}, keep
    assert set(r["preconditioner"]) == {"jacobi"}
    if maxiter > 0:
        assert set(r["iterations"]) == {maxiter}, keep


@pytest.mark.gpu
@pytest.mark.parametrize("world,kind,nx,ny,solver,pmode,halo,entry,maxiter", [
    (2, "vardiff", 96, 64, "cg", "local", "p2p", "solver", -1),
    (3, "vardiff", 96, 64, "cg", "global", "allgather", "module_a", -1),
    (2, "random_spd", 80, 77, "cg", "local", "allgather", "module_a", -1),
    (3, "random_spd", 96, 64, "cg", "global", "p2p", "solver", -1),
    (2, "vardiff", 96, 64, "cg", "local", "p2p", "module_a", 9),
    (2, "convdiff", 96, 64, "bicgstab", "local", "p2p", "solver", -1),
    (3, "vardiff", 96, 64, "bicgstab", "global", "allgather", "module_a", -1),
    (2, "vardiff", 96, 64, "bicgstab", "local", "allgather", "module_a", 9),
    (2, "convdiff", 96, 64, "gmres", "global", "p2p", "solver", -1),
    (3, "vardiff", 96, 64, "gmres", "local", "allgather", "module_a", -1),
    (2, "vardiff", 96, 64, "gmres_incremental", "local", "p2p", "module_a", 20),
    (2, "convdiff", 96, 64, "gmres_incremental", "global", "allgather", "solver", 2),
])
def test_row_partitioned_jacobi_solves_shared_gpu(world, kind, nx, ny, solver, pmode, halo, entry, maxiter, tmp_path):
    """Every rank's x concatenates to the oracle's preconditioned solve and to the single-device one, bit for bit; info, iteration
    (cycle) count and residual norm are the same on every rank; a second solve, warm-started, on the cached plan and dinv."""
    args = {"kind": kind, "nx": nx, "ny": ny, "solver": solver, "pmode": pmode, "entry": entry, "tol": 1e-8, "maxiter": maxiter}
    r = _run(world, "hip", args, tmp_path, env_extra={"HIPK_DIST_HALO": halo})
    _check(r, maxiter)


def _expected_traces(c, world, halo):
    """The collective calls of one rank's six C loops, per solver: (set-up, one iteration or cycle, final) blocks, built from the
    halo mode and this rank's peer counts.  A halo is the neighbour send/recv pairs (p2p) or one all-gather of padded slabs; a
    p2p rank with nothing to send or receive has none.  GMRES completes its global partial arrays in place, with restart 3."""
    GS, GE = ["group_start"], ["group_end"]
    ag, agi = ["all_gather", c["per"], False], ["all_gather", c["per"], True]
    H = []
    if world > 1 and halo == "allgather":
        H = [["all_gather", c["slab"], False]]
    elif world > 1:
        for peer, (ns, nr) in enumerate(zip(c["send_counts"], c["recv_counts"])):
            H += ([["send", ns, peer]] if ns else []) + ([["recv", nr, peer]] if nr else [])

    def group(calls, when=world > 1):
        return [GS] + calls + [GE] if when else calls
    alone = group(H, bool(H) and halo == "p2p")          # a stand-alone halo exchange: the pairs in a group, the slabs alone
    cg = (alone + [ag, ag] + alone, [ag] + group([ag] + H), alone + [ag, ag])
    pcg = (alone + [ag, ag] + group([ag] + H, world > 1 and bool(H)), [ag] + group([ag, ag] + H), alone + [ag, ag])
    bi = (group(H) + [ag, ag], group(H) + [ag] + group([ag] + H) + group([ag, ag]) + group([ag, ag]), group(H) + [ag, ag])
    cycle = []
    for k in range(3):
        cycle += alone + [agi] + 2 * (group([agi] * (k + 1)) + [agi])
    cycle += alone + [agi]                                   # the residual after the cycle
    gm_final = alone + [agi, agi]
    return {"cg": cg, "pcg": pcg, "bicgstab": bi, "pbicgstab": bi,
            "gmres": ([agi] + alone + [agi], cycle, gm_final), "pgmres": ([agi] + alone + [agi, agi], cycle, gm_final)}


@pytest.mark.gpu
@pytest.mark.parametrize("world,halo", [(2, "p2p"), (3, "allgather")])
def test_row_partitioned_jacobi_cg_keeps_the_collective_count(world, halo, tmp_path):
    """Every collective call of the six row-partitioned loops (cg, bicgstab, gmres, plain and with Jacobi), in order, on every
    rank: the set-up block, one identical block per iteration (GMRES: per restart cycle) at two maxiter values, the final block.
    The <r,z> partials ride in the group of the <r,r> partials and the halo of r: a Jacobi CG iteration makes exactly as many
    group_end calls as a plain CG iteration on the same partition."""
    args = {"kind": "vardiff", "nx": 96, "ny": 64, "solver": "cg", "pmode": "local", "entry": "module_a", "tol": 1e-8,
            "maxiter": -1, "count": True}
    r = _run(world, "hip", args, tmp_path, env_extra={"HIPK_DIST_HALO": halo})
    _check(r)
    for c in r["counts"]:
        tr = c["traces"]
        for name, (setup, step, final) in _expected_traces(c, world, halo).items():
            for k in ((1, 2) if name.endswith("gmres") else (3, 8)):
                assert tr[f"{name}_{k}"] == setup + k * step + final, (name, k, c)
        ends = {name: sum(call == ["group_end"] for call in calls) for name, calls in tr.items()}
        assert ends["pcg_8"] - ends["pcg_3"] == ends["cg_8"] - ends["cg_3"] == 5, ends      # one grouped exchange per iteration


@pytest.mark.gpu
def test_row_partitioned_entry_points_report_errors_at_world_1(tmp_path):
    """World 1, host-staged collectives, all six entry points: a failed all_gather returns HIPK_ERR_HIP with the entry point's
    ncclResult text; a single bad argument returns its code and message."""
    r = _run(1, "hip_errors", {"nx": 24, "ny": 20, "fail_nth": 4}, tmp_path)
    ARG, HIP, ALIGN, WORKSPACE = -1, -2, -3, -5
    for solver in ("cg", "bicgstab", "gmres"):
        for pre in ("", "p"):
            got = r[pre + solver]
            assert got["nccl"] == [HIP, f"hipk_dist_{pre}{solver}_solve: all_gather(partials) failed (ncclResult 7)"], got
            want = {"null": (ARG, "null argument"), "work": (WORKSPACE, "work too small"), "rank": (ARG, "rank / world"),
                    "align": (ALIGN, "work must be 256-byte, x / b / dinv 16-byte aligned" if pre else
                              "work must be 256-byte, x / b 16-byte aligned")}
            if solver == "gmres":
                want["restart"] = (ARG, "restart must be in [1, 31]")
            if pre:
                want["dinv"] = (ARG, "null argument")
            assert set(got) == set(want) | {"nccl"}, got
            for case, (code, text) in want.items():
                assert got[case][0] == code and got[case][1].endswith(": " + text), (pre + solver, case, got[case])


@pytest.mark.gpu
def test_row_partitioned_jacobi_cg_on_device_mailboxes_with_fused_area(tmp_path):
    """HIPK_DIST_COMM=fused: the Jacobi CG declines the fused exchanges and runs the mailbox collectives -- the same bits."""
    args = {"kind": "vardiff", "nx": 96, "ny": 64, "solver": "cg", "pmode": "local", "entry": "module_a", "tol": 1e-8,
            "maxiter": -1, "comm": "fused"}
    _check(_run(2, "hip", args, tmp_path))


@pytest.mark.gpu
@pytest.mark.parametrize("solver,maxiter", [("cg", 20), ("bicgstab", 10), ("gmres", 1)])
def test_row_partitioned_jacobi_on_large_row_blocks(solver, maxiter, tmp_path):
    """Row blocks of the size a GPU really gets (1536 x 1500 variable diffusion, 1.15 M rows per rank, two ranks sharing cuda:0):
    the offset-coded sliced-ELL SpMV (too many distinct values for the dictionary-coded forms) with the row scaling; a few
    iterations, bitwise equal to the oracle."""
    args = {"kind": "vardiff", "nx": 1536, "ny": 1500, "solver": solver, "pmode": "local", "entry": "module_a", "tol": 1e-12,
            "maxiter": maxiter, "restart": 8}
    r = _run(2, "hip", args, tmp_path, timeout=900)
    _check(r, maxiter)
    for k in r["spmv_kernel"]:
        assert k.startswith("hipk_spmv_sell_"), r["spmv_kernel"]


@pytest.mark.gpu
def test_row_partitioned_jacobi_nccl_world1_equals_single_gpu(tmp_path):
    """Real RCCL at world size 1: the three Jacobi loops through the direct communicator equal the single-device solves."""
    code = r'''
import os, sys, json, torch, torch.distributed as dist
sys.path[:0] = [%r, %r]
import pytorch_sparse_solver as pss
from pytorch_sparse_solver.module_a import JacobiPreconditioner, bicgstab, cg, gmres, get_last_stats
from pytorch_sparse_solver.utils.matrix_utils import create_variable_diffusion_2d_csr
dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
A = create_variable_diffusion_2d_csr(96, 64, device="cuda:0")
b = torch.randn(96 * 64, dtype=torch.float64, generator=torch.Generator().manual_seed(3)).to("cuda:0")
Arb = pss.RowBlockCSR.from_global_csr(A)
P = JacobiPreconditioner(Arb)
out = {}
for name, fn, kw in (("cg", cg, {}), ("bicgstab", bicgstab, {}), ("gmres", gmres, {"restart": 15})):
    x, info = fn(Arb, b, tol=1e-8, M=P, **kw)
    st = get_last_stats()
    xr, info_r = fn(A, b, tol=1e-8, M=JacobiPreconditioner(A), **kw)
    sr = get_last_stats()
    out[name] = {"equal": bool(torch.equal(x, xr)), "info": [info, info_r], "it": [st.iterations, sr.iterations],
                 "res": [st.residual_norm, sr.residual_norm], "pre": st.preconditioner}
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
    for name in ("cg", "bicgstab", "gmres"):
        s = r[name]
        assert s["equal"] and s["info"][0] == s["info"][1] and s["it"][0] == s["it"][1] and s["res"][0] == s["res"][1], r
        assert s["pre"] == "jacobi", r
