"""The Chebyshev polynomial preconditioner on the row-partitioned operand: `cg(A_rb, b_loc, M=P)` and
`SparseSolver().solve(A_rb, b_loc, method='cg', M=P)` with P = `ChebyshevPreconditioner.for_row_block(A_rb, ...)` or a
ChebyshevPreconditioner of the replicated global matrix, and `P(v_loc)` on its own.  Every rank calls with its block and gets, bit
for bit, its slice of the single-device `cg(A, b, M=ChebyshevPreconditioner(A, ...))` / of `ChebyshevPreconditioner(A)(v)`.

CPU: gloo world 2 / 3 with the CPU ops double -- the constructor's coefficients, the torch form of the apply, the errors.
GPU: ranks share cuda:0, each a fresh child process; hipk_dist_cheb_apply and hipk_dist_chebcg_solve with host-staged collectives,
real RCCL at world 1.  Every comparison is torch.equal / array_equal or integer equality.

Which form of a Chebyshev step a rank block takes (asserted from the kernel note in every case).  A block's handle is built like any
other: constant-coefficient stencils get the dictionary-coded sliced-ELL form, and below 512 reduction chunks per block (about
1 M rows) with chunks of fewer than 32 tiles that form runs its one-row-per-lane kernels, which have no Chebyshev epilogue -- so
with the default dispatch no block small enough for a quick test takes one launch per step.  The epilogue instantiations are
reached the way tests/test_gpu_chebyshev.py reaches them: HIPK_SPMV_CODED=0 puts the block on the plain tile kernel, whose twin
hipk_spmv_cheb_kernel<double,1280> runs at any size (the 100 x 61 and 96 x 64 Poisson cases), and HIPK_SPMV_SELL_STRIDED=1 selects
the grouped walk of the two-rows-per-lane kernel, hipk_spmv_sell_wide_kernel<5,28,1> -- what a rank of BASELINE config 5 runs, where
a chunk has 128 tiles (the 600 x 1024 case)."""
import json
import os
import socket
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "pytorch-sparse-linalg-torch-amgx.cg.bicg.gmres_amd")
STEP = " + hipk_cheb_step_kernel<double>"
TILE_CHEB = "hipk_spmv_cheb_kernel<double,1280>"
WIDE_CHEB = "hipk_spmv_sell_wide_kernel<5,28,1>"


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run(world, task, args, tmp_path, env_extra=None, timeout=300):
    out = str(tmp_path / f"cheb_{task}_{world}_{abs(hash(json.dumps(args, sort_keys=True)))}.json")
    for _attempt in range(3):   # a port found free can be taken before the store binds it (EADDRINUSE): try another one
        port = _free_port()
        procs = []
        for r in range(world):
            env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1",
                       MASTER_PORT=str(port), OMP_NUM_THREADS="1", **(env_extra or {}))
            procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "_dist_chebyshev_worker.py"), task, out, json.dumps(args)],
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
def test_for_row_block_has_the_global_coefficients_on_every_rank(world, kind, nx, ny, tmp_path):
    """c0, c1, c2, scale, lmin, lmax (and the packed array) of ChebyshevPreconditioner(A_global) with the same arguments, bitwise,
    on every rank; dinv the rank's slice: degree 1, 3, 6, normalize both ways, lmax defaulted (Gershgorin, MAX over ranks) and given."""
    pieces = _run(world, "coef", {"kind": kind, "nx": nx, "ny": ny}, tmp_path)
    n = nx * ny
    assert pieces[0]["rows"][0] == 0 and pieces[-1]["rows"][1] == n
    for p in pieces:
        assert len(p["cases"]) == 12
        for c in p["cases"]:
            assert c["coef_equal"] and c["dinv_equal"], c
            assert c["shape"] == [n, n] and c["row_range"] == p["rows"] and c["degree_attr"] == c["degree"], c
            assert c["counters"] == [0, 0], c


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("kind,nx,ny", [("vardiff", 40, 37), ("random_spd", 80, 77)])
def test_row_block_apply_on_cpu_vectors_equals_the_global_apply(world, kind, nx, ny, tmp_path):
    pieces = _run(world, "apply", {"kind": kind, "nx": nx, "ny": ny}, tmp_path)
    for p in pieces:
        assert p["equal"] == {"1": True, "2": True, "5": True}, pieces
        assert p["counters"] == [1, 5], p


@pytest.mark.parametrize("world", [2, 3])
def test_nonpositive_diagonal_on_one_rank_raises_on_every_rank(world, tmp_path):
    pieces = _run(world, "zero", {"kind": "vardiff", "nx": 40, "ny": 37}, tmp_path, timeout=120)
    assert all("zero or negative entry on the diagonal" in p["raised"] for p in pieces), pieces


@pytest.mark.parametrize("world", [2, 3])
def test_row_block_chebyshev_errors(world, tmp_path):
    pieces = _run(world, "errors", {"kind": "vardiff", "nx": 40, "ny": 37}, tmp_path)
    for p in pieces:
        for name in ("bicgstab", "gmres", "solver_gmres"):
            assert p[name].startswith("ValueError") and "runs under cg only" in p[name], p
        for name in ("cpu_cg", "cpu_cg_global"):
            assert p[name].startswith("RuntimeError") and "C-driven loop" in p[name], p
        assert p["constructor"].startswith("ValueError") and "not available on a RowBlockCSR" in p["constructor"], p
        assert p["wrong_rows"].startswith("ValueError") and "ChebyshevPreconditioner of rows" in p["wrong_rows"], p
        for name in ("wrong_shape", "wrong_shape_global"):
            assert p[name].startswith("ValueError") and "ChebyshevPreconditioner of shape" in p[name], p
        assert p["callable"].startswith("ValueError") and "preconditioners" in p["callable"], p


def test_for_row_block_without_a_process_group():
    """No process group: the world is 1, nothing is exchanged, and the construction equals the global one."""
    import torch
    from pytorch_sparse_solver import RowBlockCSR
    from pytorch_sparse_solver.module_a import ChebyshevPreconditioner, bicgstab
    from pytorch_sparse_solver.utils.matrix_utils import create_variable_diffusion_2d_csr
    A = create_variable_diffusion_2d_csr(23, 19)
    Arb = RowBlockCSR.from_global_csr(A)
    for degree, normalize, lmax in ((1, True, None), (3, False, None), (6, True, 2.5)):
        P = ChebyshevPreconditioner.for_row_block(Arb, degree=degree, normalize=normalize, lmax=lmax)
        G = ChebyshevPreconditioner(A, degree=degree, normalize=normalize, lmax=lmax)
        assert isinstance(P, ChebyshevPreconditioner)
        for k in ("degree", "c0", "c1", "c2", "scale", "lmin", "lmax", "applies", "spmvs"):
            assert getattr(P, k) == getattr(G, k), k
        assert list(P._coef) == list(G._coef) and torch.equal(P.dinv, G.dinv)
        assert P.shape == (437, 437) and P.row_range == (0, 437)
    with pytest.raises(ValueError, match="not available on a RowBlockCSR"):
        ChebyshevPreconditioner(Arb)
    with pytest.raises(ValueError, match="runs under cg only"):
        bicgstab(Arb, torch.ones(437, dtype=torch.float64), M=P)
    with pytest.raises(ValueError, match="lmin < lmax"):
        ChebyshevPreconditioner.for_row_block(Arb, lmax=1.0, lmin=2.0)
    with pytest.raises(ValueError, match="degree"):
        ChebyshevPreconditioner.for_row_block(Arb, degree=33)


# ---------------------------------------------------------------------------------------------------- GPU (ranks share cuda:0)
def _check_apply(r, want):
    """want(fused switch) -> (predicate on a kernel note, its description); every rank, every degree."""
    keep = json.dumps(r)
    assert set(r["cases"]) == {f"{m}/{f}" for m in (1, 2, 5) for f in "10"}, keep
    for key, c in r["cases"].items():
        assert c["mirror_equal"] and c["single_equal"], (key, keep)
        ok, what = want(key.split("/")[1])
        assert all(ok(note) for note in c["notes"]), (key, what, c["notes"])
    assert r["solve_after_equal"] and set(r["solve_after_info"][0]) == {r["solve_after_info"][1]}, keep


def _two_launches(note):
    return note.endswith(STEP)


@pytest.mark.gpu
@pytest.mark.parametrize("world,kind,nx,ny,halo", [(2, "vardiff", 100, 61, "p2p"), (3, "vardiff", 96, 64, "allgather"),
                                                   (2, "poisson", 100, 61, "allgather"), (3, "poisson", 96, 64, "p2p")])
def test_row_block_apply_two_launches_per_step(world, kind, nx, ny, halo, tmp_path):
    """hipk_dist_cheb_apply, concatenated over the ranks, against the numpy mirror and the single-device hipk_cheb_apply, degree
    1, 2 and 5.  100 x 61 at world 2: 6100 rows in chunks of 2048, so the last rank's block is ragged, the ghost count 61 is odd
    and n_ext is no multiple of 4; 96 x 64 at world 3: the middle rank has ghosts on both sides.  Default dispatch: these blocks'
    SpMV kernels have no Chebyshev epilogue, every step is SpMV + hipk_cheb_step_kernel on every rank, with HIPK_CHEB_FUSED unset
    and 0 alike.  A solve on the same operand after the applies is unaffected."""
    r = _run(world, "hip_apply", {"kind": kind, "nx": nx, "ny": ny}, tmp_path, env_extra={"HIPK_DIST_HALO": halo})
    _check_apply(r, lambda fused: (_two_launches, "SpMV" + STEP))
    if (world, nx, ny) == (2, 100, 61):
        assert r["n_local"] == [4096, 2004] and r["n_ghost"] == [61, 61] and r["n_ext"][0] % 4 == 1, r["n_ext"]
    else:
        assert r["n_local"] == [2048, 2048, 2048] and r["n_ghost"] == [64, 128, 64], r


@pytest.mark.gpu
@pytest.mark.parametrize("world,nx,ny,halo", [(2, 100, 61, "p2p"), (3, 96, 64, "allgather")])
def test_row_block_apply_one_launch_per_step(world, nx, ny, halo, tmp_path):
    """The same constant-coefficient 5-point cases on the plain tile kernel (HIPK_SPMV_CODED=0): every rank's block resolves to
    hipk_spmv_cheb_kernel<double,1280> and a step is ONE launch, z ping-ponging between two n_ext-long buffers with ghost columns
    gathered from the tail; HIPK_CHEB_FUSED=0 turns the same blocks to two launches.  The same bits."""
    r = _run(world, "hip_apply", {"kind": "poisson", "nx": nx, "ny": ny}, tmp_path,
             env_extra={"HIPK_DIST_HALO": halo, "HIPK_SPMV_CODED": "0"})
    _check_apply(r, lambda fused: ((lambda note: note == TILE_CHEB), TILE_CHEB) if fused == "1" else
                 ((lambda note: note == "hipk_spmv_kernel<double,1280,true>" + STEP), "tile kernel" + STEP))


def _check_solve(r, maxiter=-1):
    keep = json.dumps({k: v for k, v in r.items() if k != "traces"})
    assert r["single_equal"], keep
    assert set(r["info"]) == {r["single_info"]}, keep
    assert set(r["iterations"]) == {r["single_iterations"]}, keep
    assert set(r["residual_norm"]) == {r["single_residual_norm"]}, keep
    assert r["second_equal"] and set(r["second_info"]) == {r["single_second_info"]}, keep
    assert set(r["second_iterations"]) == {r["single_second_iterations"]}, keep
    assert set(r["second_residual_norm"]) == {r["single_second_residual_norm"]}, keep
    assert set(r["preconditioner"]) == {"chebyshev"}, keep
    it = r["single_iterations"]
    assert set(r["applies"]) == {it + 2} and set(r["spmvs"]) == {(it + 2) * r["degree"]}, keep
    assert set(r["matvecs"]) == {it + 2}, keep
    assert set(r["solve_path"]) == {"hipk_dist_chebcg launch sequence"}, keep
    assert all(r["coef_equal_global"]), keep
    if maxiter > 0:
        assert set(r["iterations"]) == {maxiter}, keep
    else:
        assert set(r["info"]) == {0} and it > 3, keep


@pytest.mark.gpu
@pytest.mark.parametrize("world,kind,nx,ny,pmode,halo,entry,maxiter,degree", [
    (2, "vardiff", 100, 61, "local", "p2p", "solver", -1, 3),
    (3, "vardiff", 96, 64, "global", "allgather", "module_a", -1, 3),
    (2, "random_spd", 80, 77, "local", "allgather", "module_a", -1, 3),      # scattered send lists: the pack kernel runs
    (3, "poisson", 96, 64, "global", "p2p", "module_a", -1, 3),
    (2, "vardiff", 100, 61, "local", "p2p", "module_a", 9, 3),
    (2, "vardiff", 100, 61, "global", "allgather", "module_a", -1, 1),
    (3, "vardiff", 96, 64, "local", "p2p", "solver", -1, 4),
])
def test_row_partitioned_chebyshev_cg_shared_gpu(world, kind, nx, ny, pmode, halo, entry, maxiter, degree, tmp_path):
    """Every rank's x concatenates to the single-device cg(A, b, M=ChebyshevPreconditioner(A)), bit for bit; info, iterations and
    the residual norm ||M (b - A x)|| are the same on every rank and those of the single-device solve; a second solve,
    warm-started, on the cached plan and dinv; applies = iterations + 2.  With P built from the row block on the device, the
    single-device preconditioner is given P's lmin and lmax (the global class sums |a_ij| with device atomics, in no fixed
    order), and P's coefficients are checked against ChebyshevPreconditioner of the global matrix on the CPU, bitwise."""
    args = {"kind": kind, "nx": nx, "ny": ny, "pmode": pmode, "entry": entry, "tol": 1e-8, "maxiter": maxiter, "degree": degree}
    r = _run(world, "hip_solve", args, tmp_path, env_extra={"HIPK_DIST_HALO": halo})
    _check_solve(r, maxiter)


@pytest.mark.gpu
@pytest.mark.parametrize("halo,coded", [("p2p", "1"), ("allgather", "0")])
def test_row_partitioned_chebyshev_cg_fused_switch_and_epilogue_kernel(halo, coded, tmp_path):
    """Poisson 100 x 61 at world 2, normalize=False: with HIPK_SPMV_CODED=0 the in-loop steps run hipk_spmv_cheb_kernel<double,1280>,
    one launch each (the note names it on both ranks); on the coded form SpMV + hipk_cheb_step_kernel.  The same solve."""
    args = {"kind": "poisson", "nx": 100, "ny": 61, "pmode": "local", "entry": "module_a", "tol": 1e-8, "maxiter": -1,
            "normalize": False}
    r = _run(2, "hip_solve", args, tmp_path, env_extra={"HIPK_DIST_HALO": halo, "HIPK_SPMV_CODED": coded})
    _check_solve(r)
    # the last SpMV launch of a solve is the final apply's last step
    assert all(n == TILE_CHEB if coded == "0" else n.endswith(STEP) for n in r["notes"]), r["notes"]


def _golden_runs():
    from _cheb_mirror import runs
    return [r for r in runs() if r["case"] in ("cheb_poisson_nx48_ones", "cheb_vardiff_nx48") and r["solver"] == "cg"]


@pytest.mark.gpu
@pytest.mark.parametrize("run", _golden_runs(), ids=lambda r: f"{r['case']}-{r['tag']}")
def test_row_partitioned_chebyshev_cg_reference_fixtures(run, tmp_path):
    """The reference's CG runs with this preconditioner (tests/golden/cheb_*_nx48: 2304 rows, two chunks) at world 2, held as
    tests/test_gpu_chebyshev.py holds the single-device solve: the same info, the same matvec count, x within 1e-8."""
    args = {"golden": run["case"], "tag": run["tag"], "has_x0": run["has_x0"], "pmode": "local", "entry": "module_a",
            "tol": run["kwargs"]["tol"], "maxiter": run["kwargs"].get("maxiter", -1), "degree": run["degree"],
            "normalize": run["normalize"]}
    r = _run(2, "hip_solve", args, tmp_path)
    assert r["single_equal"] and r["second_equal"], {k: v for k, v in r.items() if k != "traces"}
    print(f"{run['case']}-{run['tag']}: info {r['info']} (reference {run['info']}), matvecs {r['matvecs']} (reference "
          f"{run['matvecs']}), |x - x_ref| / |x_ref| = {r['golden_err']:.3e}")
    assert set(r["info"]) == {run["info"]}
    assert set(r["matvecs"]) == {run["matvecs"]}
    assert r["golden_err"] <= 1e-8
    assert all(r["coef_equal_global"]) and set(r["preconditioner"]) == {"chebyshev"}


def _expected_trace(c, world, halo, m):
    """(set-up, one iteration, final) of hipk_dist_chebcg_solve at degree m, from the halo mode and this rank's peer counts."""
    GS, GE = ["group_start"], ["group_end"]
    ag = ["all_gather", c["per"], False]
    H = []
    if halo == "allgather":
        H = [["all_gather", c["slab"], False]]
    else:
        for peer, (ns, nr) in enumerate(zip(c["send_counts"], c["recv_counts"])):
            H += ([["send", ns, peer]] if ns else []) + ([["recv", nr, peer]] if nr else [])
    assert H and world > 1
    alone = [GS] + H + [GE] if halo == "p2p" else H      # a stand-alone halo: the pairs in a group, the slab all-gather alone
    both = [GS] + [ag] + H + [GE]                         # an all-gather of partials and a halo in ONE group
    apply = m * alone                                     # the halo of r, then of z_1 .. z_{m-1}
    setup = alone + [ag, ag] + apply + both               # x | <r,r>, <b,b> | z0 = M r0 | <r,z> + halo of z0
    step = [ag] + both + (m - 1) * alone + both
    final = alone + apply + [ag, ag]                      # x | M (b - A x) | <zr,zr>, <x,x>
    return setup, step, final


@pytest.mark.gpu
@pytest.mark.parametrize("world,halo", [(2, "p2p"), (3, "allgather")])
def test_row_partitioned_chebyshev_cg_collective_schedule(world, halo, tmp_path):
    """Every collective call of hipk_dist_chebcg_solve, in order, on every rank, at degree 1 and 3 and maxiter 3 and 8: set-up +
    k x step + final with step = all-gather <p,Ap> | group(all-gather <r,r> + halo of r) | (m - 1) stand-alone halos |
    group(all-gather <r,z> + halo of z_m) -- m + 2 collective launches and no other halo."""
    args = {"kind": "vardiff", "nx": 96, "ny": 64, "pmode": "local", "entry": "module_a", "tol": 1e-8, "maxiter": -1, "trace": True}
    r = _run(world, "hip_solve", args, tmp_path, env_extra={"HIPK_DIST_HALO": halo})
    _check_solve(r)
    for c in r["traces"]:
        for m in (1, 3):
            setup, step, final = _expected_trace(c, world, halo, m)
            for k in (3, 8):
                assert c["runs"][f"{m}_{k}"] == setup + k * step + final, (m, k, c)
            ends = {k: sum(call == ["group_end"] for call in c["runs"][f"{m}_{k}"]) for k in (3, 8)}
            groups = 2 + (m - 1 if halo == "p2p" else 0)      # stand-alone p2p halos are groups of their own
            assert ends[8] - ends[3] == 5 * groups, (m, ends)
            launches = sum(1 for call in step if call[0] == "group_end") + sum(1 for i, call in enumerate(step) if call[0] == "all_gather"
                                                                                   and not _inside_group(step, i))
            assert launches == m + 2, (m, step)


def _inside_group(calls, i):
    depth = 0
    for call in calls[:i]:
        depth += (call[0] == "group_start") - (call[0] == "group_end")
    return depth > 0


@pytest.mark.gpu
def test_row_partitioned_chebyshev_entry_points_report_errors_at_world_1(tmp_path):
    r = _run(1, "hip_errors", {"nx": 24, "ny": 20, "fail_nth": 5}, tmp_path)
    ARG, HIP, ALIGN, WORKSPACE = -1, -2, -3, -5
    want = {"null": (ARG, "null argument"), "coef": (ARG, "null argument"), "dinv": (ARG, "null argument"),
            "work": (WORKSPACE, "work too small"), "align": (ALIGN, "work must be 256-byte, x / b / dinv 16-byte aligned"),
            "degree0": (ARG, "degree must be in [1, 32]"), "degree33": (ARG, "degree must be in [1, 32]"),
            "rank": (ARG, "rank / world")}
    for name in ("hipk_dist_chebcg_solve", "hipk_dist_cheb_apply"):
        got = r[name]
        assert set(got) == set(want) | ({"nccl"} if name.endswith("solve") else set()), got
        for case, (code, text) in want.items():
            assert got[case][0] == code and got[case][1].endswith(": " + text), (name, case, got[case])
    assert r["hipk_dist_chebcg_solve"]["nccl"] == [HIP, "hipk_dist_chebcg_solve: all_gather(partials) failed (ncclResult 7)"], r


@pytest.mark.gpu
def test_row_partitioned_chebyshev_nccl_world1_equals_single_gpu(tmp_path):
    """Real RCCL at world size 1: the loop through the direct communicator equals the single-device solve."""
    code = r'''
import os, sys, json, torch, torch.distributed as dist
sys.path[:0] = [%r, %r]
import pytorch_sparse_solver as pss
from pytorch_sparse_solver.module_a import ChebyshevPreconditioner, cg, get_last_stats
from pytorch_sparse_solver.utils.matrix_utils import create_variable_diffusion_2d_csr
dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
A = create_variable_diffusion_2d_csr(96, 64, device="cuda:0")
b = torch.randn(96 * 64, dtype=torch.float64, generator=torch.Generator().manual_seed(3)).to("cuda:0")
Arb = pss.RowBlockCSR.from_global_csr(A)
P = ChebyshevPreconditioner.for_row_block(Arb)
x, info = cg(Arb, b, tol=1e-8, M=P)
st = get_last_stats()
z = P(b)
G = ChebyshevPreconditioner(A, lmax=P.lmax, lmin=P.lmin)
xr, info_r = cg(A, b, tol=1e-8, M=G)
sr = get_last_stats()
out = {"equal": bool(torch.equal(x, xr)), "info": [info, info_r], "it": [st.iterations, sr.iterations],
       "res": [st.residual_norm, sr.residual_norm], "pre": st.preconditioner, "comm": Arb._prob.comm_kind,
       "apply_equal": bool(torch.equal(z, G(b))), "applies": P.applies}
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
    assert r["equal"] and r["info"] == [0, 0] and r["it"][0] == r["it"][1] and r["res"][0] == r["res"][1], r
    assert r["pre"] == "chebyshev" and r["apply_equal"] and r["applies"] == r["it"][0] + 3, r


@pytest.mark.gpu
def test_row_partitioned_chebyshev_cg_on_large_row_blocks(tmp_path):
    """One block of realistic size: constant-coefficient Poisson 600 x 1024 (614 400 rows, 300 chunks) over two ranks sharing
    cuda:0, maxiter 5, degree 3, with the grouped walk (HIPK_SPMV_SELL_STRIDED=1): every Chebyshev step inside the loop is one
    launch of hipk_spmv_sell_wide_kernel<5,28,1> on the rectangular block handle with ghost columns -- the kernel a rank of
    BASELINE config 5 runs.  Bitwise the single-device solve."""
    args = {"kind": "poisson_ones", "nx": 600, "ny": 1024, "pmode": "local", "entry": "module_a", "tol": 1e-12, "maxiter": 5}
    r = _run(2, "hip_solve", args, tmp_path, env_extra={"HIPK_SPMV_SELL_STRIDED": "1"}, timeout=600)
    _check_solve(r, 5)
    assert r["notes"] == [WIDE_CHEB, WIDE_CHEB], r["notes"]
    assert r["n_local"] == [307200, 307200]
