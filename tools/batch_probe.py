"""Batch kernels (cg_batch / bicgstab_batch, route='kernel': csrc/hipk_batch.hip) against the system loop (route='loop': one public
single solve per system, the code path that existed before the batch kernels), in one process, alternating.

For every case and S the two routes are timed back to back `--reps` times (wall clock around the whole call, device synchronised);
throughput = sum of the systems' iterations / wall time, reported as best and as min..max over the repeats.  The solves run to
their natural stop at tol = 1e-8, so the systems of a batch stop at different iterations as they do for a user.  The loop's rate
does not depend on S (the systems run one after the other): for S > --loop-cap it is timed on the first --loop-cap systems.
Every row checks that the two routes returned the same bits.  At S = 1 the kernel's device time per iteration is printed next to
the single solve's (its one-launch loop).

  python tools/batch_probe.py                       # all cases, S in 1 8 64 256 1024 4096
  python tools/batch_probe.py --solver cg --n 1024 --S 256
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "pytorch-sparse-linalg-torch-amgx.cg.bicg.gmres_amd"))

import torch  # noqa: E402

DEV = "cuda:0"
GRIDS = {256: (16, 16), 1024: (32, 32), 4096: (64, 64)}
VARDIFF = ((0.5, 0), (1.0, 1), (1.5, 2), (2.0, 3))
CONVDIFF = ((0.5, 0.25), (0.2, 0.1), (0.8, 0.4), (0.3, 0.15))


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def _batch(solver, n, S):
    from pytorch_sparse_solver.module_a import BatchedCSR
    from pytorch_sparse_solver.utils import matrix_utils as mu
    nx, ny = GRIDS[n]
    if solver == "cg":
        four = [mu.create_variable_diffusion_2d_csr(nx, ny, contrast=c, seed=s) for c, s in VARDIFF]
    else:
        four = [mu.create_convdiff_2d_csr(nx, ny, g, d) for g, d in CONVDIFF]
    vals = torch.stack([four[s % 4].values() for s in range(S)]).to(DEV)
    A = BatchedCSR(four[0].crow_indices().to(DEV), four[0].col_indices().to(DEV), vals)
    B = torch.randn((S, n), dtype=torch.float64, generator=torch.Generator().manual_seed(S + n)).to(DEV)
    return A, B


def run_case(solver, n, S, reps, loop_cap):
    from pytorch_sparse_solver.module_a import BatchedCSR, bicgstab_batch, cg_batch, get_last_stats
    fn = cg_batch if solver == "cg" else bicgstab_batch
    A, B = _batch(solver, n, S)
    Sl = min(S, loop_cap)
    Al = A if Sl == S else BatchedCSR(A.crow, A.col, A.values[:Sl])
    Bl = B[:Sl]
    fn(A, B, tol=1e-8, route="kernel")            # warm-up: code objects, allocator
    fn(BatchedCSR(A.crow, A.col, A.values[:1]), B[:1], tol=1e-8, route="loop")
    rk, rl, dev_ms = [], [], []
    for _ in range(reps):
        (Xk, ik), tk = _timed(lambda: fn(A, B, tol=1e-8, route="kernel"))
        sk = get_last_stats()
        (Xl, il), tl = _timed(lambda: fn(Al, Bl, tol=1e-8, route="loop"))
        sl = get_last_stats()
        assert torch.equal(Xk[:Sl], Xl) and torch.equal(ik[:Sl], il) and sk.iterations[:Sl] == sl.iterations, "the routes disagree"
        rk.append(sum(sk.iterations) / tk)
        rl.append(sum(sl.iterations) / tl)
        dev_ms.append(sk.solve_ms)
    row = {"solver": solver, "n": n, "S": S, "loop_systems": Sl, "iterations_min_max": [min(sk.iterations), max(sk.iterations)],
           "path": sk.path, "kernel_sysit_per_s": [round(min(rk)), round(max(rk))], "loop_sysit_per_s": [round(min(rl)), round(max(rl))],
           "kernel_over_loop_best": round(max(rk) / max(rl), 2), "kernel_device_ms_best": round(min(dev_ms), 3)}
    if S == 1:
        single = __import__("pytorch_sparse_solver.module_a", fromlist=["cg"])
        one = single.cg if solver == "cg" else single.bicgstab
        best = None
        for _ in range(reps):
            one(A.system(0), B[0].clone(), tol=1e-8)
            st = get_last_stats()
            us = st.solve_ms * 1e3 / max(st.iterations, 1)
            best = us if best is None else min(best, us)
        from pytorch_sparse_solver import _hipk
        row["kernel_us_per_iteration"] = round(min(dev_ms) * 1e3 / max(sk.iterations[0], 1), 2)
        row["single_solve_us_per_iteration"] = round(best, 2)
        row["single_solve_path"] = _hipk.last_solve_path()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--solver", nargs="*", default=["cg", "bicgstab"])
    ap.add_argument("--n", nargs="*", type=int, default=[256, 1024, 4096])
    ap.add_argument("--S", nargs="*", type=int, default=[1, 8, 64, 256, 1024, 4096])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--loop-cap", type=int, default=64)
    args = ap.parse_args()
    from pytorch_sparse_solver import _hipk
    print(json.dumps({"hipk_build_id": _hipk.lib().hipk_build_id().decode(), "device": torch.cuda.get_device_name(0), "reps": args.reps,
                      "loop_cap": args.loop_cap, "tol": 1e-8, "dtype": "float64"}), flush=True)
    for solver in args.solver:
        for n in args.n:
            for S in args.S:
                print(json.dumps(run_case(solver, n, S, args.reps, args.loop_cap)), flush=True)


if __name__ == "__main__":
    main()
