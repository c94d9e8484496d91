"""Block-Jacobi batch kernels (cg_batch / bicgstab_batch with a BatchedBlockJacobiPreconditioner, route='kernel':
csrc/hipk_batch_bj.hip) against the system loop (route='loop': one single solve per system with M.system(s) as its callable, the
only path such an M had before the kernels), in one process, alternating.

For every case, block size and S the two routes are timed back to back `--reps` times (wall clock around the whole call, device
synchronised); throughput = sum of the systems' iterations / wall time, reported as min..max over the repeats and as the ratio of
the bests.  The solves run to their natural stop at tol = 1e-8.  The loop's rate does not depend on S (the systems run one after
the other): for S > --loop-cap it is timed on the first --loop-cap systems.  Every row checks that the two routes returned the same
bits.  At S >= --apply-from the device time per system-iteration of the block kernel is printed next to that of the Jacobi batch
kernel (BatchedJacobiPreconditioner) on the same systems: their ratio is what the block apply costs, binv streaming included.

  python tools/bj_batch_probe.py                       # all cases, bs 4 and 32, S in 1 2 4 8 16 64 1024 4096
  python tools/bj_batch_probe.py --solver cg --n 1024 --bs 32 --S 256
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "pytorch-sparse-linalg-torch-amgx.cg.bicg.gmres_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

from batch_probe import _batch, _timed  # noqa: E402


def run_case(solver, n, bs, S, reps, loop_cap, apply_from):
    from pytorch_sparse_solver.module_a import (BatchedBlockJacobiPreconditioner, BatchedCSR, BatchedJacobiPreconditioner, bicgstab_batch,
                                                cg_batch, get_last_stats)
    fn = cg_batch if solver == "cg" else bicgstab_batch
    A, B = _batch(solver, n, S)
    M = BatchedBlockJacobiPreconditioner(A, block_size=bs)
    Sl = min(S, loop_cap)
    Al = A if Sl == S else BatchedCSR(A.crow, A.col, A.values[:Sl])
    Ml = M if Sl == S else BatchedBlockJacobiPreconditioner(Al, block_size=bs, binv=M.binv[:Sl])
    Bl = B[:Sl]
    fn(A, B, tol=1e-8, M=M, route="kernel")            # warm-up: code objects, allocator
    A1 = BatchedCSR(A.crow, A.col, A.values[:1])
    fn(A1, B[:1], tol=1e-8, M=BatchedBlockJacobiPreconditioner(A1, block_size=bs, binv=M.binv[:1]), route="loop")
    rk, rl, dev_ms = [], [], []
    for _ in range(reps):
        (Xk, ik), tk = _timed(lambda: fn(A, B, tol=1e-8, M=M, route="kernel"))
        sk = get_last_stats()
        (Xl, il), tl = _timed(lambda: fn(Al, Bl, tol=1e-8, M=Ml, route="loop"))
        sl = get_last_stats()
        assert torch.equal(Xk[:Sl], Xl) and torch.equal(ik[:Sl], il) and sk.iterations[:Sl] == sl.iterations, "the routes disagree"
        rk.append(sum(sk.iterations) / tk)
        rl.append(sum(sl.iterations) / tl)
        dev_ms.append(sk.solve_ms)
    row = {"solver": solver, "n": n, "bs": bs, "S": S, "loop_systems": Sl, "iterations_min_max": [min(sk.iterations), max(sk.iterations)],
           "path": sk.path, "kernel_sysit_per_s": [round(min(rk)), round(max(rk))], "loop_sysit_per_s": [round(min(rl)), round(max(rl))],
           "kernel_over_loop_best": round(max(rk) / max(rl), 2), "kernel_device_ms_best": round(min(dev_ms), 3)}
    if S >= apply_from:
        J = BatchedJacobiPreconditioner(A)
        fn(A, B, tol=1e-8, M=J, route="kernel")
        jac = []
        for _ in range(reps):
            fn(A, B, tol=1e-8, M=J, route="kernel")
            sj = get_last_stats()
            jac.append(sj.solve_ms * 1e3 / max(sum(sj.iterations), 1))
        blk = min(dev_ms) * 1e3 / max(sum(sk.iterations), 1)
        row.update({"block_us_per_system_iteration": round(blk, 3), "jacobi_us_per_system_iteration": round(min(jac), 3),
                    "jacobi_path": sj.path, "block_over_jacobi": round(blk / min(jac), 2)})
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--solver", nargs="*", default=["cg", "bicgstab"])
    ap.add_argument("--n", nargs="*", type=int, default=[256, 1024, 4096])
    ap.add_argument("--bs", nargs="*", type=int, default=[4, 32])
    ap.add_argument("--S", nargs="*", type=int, default=[1, 2, 4, 8, 16, 64, 1024, 4096])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--loop-cap", type=int, default=16)
    ap.add_argument("--apply-from", type=int, default=1024)
    args = ap.parse_args()
    from pytorch_sparse_solver import _hipk
    print(json.dumps({"hipk_build_id": _hipk.lib().hipk_build_id().decode(), "device": torch.cuda.get_device_name(0), "reps": args.reps,
                      "loop_cap": args.loop_cap, "tol": 1e-8, "dtype": "float64"}), flush=True)
    for solver in args.solver:
        for n in args.n:
            for bs in args.bs:
                for S in args.S:
                    print(json.dumps(run_case(solver, n, bs, S, args.reps, args.loop_cap, args.apply_from)), flush=True)


if __name__ == "__main__":
    main()
