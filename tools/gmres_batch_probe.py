"""The GMRES batch kernel (gmres_batch, route='kernel': csrc/hipk_batch_gm.hip) against the system loop (route='loop': one public
`gmres` per system, the code path that existed before the kernel), in one process, alternating.

For every n and S the two routes are timed back to back `--reps` times (wall clock around the whole call, device synchronised);
throughput = sum of the systems' Arnoldi steps (operator applications inside the cycles) / wall time, reported as best and as
min..max over the repeats.  The solves run to their natural stop at tol = 1e-8 with restart 20, so the systems of a batch end at
different cycles as they do for a user.  The loop's rate does not depend on S (the systems run one after the other): for
S > --loop-cap it is timed on the first --loop-cap systems.  Every row checks that the two routes returned the same bits.  At S = 1
the kernel's device time per Arnoldi step is printed next to the single solve's.

  python tools/gmres_batch_probe.py                       # n in 256 1024 4096, S in 1 2 4 8 64 256 1024 4096
  python tools/gmres_batch_probe.py --n 1024 --S 256 --method incremental
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
CONVDIFF = ((0.5, 0.25), (0.2, 0.1), (0.8, 0.4), (0.3, 0.15))


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def _batch(n, S):
    from pytorch_sparse_solver.module_a import BatchedCSR
    from pytorch_sparse_solver.utils import matrix_utils as mu
    nx, ny = GRIDS[n]
    four = [mu.create_convdiff_2d_csr(nx, ny, g, d) for g, d in CONVDIFF]
    vals = torch.stack([four[s % 4].values() for s in range(S)]).to(DEV)
    A = BatchedCSR(four[0].crow_indices().to(DEV), four[0].col_indices().to(DEV), vals)
    B = torch.randn((S, n), dtype=torch.float64, generator=torch.Generator().manual_seed(S + n)).to(DEV)
    return A, B


def _steps(st):
    """Arnoldi steps per system: the operator applications that are not a residual (one at the start, one per cycle, one at the end)."""
    return [m - 2 - c for m, c in zip(st.matvecs, st.iterations)]


def run_case(n, S, reps, loop_cap, restart, method):
    from pytorch_sparse_solver.module_a import BatchedCSR, get_last_stats, gmres, gmres_batch
    kw = dict(tol=1e-8, restart=restart, solve_method=method)
    A, B = _batch(n, S)
    Sl = min(S, loop_cap)
    Al = A if Sl == S else BatchedCSR(A.crow, A.col, A.values[:Sl])
    Bl = B[:Sl]
    gmres_batch(A, B, route="kernel", **kw)            # warm-up: code objects, allocator
    gmres_batch(BatchedCSR(A.crow, A.col, A.values[:1]), B[:1], route="loop", **kw)
    rk, rl, dev_ms = [], [], []
    for _ in range(reps):
        (Xk, ik), tk = _timed(lambda: gmres_batch(A, B, route="kernel", **kw))
        sk = get_last_stats()
        (Xl, il), tl = _timed(lambda: gmres_batch(Al, Bl, route="loop", **kw))
        sl = get_last_stats()
        assert torch.equal(Xk[:Sl], Xl) and torch.equal(ik[:Sl], il) and sk.matvecs[:Sl] == sl.matvecs, "the routes disagree"
        rk.append(sum(_steps(sk)) / tk)
        rl.append(sum(_steps(sl)) / tl)
        dev_ms.append(sk.solve_ms)
    row = {"n": n, "S": S, "restart": restart, "method": method, "loop_systems": Sl, "cycles_min_max": [min(sk.iterations), max(sk.iterations)],
           "steps_min_max": [min(_steps(sk)), max(_steps(sk))], "path": sk.path,
           "kernel_syssteps_per_s": [round(min(rk)), round(max(rk))], "loop_syssteps_per_s": [round(min(rl)), round(max(rl))],
           "kernel_over_loop_best": round(max(rk) / max(rl), 2), "kernel_device_ms_best": round(min(dev_ms), 3)}
    if S == 1:
        best = None
        for _ in range(reps):
            gmres(A.system(0), B[0].clone(), **kw)
            st = get_last_stats()
            us = st.solve_ms * 1e3 / max(st.matvecs - 2 - st.iterations, 1)
            best = us if best is None else min(best, us)
        from pytorch_sparse_solver import _hipk
        row["kernel_us_per_step"] = round(min(dev_ms) * 1e3 / max(_steps(sk)[0], 1), 2)
        row["single_solve_us_per_step"] = round(best, 2)
        row["single_solve_path"] = _hipk.last_solve_path()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", nargs="*", type=int, default=[256, 1024, 4096])
    ap.add_argument("--S", nargs="*", type=int, default=[1, 2, 4, 8, 64, 256, 1024, 4096])
    ap.add_argument("--restart", type=int, default=20)
    ap.add_argument("--method", default="batched", choices=["batched", "incremental"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--loop-cap", type=int, default=32)
    args = ap.parse_args()
    from pytorch_sparse_solver import _hipk
    print(json.dumps({"hipk_build_id": _hipk.lib().hipk_build_id().decode(), "device": torch.cuda.get_device_name(0), "reps": args.reps,
                      "loop_cap": args.loop_cap, "tol": 1e-8, "dtype": "float64"}), flush=True)
    for n in args.n:
        for S in args.S:
            print(json.dumps(run_case(n, S, args.reps, args.loop_cap, args.restart, args.method)), flush=True)


if __name__ == "__main__":
    main()
