"""Block solves (multi_rhs._block_solve: hipk_{cg,bicgstab}_solve_multi) against the column loop (`cg(A, B[:, j])` for every j), in one process, alternating.

For every case and k the two are timed back to back `--reps` times (wall clock around the whole call, device synchronised) and the
best of each is kept; throughput = sum of the columns' iterations / wall time.  Every column of the block result is checked to be
bitwise equal to the column loop's.  tol is set so low that no column converges: each runs `--maxiter` iterations.

  python tools/multi_rhs_probe.py                          # all cases, k in 1 2 4 8 16
  python tools/multi_rhs_probe.py --case general4m --k 8   # one case (e.g. under rocprofv3 --kernel-trace --stats)

Cases: general4m (2000^2 Poisson, coded form off), vardiff4m (variable-coefficient 2000^2), coded4m (2000^2 Poisson, coded form
on: what the column loop streams is 67 MB of codes instead of 256 MB of CSR), n40k (200^2), n250k (500^2).
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
CASES = {  # name: (grid, matrix, plain CSR only, maxiter)
    "general4m": (2000, "poisson", True, 60),
    "vardiff4m": (2000, "vardiff", True, 60),
    "coded4m": (2000, "poisson", False, 60),
    "n40k": (200, "poisson", False, 400),
    "n250k": (500, "poisson", False, 300),
}


def _matrix(kind, nx):
    from pytorch_sparse_solver.utils import matrix_utils as mu
    if kind == "poisson":
        return mu.create_poisson_2d_csr(nx, nx, device=DEV)
    return mu.create_variable_diffusion_2d_csr(nx, nx, device=DEV).to(DEV)


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def run_case(name, ks, reps, solver):
    from pytorch_sparse_solver import _hipk
    from pytorch_sparse_solver.module_a import bicgstab, cg, get_last_stats
    from pytorch_sparse_solver.module_a.multi_rhs import _block_solve
    single = cg if solver == "cg" else bicgstab

    def multi(A, B, tol, maxiter):
        return _block_solve(solver, A, B, None, tol, 0.0, maxiter, None)
    nx, kind, plain, maxiter = CASES[name]
    A = _matrix(kind, nx)
    h = _hipk.handle_for(A)
    if plain:
        h.set_path(True)
    n = nx * nx
    rows = []
    for k in ks:
        B = torch.randn(n, k, dtype=torch.float64, device=DEV, generator=torch.Generator(device=DEV).manual_seed(k))
        kw = dict(tol=1e-30, maxiter=maxiter)
        multi(A, B, **kw)   # warm-up: handle, workspace, code objects
        best_b = best_c = float("inf")
        for _ in range(reps):
            (Xb, _), tb = _timed(lambda: multi(A, B, **kw))
            stb = get_last_stats()
            path = _hipk.last_solve_path()

            def loop():
                return [single(A, B[:, j], **kw)[0] for j in range(k)]
            xs, tc = _timed(loop)
            best_b, best_c = min(best_b, tb), min(best_c, tc)
        its = sum(c.iterations for c in stb.columns)
        equal = all(torch.equal(Xb[:, j], xs[j]) for j in range(k))
        row = dict(case=name, solver=solver, n=n, k=k, spmv_path=h.path(), block_path=path, iterations=its,
                   block_spmvs=stb.block_spmvs, block_ms=round(best_b * 1e3, 3), loop_ms=round(best_c * 1e3, 3),
                   block_kits=round(its / best_b / 1e3, 2), loop_kits=round(its / best_c / 1e3, 2),
                   speedup=round(best_c / best_b, 3), bitwise_equal=equal)
        print(json.dumps(row), flush=True)
        rows.append(row)
        del B, Xb, xs
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=sorted(CASES), action="append")
    ap.add_argument("--k", type=int, action="append")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--solver", choices=["cg", "bicgstab"], default="cg")
    ap.add_argument("--out", default=None, help="also write the rows as a JSON list here")
    a = ap.parse_args()
    cases = a.case or ["n40k", "n250k", "general4m", "vardiff4m", "coded4m"]
    ks = a.k or [1, 2, 4, 8, 16]
    rows = []
    for c in cases:
        rows += run_case(c, ks, a.reps, a.solver)
    print(f"{'case':>10} {'k':>3} {'block kit/s':>12} {'loop kit/s':>11} {'speedup':>8} bitwise")
    for r in rows:
        print(f"{r['case']:>10} {r['k']:>3} {r['block_kits']:>12} {r['loop_kits']:>11} {r['speedup']:>8} {r['bitwise_equal']}")
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)
    if not all(r["bitwise_equal"] for r in rows):
        sys.exit(1)


if __name__ == "__main__":
    main()
