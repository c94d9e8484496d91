"""cg(tol=1e-6) with and without the Chebyshev preconditioner on the 5-point Poisson matrix, in one process: plain CG, then
`ChebyshevPreconditioner(A, degree)` for every degree with one launch per Chebyshev step (the SpMV kernels' epilogue) and with two
(HIPK_CHEB_FUSED=0: SpMV + hipk_cheb_step_kernel).  Prints, per row: iterations, info, operator applications
((degree + 1) x iterations for the preconditioned solves), best wall time of `--reps` solves (device synchronised), the time of
one Chebyshev step measured on stand-alone applies (HIP events around `--applies` applies, divided by applies x degree: it
includes a share of the step-0 kernel), and the SpMV kernel the steps ran.

  python tools/cheb_probe.py                                  # N = 4 M (headline), 16 M, 64 M; degrees 1 2 3 5 7
  python tools/cheb_probe.py --sizes 2000 --degrees 3 --reps 1    # one case, e.g. under rocprofv3 --kernel-trace --stats -- python ...
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


def _timed(fn, reps):
    best, out = None, None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return out, best * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[2000, 4000, 8000], help="grid sizes nx (N = nx^2)")
    ap.add_argument("--degrees", type=int, nargs="+", default=[1, 2, 3, 5, 7])
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--applies", type=int, default=10)
    ap.add_argument("--tol", type=float, default=1e-6)
    ap.add_argument("--no-plain", action="store_true", help="skip the unpreconditioned solve")
    args = ap.parse_args()
    from pytorch_sparse_solver import _hipk
    from pytorch_sparse_solver.module_a import ChebyshevPreconditioner, cg, get_last_stats
    from pytorch_sparse_solver.utils.matrix_utils import create_poisson_2d_csr
    print(f"# build {_hipk.lib().hipk_build_id().decode()}  device {torch.cuda.get_device_name(0)}  tol {args.tol}")
    for nx in args.sizes:
        A = create_poisson_2d_csr(nx, nx, device=DEV)
        n = nx * nx
        b = torch.ones(n, dtype=torch.float64, device=DEV)
        cg(A, b, tol=args.tol, maxiter=5)                          # handle creation, first-launch costs
        rows = []
        base_ms = None
        if not args.no_plain:
            (_, info), ms = _timed(lambda: cg(A, b, tol=args.tol), args.reps)
            st = get_last_stats()
            base_ms = ms
            rows.append(dict(n=n, precond="none", form="-", iterations=st.iterations, info=info, applications=st.matvecs, solve_ms=ms,
                             step_ms=None, kernel=_hipk.CsrHandle.last_spmv_kernel()))
            print(f"N = {n:>9}  plain cg            {st.iterations:6d} its  info {info:2d}  {st.matvecs:6d} applications  {ms:10.2f} ms")
        for m in args.degrees:
            for fused in ("1", "0"):
                os.environ["HIPK_CHEB_FUSED"] = fused
                M = ChebyshevPreconditioner(A, degree=m)
                z = M(b)                                           # warm-up apply; names the kernel the steps run
                kernel = _hipk.CsrHandle.last_spmv_kernel()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(args.applies):
                    z = M(b)
                e1.record()
                torch.cuda.synchronize()
                step_ms = e0.elapsed_time(e1) / (args.applies * m)
                del z
                (x, info), ms = _timed(lambda: cg(A, b, tol=args.tol, M=M), args.reps)
                st = get_last_stats()
                y = _hipk.spmv(_hipk.handle_for(A), x)
                relres = float(torch.linalg.vector_norm(b - y) / torch.linalg.vector_norm(b))
                apps = (m + 1) * st.iterations
                form = "one launch" if fused == "1" and "hipk_cheb_step_kernel" not in kernel else "two launches"
                rows.append(dict(n=n, precond=f"chebyshev({m})", form=form, iterations=st.iterations, info=info, applications=apps,
                                 solve_ms=ms, step_ms=step_ms, relres=relres, kernel=kernel))
                rel = f"  x{ms / base_ms:5.2f} of plain" if base_ms else ""
                print(f"N = {n:>9}  chebyshev({m}) {form:12s} {st.iterations:6d} its  info {info:2d}  {apps:6d} applications  {ms:10.2f} ms{rel}"
                      f"  step {step_ms * 1e3:8.1f} us  relres {relres:.2e}  [{kernel}]")
                del x, y, M
        os.environ.pop("HIPK_CHEB_FUSED", None)
        print(json.dumps({"cheb_probe": rows}))
        del A, b
        _hipk.clear_cache()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
