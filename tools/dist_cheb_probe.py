#!/usr/bin/env python3
"""World-size-1 RCCL run of the row-partitioned Chebyshev CG against the three figures it is judged by, on one build and in one
process: the single-device cg(A, b, M=ChebyshevPreconditioner(A)) (the baseline), the single-device plain cg, the row-partitioned
plain cg -- microseconds per iteration from the solves' device events (DistStats / get_last_stats solve_ms), fixed iteration
count (tol = 0), on the nx x nx variable-diffusion matrix and the nx x nx Poisson matrix.  The four cases are run in rounds (all
four, four times over; the first round warms up plan, communicator and dinv halo), best and median of the timed rounds.
With `trace` as the third argument it runs the single-device and the row-partitioned Chebyshev CG only, once warm and once timed:
the run to put under `rocprofv3 --kernel-trace --stats` for the per-kernel split -- hipk_cg_update_kernel and
hipk_cheb_init_kernel of the first against hipk_cheb_update_kernel of the second.
usage: python3 tools/dist_cheb_probe.py [nx=2000] [iterations=300] [all|trace] [degree=3]"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pytorch-sparse-linalg-torch-amgx.cg.bicg.gmres_amd")]
os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
os.environ.setdefault("MASTER_PORT", "29543")
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402
import pytorch_sparse_solver as pss  # noqa: E402
from pytorch_sparse_solver import _hipk  # noqa: E402
from pytorch_sparse_solver.module_a import ChebyshevPreconditioner, cg, get_last_stats  # noqa: E402
from pytorch_sparse_solver.utils.matrix_utils import create_poisson_2d_csr, create_variable_diffusion_2d_csr  # noqa: E402

nx = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
its = int(sys.argv[2]) if len(sys.argv) > 2 else 300
which = sys.argv[3] if len(sys.argv) > 3 else "all"
degree = int(sys.argv[4]) if len(sys.argv) > 4 else 3
dev = torch.device("cuda", 0)
dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
print(f"build {_hipk.lib().hipk_build_id().decode()}, {nx} x {nx}, {its} iterations per solve, degree {degree}", flush=True)
for kind, make in (("variable diffusion", create_variable_diffusion_2d_csr), ("Poisson", create_poisson_2d_csr)):
    A = make(nx, nx).to(dev)
    b = torch.randn(nx * nx, dtype=torch.float64, generator=torch.Generator().manual_seed(3)).to(dev)
    Arb = pss.RowBlockCSR.from_global_csr(A)
    P = ChebyshevPreconditioner.for_row_block(Arb, degree=degree)
    Ps = ChebyshevPreconditioner(A, degree=degree, lmax=P.lmax, lmin=P.lmin)
    cases = [("single-device Chebyshev CG", lambda: cg(A, b, tol=0.0, maxiter=its, M=Ps)),
             ("row-partitioned Chebyshev CG", lambda: cg(Arb, b, tol=0.0, maxiter=its, M=P))]
    if which == "all":
        cases += [("single-device plain CG", lambda: cg(A, b, tol=0.0, maxiter=its)),
                  ("row-partitioned plain CG", lambda: cg(Arb, b, tol=0.0, maxiter=its))]
    us = {name: [] for name, _ in cases}
    notes = {}
    for rnd in range(2 if which == "trace" else 5):
        for name, run in cases:
            x, _ = run()
            st = get_last_stats()
            assert st.iterations == its, (name, st.iterations)
            notes[name] = _hipk.CsrHandle.last_spmv_kernel()
            if rnd:
                us[name].append(1e3 * st.solve_ms / its)
    for name, _ in cases:
        print(f"{kind}: {name}: best {min(us[name]):.1f}, median {statistics.median(us[name]):.1f} us per iteration "
              f"(last SpMV launch: {notes[name]})", flush=True)
    if which == "all":
        xs, _ = cg(A, b, tol=0.0, maxiter=its, M=Ps)
        xr, _ = cg(Arb, b, tol=0.0, maxiter=its, M=P)
        print(f"{kind}: row-partitioned == single-device Chebyshev CG bitwise: {bool(torch.equal(xs, xr))}", flush=True)
    print(f"{kind}: comm {Arb._prob.comm_kind}", flush=True)
    del A, Arb, P, Ps
    _hipk.clear_cache()
dist.destroy_process_group()
