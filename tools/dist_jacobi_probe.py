#!/usr/bin/env python3
"""World-size-1 RCCL run of the row-partitioned Jacobi CG against the plain row-partitioned CG and the single-device
cg(..., M=JacobiPreconditioner) on an nx x nx variable-diffusion block: microseconds per iteration from the solves' device
events (DistStats / get_last_stats solve_ms), fixed iteration count (tol = 0).  Run it under `rocprofv3 --kernel-trace --stats`
for the per-kernel split.
usage: python3 tools/dist_jacobi_probe.py [nx=2000] [iterations=400] [which=all|pcg]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pytorch-sparse-linalg-torch-amgx.cg.bicg.gmres_amd")]
os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
os.environ.setdefault("MASTER_PORT", "29541")
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402
import pytorch_sparse_solver as pss  # noqa: E402
from pytorch_sparse_solver.module_a import JacobiPreconditioner, cg, get_last_stats  # noqa: E402
from pytorch_sparse_solver.utils.matrix_utils import create_variable_diffusion_2d_csr  # noqa: E402

nx = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
its = int(sys.argv[2]) if len(sys.argv) > 2 else 400
which = sys.argv[3] if len(sys.argv) > 3 else "all"
dev = torch.device("cuda", 0)
dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
A = create_variable_diffusion_2d_csr(nx, nx, device=dev)
b = torch.randn(nx * nx, dtype=torch.float64, generator=torch.Generator().manual_seed(3)).to(dev)
Arb = pss.RowBlockCSR.from_global_csr(A)
P = JacobiPreconditioner(Arb)
cases = [("row-partitioned Jacobi CG", lambda: cg(Arb, b, tol=0.0, maxiter=its, M=P))]
if which == "all":
    Ps = JacobiPreconditioner(A)
    cases += [("row-partitioned plain CG", lambda: cg(Arb, b, tol=0.0, maxiter=its)),
              ("single-device Jacobi CG", lambda: cg(A, b, tol=0.0, maxiter=its, M=Ps))]
for name, run in cases:
    best = None
    for _ in range(4):   # the first one warms up (plan, communicator, dinv halo)
        run()
        st = get_last_stats()
        us = 1e3 * st.solve_ms / max(st.iterations, 1)
        best = us if best is None or us < best else best
    print(f"{name}: {st.iterations} iterations, best {best:.1f} us per iteration (device events, {nx} x {nx} variable diffusion)",
          flush=True)
print("comm:", Arb._prob.comm_kind)
dist.destroy_process_group()
