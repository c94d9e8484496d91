#!/usr/bin/env python3
"""World-size-1 RCCL run of the row-partitioned GMRES -- the restart <= 31 loop (hipk_dist_gmres_solve) and the restart 32 .. 255
loop (hipk_dist_gmres_wide_solve) -- against the single-device gmres on an nx x nx convection-diffusion block: milliseconds per
restart cycle from the solves' device events (DistStats / get_last_stats solve_ms), fixed cycle count (tol = 0, batched).  Run it
under `rocprofv3 --kernel-trace --stats` for the per-kernel split.
usage: python3 tools/dist_gmres_probe.py [nx=2000] [cycles=2] [restarts=30,31,32,64,128] [which=all|dist]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pytorch-sparse-linalg-torch-amgx.cg.bicg.gmres_amd")]
os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
os.environ.setdefault("MASTER_PORT", "29543")
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402
import pytorch_sparse_solver as pss  # noqa: E402
from pytorch_sparse_solver import _hipk  # noqa: E402
from pytorch_sparse_solver.module_a import get_last_stats, gmres  # noqa: E402
from pytorch_sparse_solver.utils.matrix_utils import create_convdiff_2d_csr  # noqa: E402

nx = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
cycles = int(sys.argv[2]) if len(sys.argv) > 2 else 2
restarts = [int(v) for v in sys.argv[3].split(",")] if len(sys.argv) > 3 else [30, 31, 32, 64, 128]
which = sys.argv[4] if len(sys.argv) > 4 else "all"
dev = torch.device("cuda", 0)
dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
A = create_convdiff_2d_csr(nx, nx, device=dev)
b = torch.randn(nx * nx, dtype=torch.float64, generator=torch.Generator().manual_seed(3)).to(dev)
Arb = pss.RowBlockCSR.from_global_csr(A)
print(f"build {_hipk.lib().hipk_build_id().decode()}, {nx} x {nx} convection-diffusion ({nx * nx} rows), {cycles} cycles, "
      f"batched, device events", flush=True)
for m in restarts:
    loop = "hipk_dist_gmres_wide_solve" if m > 31 else "hipk_dist_gmres_solve"
    cases = [(f"row-partitioned ({loop})", lambda m=m: gmres(Arb, b, tol=0.0, restart=m, maxiter=cycles))]
    if which == "all":
        cases.append(("single-device gmres", lambda m=m: gmres(A, b, tol=0.0, restart=m, maxiter=cycles)))
    for name, run in cases:
        best = None
        for _ in range(3):   # the first one warms up (plan, communicator, workspace)
            run()
            st = get_last_stats()
            ms = st.solve_ms / max(st.iterations, 1)
            best = ms if best is None or ms < best else best
        print(f"restart {m:3d}  {name}: {st.iterations} cycles, {st.matvecs} matvecs, best {best:.2f} ms per cycle", flush=True)
print("comm:", Arb._prob.comm_kind)
dist.destroy_process_group()
