"""Worker of tests/test_dist_jacobi.py: one rank of the row-partitioned solvers with M = JacobiPreconditioner, reached through the
reference's call surface with a `RowBlockCSR` operand.  cpu tasks: gloo + the CPU ops double (the preconditioner's set-up and its
errors); hip tasks: several ranks share cuda:0, the C-driven Jacobi loops run with host-staged stand-ins for the collectives (or
the device mailboxes) -- tests/_dist_worker.py."""
import ctypes
import json
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pytorch-sparse-linalg-torch-amgx.cg.bicg.gmres_amd"), os.path.join(ROOT, "tests")]

from _dist_worker import HostStagedNative, MailboxNative, build_global  # noqa: E402
from dist_cpu_ops import OracleOps  # noqa: E402
from oracle import oracle as O  # noqa: E402
import pytorch_sparse_solver as pss  # noqa: E402
from pytorch_sparse_solver import SparseSolver, _hipk  # noqa: E402
from pytorch_sparse_solver import module_a  # noqa: E402
from pytorch_sparse_solver.module_a import BlockJacobiPreconditioner, JacobiPreconditioner  # noqa: E402
from pytorch_sparse_solver.utils.matrix_utils import create_variable_diffusion_2d_csr  # noqa: E402


def global_system(kind, nx, ny):
    if kind == "vardiff":
        A = create_variable_diffusion_2d_csr(nx, ny)
        b = torch.randn(nx * ny, dtype=torch.float64, generator=torch.Generator().manual_seed(11))
        return A, b
    return build_global(kind, nx, ny)


def _from_block(self, crow, col_global, val, b_local, part, ops):
    """DistProblem set-up for ranks sharing cuda:0: the halo plan's collectives on CPU tensors (gloo), matrix and vectors on the GPU."""
    from pytorch_sparse_solver.distributed import HaloPlan
    dev = ops.device
    plan = HaloPlan(col_global.cpu(), part)
    for name in ("col_local", "send_idx", "ghost_src"):
        setattr(plan, name, getattr(plan, name).to(dev))
    self.part, self.ops, self.group, self.plan = part, ops, None, plan
    self.n_local, self.n_ext, self.nnz_local = part.n_local, part.n_local + plan.n_ghost, int(val.numel())
    self.b = b_local.to(dev)
    self.A = ops.make_matrix(crow.to(dev), plan.col_local, val.to(dev), part.n_local, max(self.n_ext, 1), part.ch)
    self.spmv_bytes = 0
    self.send_buf = ops.empty(max(plan.n_send, 1))
    self.slab_loc, self.slab_all = ops.zeros(plan.slab), ops.zeros(plan.slab * part.world)
    self.comm, self.p2p, self.comm_kind = None, None, "host-staged (test)"


class StagedCounting(HostStagedNative):
    """Host-staged collectives; counts the group_end calls the C-driven loop makes."""

    def __init__(self, crow, col_global, val, b_local, part, ops, group=None):
        _from_block(self, crow, col_global, val, b_local, part, ops)
        self.group_ends = 0

    def coll_struct(self):
        if getattr(self, "_counted", None) is None:
            coll = super().coll_struct()
            inner = self._cbs[1]

            def group_end():
                self.group_ends += 1
                return inner()
            self._counted = _hipk.COLL_GROUP_FN(group_end)
            coll.group_end = ctypes.cast(self._counted, ctypes.c_void_p).value
        return self._coll


class FusedMailbox(MailboxNative):
    """The device mailboxes with the fused area (HIPK_DIST_COMM=fused): the plain CG folds its exchanges into its kernels."""

    def __init__(self, crow, col_global, val, b_local, part, ops, group=None):
        from pytorch_sparse_solver.distributed import P2PComm
        _from_block(self, crow, col_global, val, b_local, part, ops)
        self.p2p = P2PComm(part.rank, part.world, ops.device, max(part.per, self.plan.slab), fx_per=part.per,
                           fx_ghost_cap=self.plan.ghost_cap)


def cpu_task(task, a, rank, world):
    A, b = global_system(a["kind"], a["nx"], a["ny"])
    n = A.shape[0]
    r0, r1 = pss.RowBlockCSR.row_range(n)
    res = {}
    if task == "zero":                 # a zero on the diagonal of the LAST rank's rows only
        crow, col, val = A.crow_indices(), A.col_indices(), A.values().clone()
        i = n - 3
        j = int(crow[i]) + int((col[int(crow[i]):int(crow[i + 1])] == i).nonzero()[0])
        val[j] = 0.0
        A = torch.sparse_csr_tensor(crow, col, val, A.shape)
    Arb = pss.RowBlockCSR.from_global_csr(A, ops=OracleOps())
    if task == "dinv":
        P = JacobiPreconditioner(Arb)
        Pg = JacobiPreconditioner(A)
        res = {"equal": bool(torch.equal(P.dinv, Pg.dinv[r0:r1])), "shape": list(P.shape), "rows": list(P.row_range),
               "n": int(P.dinv.numel())}
    elif task == "zero":
        try:
            JacobiPreconditioner(Arb)
            res = {"raised": ""}
        except ValueError as e:
            res = {"raised": str(e)}
    elif task == "errors":
        b_loc = b[r0:r1].clone()
        out = {}
        for name, M in (("callable", lambda v: v), ("block", BlockJacobiPreconditioner(A, 4)), ("matrix", A),
                        ("wrong_size", JacobiPreconditioner(create_variable_diffusion_2d_csr(4, 5)))):
            try:
                module_a.cg(Arb, b_loc, M=M)
                out[name] = "no error"
            except ValueError as e:
                out[name] = "ValueError: " + str(e)
        for method in ("cg", "bicgstab", "gmres"):
            try:
                getattr(module_a, method)(Arb, b_loc, M=JacobiPreconditioner(A))
                out["cpu_" + method] = "no error"
            except RuntimeError as e:
                out["cpu_" + method] = "RuntimeError: " + str(e)
        res = out
    return res


def hip_task(a, rank, world):
    kind, nx, ny, solver, tol, maxiter = a["kind"], a["nx"], a["ny"], a["solver"], a["tol"], a["maxiter"]
    A, b = global_system(kind, nx, ny)
    n = A.shape[0]
    r0, r1 = pss.RowBlockCSR.row_range(n)
    dev = torch.device("cuda", 0)
    from pytorch_sparse_solver.distributed import HipOps, dist_cg
    cls = FusedMailbox if a.get("comm") == "fused" else StagedCounting
    Arb = pss.RowBlockCSR.from_global_csr(A.to(dev), ops=HipOps(dev), problem_cls=cls)
    b_loc = b[r0:r1].to(dev)
    P = JacobiPreconditioner(Arb) if a["pmode"] == "local" else JacobiPreconditioner(A.to(dev))
    method = "gmres" if solver.startswith("gmres") else solver
    kw = {"tol": tol}
    if maxiter >= 0:
        kw["maxiter"] = maxiter
    if method == "gmres":
        kw.update(restart=a.get("restart", 12), solve_method="incremental" if solver.endswith("incremental") else "batched")
    if a["entry"] == "solver":
        x_loc, rec = SparseSolver().solve(Arb, b_loc, method=method, backend="module_a", M=P, **kw)
        info = 0 if rec.converged else -1
    else:
        x_loc, info = getattr(module_a, method)(Arb, b_loc, M=P, **kw)
    st = module_a.get_last_stats()
    x2, info2 = getattr(module_a, method)(Arb, b_loc, x0=x_loc, M=P, **kw)     # cached plan and dinv, warm start
    st2 = module_a.get_last_stats()
    counts = None
    if a.get("count"):                 # group_end calls per iteration: Jacobi CG against plain CG on this partition
        prob, dinv = Arb._prob, Arb._jacobi[2]
        c = {}
        for pre in (False, True):
            for k in (3, 8):
                before = prob.group_ends
                dist_cg(prob, tol=0.0, maxiter=k, dinv=dinv if pre else None)
                c[f"{'p' if pre else ''}cg_{k}"] = prob.group_ends - before
        counts = c
    kname = _hipk.CsrHandle.last_spmv_kernel()
    pieces = [None] * world
    dist.all_gather_object(pieces, (r0, x_loc.cpu().numpy().copy(), int(info), st.iterations, st.residual_norm,
                                    x2.cpu().numpy().copy(), int(info2), st2.iterations, st.preconditioner, counts, kname))
    if rank != 0:
        return None
    pieces.sort(key=lambda q: q[0])
    x = np.concatenate([p[1] for p in pieces])
    x2g = np.concatenate([p[5] for p in pieces])
    crow, col, val = A.crow_indices().numpy(), A.col_indices().numpy(), A.values().numpy()
    dinv = JacobiPreconditioner(A).dinv.numpy()
    okw = dict(tol=tol, maxiter=None if maxiter < 0 else maxiter)
    if method == "gmres":
        okw.update(restart=kw["restart"], solve_method=kw["solve_method"], gpu_tolerances=True)
    orc = {"cg": O.pcg_jacobi, "bicgstab": O.bicgstab_jacobi, "gmres": O.gmres_jacobi}[method]
    ref = orc(crow, col, val, dinv, b.numpy(), **okw)
    ref2 = orc(crow, col, val, dinv, b.numpy(), x0=ref.x, **okw)
    # the single-device solve of the global system with the same preconditioner
    Ad, bd = A.to(dev), b.to(dev)
    xs, info_s = getattr(module_a, method)(Ad, bd, M=JacobiPreconditioner(Ad), **kw)
    ss = module_a.get_last_stats()
    return {"bitwise_equal": bool(np.array_equal(x, ref.x)), "single_equal": bool(np.array_equal(x, xs.cpu().numpy())),
            "single_vs_oracle": bool(np.array_equal(ref.x, xs.cpu().numpy())),
            "info": [p[2] for p in pieces], "ref_info": ref.info, "single_info": int(info_s),
            "iterations": [p[3] for p in pieces], "ref_iterations": ref.iterations, "single_iterations": ss.iterations,
            "residual_norm": [p[4] for p in pieces], "ref_residual_norm": ref.residual_norm,
            "single_residual_norm": ss.residual_norm,
            "second_bitwise_equal": bool(np.array_equal(x2g, ref2.x)), "second_info": [p[6] for p in pieces],
            "ref2_info": ref2.info, "second_iterations": [p[7] for p in pieces], "ref2_iterations": ref2.iterations,
            "preconditioner": [p[8] for p in pieces], "counts": [p[9] for p in pieces],
            "spmv_kernel": [p[10] for p in pieces], "n_local": [int(p[1].size) for p in pieces]}


def main():
    task, out, args = sys.argv[1], sys.argv[2], json.loads(sys.argv[3])
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    if task == "hip":
        res = hip_task(args, rank, world)
        if rank == 0:
            with open(out, "w") as f:
                json.dump(res, f)
    else:
        res = cpu_task(task, args, rank, world)
        pieces = [None] * world
        dist.all_gather_object(pieces, res)
        if rank == 0:
            with open(out, "w") as f:
                json.dump(pieces, f)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
