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
    """Host-staged collectives; records every collective call the C-driven loop makes, in order: ("group_start",),
    ("group_end",), ("all_gather", count, in_place), ("send", count, peer), ("recv", count, peer).  fail_nth = n: the n-th
    all_gather from then on returns ncclResult 7 instead of running."""

    def __init__(self, crow, col_global, val, b_local, part, ops, group=None):
        _from_block(self, crow, col_global, val, b_local, part, ops)
        self.calls, self.fail_nth = [], None

    def coll_struct(self):
        if getattr(self, "_recorded", None) is None:
            coll = super().coll_struct()
            g_start, g_end, a_gather, c_send, c_recv = self._cbs
            rank, calls = self.part.rank, self.calls

            def group_start():
                calls.append(("group_start",))
                return g_start()

            def group_end():
                calls.append(("group_end",))
                return g_end()

            def all_gather(send, recv, count, dtype, comm, stream):
                calls.append(("all_gather", int(count), send == recv + rank * count * 8))   # in place: arr + rank * per -> arr
                if self.fail_nth is not None:
                    self.fail_nth -= 1
                    if self.fail_nth == 0:
                        self.fail_nth = None
                        return 7
                return a_gather(send, recv, count, dtype, comm, stream)

            def send(buf, count, dtype, peer, comm, stream):
                calls.append(("send", int(count), int(peer)))
                return c_send(buf, count, dtype, peer, comm, stream)

            def recv(buf, count, dtype, peer, comm, stream):
                calls.append(("recv", int(count), int(peer)))
                return c_recv(buf, count, dtype, peer, comm, stream)
            self._recorded = (_hipk.COLL_GROUP_FN(group_start), _hipk.COLL_GROUP_FN(group_end),
                              _hipk.COLL_ALLGATHER_FN(all_gather), _hipk.COLL_SENDRECV_FN(send), _hipk.COLL_SENDRECV_FN(recv))
            addr = lambda f: ctypes.cast(f, ctypes.c_void_p).value   # noqa: E731
            coll.group_start, coll.group_end, coll.all_gather, coll.send, coll.recv = [addr(f) for f in self._recorded]
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
    from pytorch_sparse_solver.distributed import HipOps
    cls = FusedMailbox if a.get("comm") == "fused" else StagedCounting
    Arb = pss.RowBlockCSR.from_global_csr(A.to(dev), ops=HipOps(dev), problem_cls=cls)
    b_loc = b[r0:r1].to(dev)
    b_owner = None
    if a.get("b_layout") == "off1":    # optional: this rank's b as a contiguous view one element off a 16-byte boundary, in guards
        b_owner = torch.full((b_loc.numel() + 129,), -3.5e203, dtype=torch.float64, device=dev)
        b_owner[65:65 + b_loc.numel()] = b_loc
        b_snap = b_owner.clone()
        b_loc = b_owner[65:65 + r1 - r0]
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
    if a.get("count"):                 # every collective call of the six C loops on this partition, at two maxiter values each
        prob, dinv, pl = Arb._prob, Arb._jacobi[2], Arb._prob.plan
        traces = {}
        for solver, ks in (("cg", (3, 8)), ("bicgstab", (3, 8)), ("gmres", (1, 2))):
            for pre in ("", "p"):
                for k in ks:
                    before = len(prob.calls)
                    _dist_fn(solver)(prob, tol=0.0, maxiter=k, dinv=dinv if pre else None, **_GMRES_KW.get(solver, {}))
                    traces[f"{pre}{solver}_{k}"] = prob.calls[before:]
        counts = {"traces": traces, "per": prob.part.per, "n_send": pl.n_send, "n_ghost": pl.n_ghost, "slab": pl.slab,
                  "send_counts": [int(v) for v in pl.send_splits], "recv_counts": [int(v) for v in pl.recv_splits]}
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
    layout = {} if b_owner is None else {"b_mod16": b_loc.data_ptr() % 16, "b_owner_unchanged": bool(torch.equal(b_owner, b_snap))}
    return {**layout,
            "bitwise_equal": bool(np.array_equal(x, ref.x)), "single_equal": bool(np.array_equal(x, xs.cpu().numpy())),
            "single_vs_oracle": bool(np.array_equal(ref.x, xs.cpu().numpy())),
            "info": [p[2] for p in pieces], "ref_info": ref.info, "single_info": int(info_s),
            "iterations": [p[3] for p in pieces], "ref_iterations": ref.iterations, "single_iterations": ss.iterations,
            "residual_norm": [p[4] for p in pieces], "ref_residual_norm": ref.residual_norm,
            "single_residual_norm": ss.residual_norm,
            "second_bitwise_equal": bool(np.array_equal(x2g, ref2.x)), "second_info": [p[6] for p in pieces],
            "ref2_info": ref2.info, "second_iterations": [p[7] for p in pieces], "ref2_iterations": ref2.iterations,
            "preconditioner": [p[8] for p in pieces], "counts": [p[9] for p in pieces],
            "spmv_kernel": [p[10] for p in pieces], "n_local": [int(p[1].size) for p in pieces]}


_GMRES_KW = {"gmres": {"restart": 3}}


def _dist_fn(solver):
    from pytorch_sparse_solver import distributed
    return getattr(distributed, "dist_" + solver)


def entry_status(prob, solver, dinv, spoil=None, fail_nth=None):
    """One dist_<solver> call on `prob` (tol 0, 4 iterations or cycles).  spoil(args) spoils one argument of its
    hipk_dist_*_solve call first; fail_nth = n makes the n-th all_gather return ncclResult 7.  Returns the entry point's status
    and hipk_last_error()."""
    L = _hipk.lib()
    name = f"hipk_dist_{'p' if dinv is not None else ''}{solver}_solve"
    entry, seen = getattr(L, name), []

    def call(*args):
        args = list(args)
        if spoil is not None:
            spoil(args)
        seen.append(entry(*args))
        return seen[-1]
    setattr(L, name, call)
    prob.fail_nth = fail_nth
    try:
        _dist_fn(solver)(prob, tol=0.0, maxiter=4, dinv=dinv, **_GMRES_KW.get(solver, {}))
    except _hipk.HipkError:
        pass
    finally:
        setattr(L, name, entry)
        prob.fail_nth = None
    torch.cuda.synchronize()
    return seen[0], L.hipk_last_error().decode()


def hip_errors_task(a, rank, world):
    """World 1, host-staged collectives: the status and error text of each of the six entry points for a failed all_gather
    and for single bad arguments."""
    A, b = global_system("vardiff", a["nx"], a["ny"])
    dev = torch.device("cuda", 0)
    from pytorch_sparse_solver.distributed import HipOps
    Arb = pss.RowBlockCSR.from_global_csr(A.to(dev), ops=HipOps(dev), problem_cls=StagedCounting)
    module_a.cg(Arb, b.to(dev), M=JacobiPreconditioner(Arb), maxiter=2)    # builds the problem and the dinv cache
    prob, dinv = Arb._prob, Arb._jacobi[2]
    out = {}
    for solver in ("cg", "bicgstab", "gmres"):
        for pre in ("", "p"):
            d, k = (dinv, 1) if pre else (None, 0)   # the argument list of hipk_dist_p*_solve has dinv at 3
            cases = {"nccl": dict(fail_nth=a["fail_nth"]),
                     "null": dict(spoil=lambda v, k=k: v.__setitem__(3 + k, None)),                 # b_local
                     "work": dict(spoil=lambda v, k=k: v.__setitem__(6 + k, v[6 + k] - 8)),         # work_bytes
                     "align": dict(spoil=lambda v, k=k: v.__setitem__(4 + k, v[4 + k] + 8)),        # x_ext
                     "rank": dict(spoil=lambda v: setattr(v[1]._obj, "rank", v[1]._obj.world))}
            if solver == "gmres":
                cases["restart"] = dict(spoil=lambda v, k=k: setattr(v[7 + k]._obj, "restart", 32))
            if pre:
                cases["dinv"] = dict(spoil=lambda v: v.__setitem__(3, None))
            out[pre + solver] = {case: entry_status(prob, solver, d, **kw) for case, kw in cases.items()}
    return out


def main():
    task, out, args = sys.argv[1], sys.argv[2], json.loads(sys.argv[3])
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    if task.startswith("hip"):
        res = (hip_task if task == "hip" else hip_errors_task)(args, rank, world)
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
