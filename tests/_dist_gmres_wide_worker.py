"""Worker of tests/test_dist_gmres_wide.py: one rank of the row-partitioned GMRES at restart 32 .. 255
(hipk_dist_{p,}gmres_wide_solve).  Several ranks share cuda:0; the collectives are host-staged stand-ins that record every call
(StagedCounting) or the device mailboxes sized for the multi-dot block."""
import json
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pytorch-sparse-linalg-torch-amgx.cg.bicg.gmres_amd"), os.path.join(ROOT, "tests")]

from _dist_jacobi_worker import StagedCounting, _from_block  # noqa: E402
from _dist_worker import MailboxNative, build_global  # noqa: E402
from oracle import oracle as O  # noqa: E402
import pytorch_sparse_solver as pss  # noqa: E402
from pytorch_sparse_solver import _hipk, module_a  # noqa: E402
from pytorch_sparse_solver.distributed import HipOps, P2PComm, dist_gmres  # noqa: E402
from pytorch_sparse_solver.module_a import JacobiPreconditioner  # noqa: E402
from pytorch_sparse_solver.utils.matrix_utils import create_variable_diffusion_2d_csr  # noqa: E402


class WideMailbox(MailboxNative):
    """The device mailboxes sized as DistProblem sizes them: the multi-dot block of restart 255, 256 * per doubles."""

    def __init__(self, crow, col_global, val, b_local, part, ops, group=None):
        _from_block(self, crow, col_global, val, b_local, part, ops)
        self.p2p = P2PComm(part.rank, part.world, ops.device, max(256 * part.per, self.plan.slab))


def global_system(kind, nx, ny):
    if kind == "vardiff":
        A = create_variable_diffusion_2d_csr(nx, ny)
        b = torch.randn(nx * ny, dtype=torch.float64, generator=torch.Generator().manual_seed(11))
        return A, b
    if kind == "scaled_identity":
        # A = 2 I: w = A v_0 is 2 v_0 exactly and the two CGS passes leave ||q|| below eps ||w|| -- the Krylov space closes at the
        # first step of the cycle, whatever the rounding of the partial sums
        n = nx * ny
        A = (2.0 * torch.eye(n, dtype=torch.float64)).to_sparse_csr()
        b = torch.randn(n, dtype=torch.float64, generator=torch.Generator().manual_seed(11))
        return A, b
    if kind == "fewvals":
        # block diagonal, 2 x 2 upper Jordan blocks with 4 distinct eigenvalues: the minimal polynomial has degree 8, so the Krylov
        # space of any b closes at step 8 in exact arithmetic (whether ||q|| falls below the breakdown threshold there is rounding)
        n = nx * ny
        lam = torch.tensor([2.0, 3.0, 5.0, 7.0], dtype=torch.float64)[(torch.arange(n) // 2) % 4]
        i = torch.arange(n)
        even = i[(i % 2 == 0) & (i + 1 < n)]
        idx = torch.cat([torch.stack([i, i]), torch.stack([even, even + 1])], dim=1)
        val = torch.cat([lam, torch.ones(even.numel(), dtype=torch.float64)])
        A = torch.sparse_coo_tensor(idx, val, (n, n)).coalesce().to_sparse_csr()
        b = torch.randn(n, dtype=torch.float64, generator=torch.Generator().manual_seed(11))
        return A, b
    return build_global(kind, nx, ny)


def _single(A, b, dev, m, kw, jacobi, x0=None):
    Ad, bd = A.to(dev), b.to(dev)
    extra = {"M": JacobiPreconditioner(Ad)} if jacobi else {}
    xs, info = module_a.gmres(Ad, bd, x0=None if x0 is None else x0.to(dev), restart=m, **kw, **extra)
    st = module_a.get_last_stats()
    return xs.cpu().numpy(), {"info": int(info), "iterations": int(st.iterations), "matvecs": int(st.matvecs),
                              "residual_norm": float(st.residual_norm), "breakdown": int(bool(st.breakdown))}


def hip_task(a, rank, world):
    """gmres(A_rb, b_loc, restart=m) with the ranks' x concatenated, against the single-device solve (and the oracle)."""
    A, b = global_system(a["kind"], a["nx"], a["ny"])
    n, m = A.shape[0], a["restart"]
    r0, r1 = pss.RowBlockCSR.row_range(n)
    dev = torch.device("cuda", 0)
    if a.get("comm") == "product":      # the product's DistProblem (HIPK_DIST_COMM picks the provider)
        Arb = pss.RowBlockCSR.from_global_csr(A.to(dev))
    else:
        cls = WideMailbox if a.get("comm") == "mailbox" else StagedCounting
        Arb = pss.RowBlockCSR.from_global_csr(A.to(dev), ops=HipOps(dev), problem_cls=cls)
    b_loc = b[r0:r1].to(dev)
    kw = {"tol": a["tol"], "solve_method": a["solve_method"]}
    if a["maxiter"] >= 0:
        kw["maxiter"] = a["maxiter"]
    jacobi = a.get("jacobi", False)
    extra = {"M": JacobiPreconditioner(Arb)} if jacobi else {}
    x0 = None
    if a.get("warm"):     # a warm start: the single-device solve of one cycle, its slice on every rank
        x0 = torch.from_numpy(_single(A, b, dev, m, dict(kw, maxiter=1), jacobi)[0])
    x_loc, info = module_a.gmres(Arb, b_loc, x0=None if x0 is None else x0[r0:r1].to(dev), restart=m, **kw, **extra)
    st = module_a.get_last_stats()
    mine = {"info": int(info), "iterations": int(st.iterations), "matvecs": int(st.matvecs),
            "residual_norm": float(st.residual_norm), "breakdown": int(st.breakdown)}
    counts = None
    if a.get("count"):   # every collective call of the wide loop, plain and Jacobi, at maxiter 1 and 2
        prob, pl = Arb._prob, Arb._prob.plan
        dinv = JacobiPreconditioner(Arb).dinv
        from pytorch_sparse_solver.distributed import jacobi_dinv_ext
        dext = jacobi_dinv_ext(prob, dinv)
        traces = {}
        for pre in ("", "p"):
            for k in (1, 2):
                before = len(prob.calls)
                dist_gmres(prob, tol=0.0, maxiter=k, restart=m, dinv=dext if pre else None)
                traces[f"{pre}gmres_{k}"] = prob.calls[before:]
        counts = {"traces": traces, "per": prob.part.per, "slab": pl.slab,
                  "send_counts": [int(v) for v in pl.send_splits], "recv_counts": [int(v) for v in pl.recv_splits]}
    pieces = [None] * world
    dist.all_gather_object(pieces, (r0, x_loc.cpu().numpy().copy(), mine, counts, Arb._prob.comm_kind))
    if rank != 0:
        return None
    pieces.sort(key=lambda q: q[0])
    x = np.concatenate([p[1] for p in pieces])
    xs, single = _single(A, b, dev, m, kw, jacobi, x0)
    out = {"single_equal": bool(np.array_equal(x, xs)), "ranks": [p[2] for p in pieces], "single": single,
           "counts": [p[3] for p in pieces], "comm": [p[4] for p in pieces], "n_local": [int(p[1].size) for p in pieces]}
    if a.get("oracle"):
        crow, col, val = A.crow_indices().numpy(), A.col_indices().numpy(), A.values().numpy()
        ref = O.gmres(crow, col, val, b.numpy(), tol=a["tol"], restart=m, maxiter=kw.get("maxiter"),
                      solve_method=a["solve_method"], gpu_tolerances=True)
        out["oracle_equal"] = bool(np.array_equal(x, ref.x))
        out["oracle"] = {"info": int(ref.info), "iterations": int(ref.iterations)}
    return out


def hip_errors_task(a, rank, world):
    """World 1: status and text of both wide entry points for restart 31 / 256, a workspace one byte short and a failed
    all-gather."""
    A, b = global_system("vardiff", a["nx"], a["ny"])
    dev = torch.device("cuda", 0)
    Arb = pss.RowBlockCSR.from_global_csr(A.to(dev), ops=HipOps(dev), problem_cls=StagedCounting)
    module_a.cg(Arb, b.to(dev), M=JacobiPreconditioner(Arb), maxiter=2)    # builds the problem and the dinv cache
    prob, dinv = Arb._prob, Arb._jacobi[2]
    out = {}
    for pre in ("", "p"):
        d, k = (dinv, 1) if pre else (None, 0)   # the argument list of hipk_dist_p*_solve has dinv at 3
        cases = {"nccl": dict(fail_nth=a["fail_nth"]),
                 "work": dict(spoil=lambda v, k=k: v.__setitem__(6 + k, v[6 + k] - 1)),        # work_bytes, one byte short
                 "restart31": dict(spoil=lambda v, k=k: setattr(v[7 + k]._obj, "restart", 31)),
                 "restart256": dict(spoil=lambda v, k=k: setattr(v[7 + k]._obj, "restart", 256))}
        res = {case: _wide_status(prob, d, **kw) for case, kw in cases.items()}
        L = _hipk.lib()
        plan = _plan_of(prob)
        res["bytes"] = {str(r): int(getattr(L, f"hipk_dist_{pre}gmres_wide_work_bytes")(plan, r)) for r in (31, 32, 255, 256)}
        out[pre + "gmres"] = res
    return out


def _plan_of(prob):
    import ctypes
    p = _hipk.DistPlan()
    p.rank, p.world, p.n_local, p.n_ext, p.n_global = prob.part.rank, prob.part.world, prob.n_local, prob.n_ext, prob.part.n_global
    p.chunk_rows, p.g_red, p.per, p.slab = prob.part.ch, prob.part.g, prob.part.per, prob.plan.slab
    return ctypes.byref(p)


def _wide_status(prob, dinv, spoil=None, fail_nth=None):
    """One dist_gmres call at restart 40 (the wide entry point), with one argument of the call spoilt or the n-th all-gather
    failing; the entry point's status and hipk_last_error()."""
    L = _hipk.lib()
    name = f"hipk_dist_{'p' if dinv is not None else ''}gmres_wide_solve"
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
        dist_gmres(prob, tol=0.0, maxiter=1, restart=40, dinv=dinv)
    except _hipk.HipkError:
        pass
    finally:
        setattr(L, name, entry)
        prob.fail_nth = None
    torch.cuda.synchronize()
    return [seen[0], L.hipk_last_error().decode()]


def main():
    task, out, args = sys.argv[1], sys.argv[2], json.loads(sys.argv[3])
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    res = (hip_task if task == "hip" else hip_errors_task)(args, rank, world)
    if rank == 0:
        with open(out, "w") as f:
            json.dump(res, f)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
