"""Worker of tests/test_dist_chebyshev.py: one rank of the row-partitioned cg with M = the Chebyshev polynomial preconditioner of
the global system (`ChebyshevPreconditioner.for_row_block`, or one of the replicated global matrix), and of that preconditioner's
apply on its own.  cpu tasks: gloo + the CPU ops double (the constructor, the torch form of the apply, the errors); hip tasks:
several ranks share cuda:0, hipk_dist_cheb_apply / hipk_dist_chebcg_solve run with host-staged stand-ins for the collectives
(tests/_dist_worker.py, tests/_dist_jacobi_worker.py)."""
import ctypes
import json
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pytorch-sparse-linalg-torch-amgx.cg.bicg.gmres_amd"), os.path.join(ROOT, "tests")]

from _dist_jacobi_worker import StagedCounting, global_system  # noqa: E402
from dist_cpu_ops import OracleOps  # noqa: E402
from oracle import oracle as O  # noqa: E402
import pytorch_sparse_solver as pss  # noqa: E402
from pytorch_sparse_solver import SparseSolver, _hipk  # noqa: E402
from pytorch_sparse_solver import module_a  # noqa: E402
from pytorch_sparse_solver.module_a import ChebyshevPreconditioner  # noqa: E402
from pytorch_sparse_solver.utils.matrix_utils import create_poisson_2d_csr, create_variable_diffusion_2d_csr  # noqa: E402

COEF = ("c0", "c1", "c2", "scale", "lmin", "lmax")


def system(kind, nx, ny):
    if kind == "poisson_ones":
        return create_poisson_2d_csr(nx, ny), torch.ones(nx * ny, dtype=torch.float64)
    return global_system(kind, nx, ny)


def coef_of(P):
    return [getattr(P, k) for k in COEF]


# ------------------------------------------------------------------------------------------------------------------ CPU
def cpu_task(task, a, rank, world):
    A, b = system(a["kind"], a["nx"], a["ny"])
    n = A.shape[0]
    r0, r1 = pss.RowBlockCSR.row_range(n)
    if task == "zero":                 # a zero on the diagonal of the LAST rank's rows only
        crow, col, val = A.crow_indices(), A.col_indices(), A.values().clone()
        i = n - 3
        j = int(crow[i]) + int((col[int(crow[i]):int(crow[i + 1])] == i).nonzero()[0])
        val[j] = 0.0
        A = torch.sparse_csr_tensor(crow, col, val, A.shape)
    Arb = pss.RowBlockCSR.from_global_csr(A, ops=OracleOps())
    if task == "coef":
        out = {"cases": [], "rows": [r0, r1]}
        for degree in (1, 3, 6):
            for normalize in (True, False):
                for lmax in (None, 2.25):
                    P = ChebyshevPreconditioner.for_row_block(Arb, degree=degree, normalize=normalize, lmax=lmax)
                    G = ChebyshevPreconditioner(A, degree=degree, normalize=normalize, lmax=lmax)
                    out["cases"].append({"degree": degree, "normalize": normalize, "lmax": lmax,
                                         "coef_equal": coef_of(P) == coef_of(G) and list(P._coef) == list(G._coef),
                                         "dinv_equal": bool(torch.equal(P.dinv, G.dinv[r0:r1])), "shape": list(P.shape),
                                         "row_range": list(P.row_range), "degree_attr": P.degree,
                                         "counters": [P.applies, P.spmvs]})
        return out
    if task == "apply":
        v = torch.randn(n, dtype=torch.float64, generator=torch.Generator().manual_seed(17))
        out = {"equal": {}, "counters": None, "rows": [r0, r1]}
        for degree in (1, 2, 5):
            P = ChebyshevPreconditioner.for_row_block(Arb, degree=degree)
            z = P(v[r0:r1].clone())
            zg = ChebyshevPreconditioner(A, degree=degree)(v)
            out["equal"][str(degree)] = bool(torch.equal(z, zg[r0:r1]))
            out["counters"] = [P.applies, P.spmvs]
        return out
    if task == "zero":
        try:
            ChebyshevPreconditioner.for_row_block(Arb)
            return {"raised": ""}
        except ValueError as e:
            return {"raised": str(e)}
    assert task == "errors"
    b_loc = b[r0:r1].clone()
    P = ChebyshevPreconditioner.for_row_block(Arb)
    out = {}

    def attempt(name, fn, *exc):
        try:
            fn()
            out[name] = "no error"
        except exc as e:
            out[name] = f"{type(e).__name__}: {e}"
    attempt("bicgstab", lambda: module_a.bicgstab(Arb, b_loc, M=P), ValueError)
    attempt("gmres", lambda: module_a.gmres(Arb, b_loc, M=P), ValueError)
    attempt("solver_gmres", lambda: SparseSolver().solve(Arb, b_loc, method="gmres", backend="module_a", M=P), ValueError)
    attempt("cpu_cg", lambda: module_a.cg(Arb, b_loc, M=P), RuntimeError)
    attempt("cpu_cg_global", lambda: module_a.cg(Arb, b_loc, M=ChebyshevPreconditioner(A)), RuntimeError)
    attempt("constructor", lambda: ChebyshevPreconditioner(Arb), ValueError)
    Pw = ChebyshevPreconditioner.for_row_block(Arb)
    Pw.row_range = (r0 + 1, r1 + 1)
    attempt("wrong_rows", lambda: module_a.cg(Arb, b_loc, M=Pw), ValueError)
    other = pss.RowBlockCSR.from_global_csr(create_variable_diffusion_2d_csr(a["nx"], a["ny"] + 1), ops=OracleOps())
    Ps = ChebyshevPreconditioner.for_row_block(other)
    attempt("wrong_shape", lambda: module_a.cg(Arb, b_loc, M=Ps), ValueError)
    attempt("wrong_shape_global", lambda: module_a.cg(Arb, b_loc, M=ChebyshevPreconditioner(create_poisson_2d_csr(4, 5))),
            ValueError)
    attempt("callable", lambda: module_a.cg(Arb, b_loc, M=lambda v: v), ValueError)
    return out


# ------------------------------------------------------------------------------------------------------------------ GPU
DEV = torch.device("cuda", 0)


def row_block(A, cls=StagedCounting):
    from pytorch_sparse_solver.distributed import HipOps
    return pss.RowBlockCSR.from_global_csr(A.to(DEV), ops=HipOps(DEV), problem_cls=cls)


def gathered(rank, world, payload):
    pieces = [None] * world
    dist.all_gather_object(pieces, payload)
    return sorted(pieces, key=lambda q: q[0]) if rank == 0 else None


def hip_apply_task(a, rank, world):
    """hipk_dist_cheb_apply through P(v_local), degrees 1, 2 and 5, with HIPK_CHEB_FUSED unset and 0: every rank's slice, the
    kernel note after each apply."""
    from _cheb_mirror import mirror
    A, _ = system(a["kind"], a["nx"], a["ny"])
    n = A.shape[0]
    r0, r1 = pss.RowBlockCSR.row_range(n)
    Arb = row_block(A)
    v = torch.from_numpy(np.random.default_rng(n).standard_normal(n))
    vd = v[r0:r1].to(DEV)
    mine = {}
    for degree in (1, 2, 5):
        P = ChebyshevPreconditioner.for_row_block(Arb, degree=degree)
        for fused in ("1", "0"):
            os.environ["HIPK_CHEB_FUSED"] = fused
            z = P(vd)
            mine[f"{degree}/{fused}"] = (z.cpu().numpy().copy(), _hipk.CsrHandle.last_spmv_kernel())
        os.environ.pop("HIPK_CHEB_FUSED")
        assert torch.equal(vd, v[r0:r1].to(DEV)) and (P.applies, P.spmvs) == (2, 2 * degree)
    # a solve on the same operand after the applies
    P3 = ChebyshevPreconditioner.for_row_block(Arb, degree=3)
    b = torch.randn(n, dtype=torch.float64, generator=torch.Generator().manual_seed(11))
    x_loc, info = module_a.cg(Arb, b[r0:r1].to(DEV), tol=1e-8, M=P3)
    pieces = gathered(rank, world, (r0, mine, x_loc.cpu().numpy().copy(), int(info), Arb._prob.plan.n_ghost, Arb._prob.n_ext))
    if rank != 0:
        return None
    O.build()
    crow, col, val = A.crow_indices().numpy(), A.col_indices().numpy(), A.values().numpy()
    Ad = A.to(DEV)
    h = _hipk.handle_for(Ad)
    res = {"cases": {}, "n_local": [int(p[2].size) for p in pieces], "n_ghost": [p[4] for p in pieces], "n_ext": [p[5] for p in pieces]}
    for key in pieces[0][1]:
        degree = int(key.split("/")[0])
        G = ChebyshevPreconditioner(A, degree=degree)
        z = np.concatenate([p[1][key][0] for p in pieces])
        single = _hipk.cheb_apply(h, degree, G.dinv.to(DEV), G._coef, v.to(DEV)).cpu().numpy()
        res["cases"][key] = {"mirror_equal": bool(np.array_equal(z, mirror(O, crow, col, val, G, v.numpy()))),
                             "single_equal": bool(np.array_equal(z, single)), "notes": [p[1][key][1] for p in pieces]}
    xs, info_s = module_a.cg(Ad, b.to(DEV), tol=1e-8, M=ChebyshevPreconditioner(Ad, degree=3))
    res["solve_after_equal"] = bool(np.array_equal(np.concatenate([p[2] for p in pieces]), xs.cpu().numpy()))
    res["solve_after_info"] = [[p[3] for p in pieces], int(info_s)]
    return res


def hip_solve_task(a, rank, world):
    """cg(A_rb, b_loc, M=P) against the single-device cg(A, b, M=ChebyshevPreconditioner(A)): the table of
    tests/test_dist_chebyshev.py.  golden: the system of a tests/golden fixture instead of a generated one."""
    degree, tol, maxiter = a.get("degree", 3), a["tol"], a["maxiter"]
    normalize = a.get("normalize", True)
    x0 = None
    if a.get("golden"):
        from _cheb_mirror import csr
        d = np.load(os.path.join(ROOT, "tests", "golden", a["golden"] + ".npz"))
        A, b = csr(d), torch.from_numpy(d["b"])
        x0 = torch.from_numpy(d["x0"]) if a.get("has_x0") else None
    else:
        A, b = system(a["kind"], a["nx"], a["ny"])
    n = A.shape[0]
    r0, r1 = pss.RowBlockCSR.row_range(n)
    Arb = row_block(A)
    Ad, bd = A.to(DEV), b.to(DEV)
    b_loc = bd[r0:r1].clone()
    if a["pmode"] == "local":
        P = ChebyshevPreconditioner.for_row_block(Arb, degree=degree, normalize=normalize)
    else:
        P = ChebyshevPreconditioner(Ad, degree=degree, normalize=normalize)
    kw = {"tol": tol}
    if maxiter >= 0:
        kw["maxiter"] = maxiter
    if x0 is not None:
        kw["x0"] = x0[r0:r1].to(DEV)
    if a.get("entry") == "solver":
        x_loc, rec = SparseSolver().solve(Arb, b_loc, method="cg", backend="module_a", M=P, **kw)
        info = 0 if rec.converged else -1
    else:
        x_loc, info = module_a.cg(Arb, b_loc, M=P, **kw)
    st = module_a.get_last_stats()
    applies, spmvs = P.applies, P.spmvs
    path, note = _hipk.last_solve_path(), _hipk.CsrHandle.last_spmv_kernel()
    kw2 = dict(kw, x0=x_loc)
    x2, info2 = module_a.cg(Arb, b_loc, M=P, **kw2)            # cached plan and dinv, warm start
    st2 = module_a.get_last_stats()
    traces = None
    if a.get("trace"):
        from pytorch_sparse_solver.distributed import dist_cg
        prob, pl = Arb._prob, Arb._prob.plan
        traces = {"per": prob.part.per, "slab": pl.slab, "send_counts": [int(v) for v in pl.send_splits],
                  "recv_counts": [int(v) for v in pl.recv_splits], "runs": {}}
        for m in (1, 3):
            Pm = ChebyshevPreconditioner.for_row_block(Arb, degree=m)
            ext = Arb._jacobi_ext(prob, Pm)
            for k in (3, 8):
                before = len(prob.calls)
                dist_cg(prob, tol=0.0, maxiter=k, dinv=ext, cheb=(m, Pm._coef))
                traces["runs"][f"{m}_{k}"] = prob.calls[before:]
    pieces = gathered(rank, world, (r0, x_loc.cpu().numpy().copy(), int(info), st.iterations, st.residual_norm, st.preconditioner,
                                    applies, spmvs, x2.cpu().numpy().copy(), int(info2), st2.iterations, st2.residual_norm, path,
                                    note, traces, coef_of(P), st.matvecs))
    if rank != 0:
        return None
    # the single-device solve of the global system; its preconditioner is built from the global matrix
    G = P if a["pmode"] == "global" else ChebyshevPreconditioner(Ad, degree=degree, normalize=normalize, lmax=P.lmax, lmin=P.lmin)
    kws = dict(kw)
    if x0 is not None:
        kws["x0"] = x0.to(DEV)
    xs, info_s = module_a.cg(Ad, bd, M=G, **kws)
    ss = module_a.get_last_stats()
    xs2, info_s2 = module_a.cg(Ad, bd, M=G, **dict(kws, x0=xs))
    ss2 = module_a.get_last_stats()
    x = np.concatenate([p[1] for p in pieces])
    x2g = np.concatenate([p[8] for p in pieces])
    res = {"single_equal": bool(np.array_equal(x, xs.cpu().numpy())), "info": [p[2] for p in pieces], "single_info": int(info_s),
           "iterations": [p[3] for p in pieces], "single_iterations": ss.iterations,
           "residual_norm": [p[4] for p in pieces], "single_residual_norm": ss.residual_norm,
           "preconditioner": [p[5] for p in pieces], "applies": [p[6] for p in pieces], "spmvs": [p[7] for p in pieces],
           "second_equal": bool(np.array_equal(x2g, xs2.cpu().numpy())), "second_info": [p[9] for p in pieces],
           "single_second_info": int(info_s2), "second_iterations": [p[10] for p in pieces], "single_second_iterations": ss2.iterations,
           "second_residual_norm": [p[11] for p in pieces], "single_second_residual_norm": ss2.residual_norm,
           "solve_path": [p[12] for p in pieces], "notes": [p[13] for p in pieces], "traces": [p[14] for p in pieces],
           "coef_equal_global": [p[15] == coef_of(ChebyshevPreconditioner(A, degree=degree, normalize=normalize)) for p in pieces],
           "matvecs": [p[16] for p in pieces], "degree": degree, "n_local": [int(p[1].size) for p in pieces]}
    if a.get("golden"):
        x_ref = d[a["tag"] + "_x"]
        res["golden_err"] = float(np.linalg.norm(x - x_ref) / np.linalg.norm(x_ref))
    return res


def entry_status(prob, name, run, spoil=None, fail_nth=None):
    """One call of the entry point `name` through run(); spoil(args) spoils one argument first, fail_nth = n makes the n-th
    all_gather return ncclResult 7.  Returns the entry point's status and hipk_last_error()."""
    L = _hipk.lib()
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
        run()
    except _hipk.HipkError:
        pass
    finally:
        setattr(L, name, entry)
        prob.fail_nth = None
    torch.cuda.synchronize()
    return seen[0], L.hipk_last_error().decode()


def hip_errors_task(a, rank, world):
    """World 1, host-staged collectives: status and error text of the two entry points for single bad arguments and for a failed
    all_gather.  Argument positions: (A, plan, coll, degree, dinv, coef, b | r, x | z, work, work_bytes, ...)."""
    from pytorch_sparse_solver.distributed import dist_cg, dist_cheb_apply
    A, b = global_system("vardiff", a["nx"], a["ny"])
    Arb = row_block(A)
    P = ChebyshevPreconditioner.for_row_block(Arb, degree=3)
    module_a.cg(Arb, b.to(DEV), M=P, maxiter=2)    # builds the problem and the dinv cache
    prob, ext = Arb._prob, Arb._jacobi[2]
    v = b.to(DEV)
    runs = {"hipk_dist_chebcg_solve": lambda: dist_cg(prob, tol=0.0, maxiter=4, dinv=ext, cheb=(3, P._coef)),
            "hipk_dist_cheb_apply": lambda: dist_cheb_apply(prob, 3, ext, P._coef, v)}
    out = {}
    for name, run in runs.items():
        cases = {"null": dict(spoil=lambda v: v.__setitem__(6, None)),
                 "coef": dict(spoil=lambda v: v.__setitem__(5, None)),
                 "dinv": dict(spoil=lambda v: v.__setitem__(4, None)),
                 "work": dict(spoil=lambda v: v.__setitem__(9, v[9] - 8)),
                 "align": dict(spoil=lambda v: v.__setitem__(7, v[7] + 8)),
                 "degree0": dict(spoil=lambda v: v.__setitem__(3, 0)),
                 "degree33": dict(spoil=lambda v: v.__setitem__(3, 33)),
                 "rank": dict(spoil=lambda v: setattr(v[1]._obj, "rank", v[1]._obj.world))}
        if name.endswith("solve"):
            cases["nccl"] = dict(fail_nth=a["fail_nth"])
        out[name] = {case: entry_status(prob, name, run, **kw) for case, kw in cases.items()}
    return out


def main():
    task, out, args = sys.argv[1], sys.argv[2], json.loads(sys.argv[3])
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    if task.startswith("hip"):
        res = {"hip_apply": hip_apply_task, "hip_solve": hip_solve_task, "hip_errors": hip_errors_task}[task](args, rank, world)
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
