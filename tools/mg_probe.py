"""AggregationMultigridPreconditioner against plain cg and the Chebyshev preconditioner on one MI355X, fp64, one process.

For every system -- 5-point Poisson 1000^2, 2000^2 and 4000^2, `create_variable_diffusion_2d_csr(2000, 2000)`, 7-point Poisson 128^3;
b = ones, cg(tol=1e-6) -- the four configurations
    plain | ChebyshevPreconditioner(degree=3) | multigrid degree 1 | multigrid degree 2
are solved `--reps` times in alternation (plain, cheb, mg1, mg2, plain, ...): wall clock around the whole public call, device
synchronised before and after; iterations, info and the true relative residual are recorded, times as min..max.  Plain cg does not
touch the code of this preconditioner: it is the library's path as it was.  The preconditioners are built once per system (the
set-up time is printed, it is not part of a solve).

Then the device time of one multigrid apply (HIP events around `--applies` applies, degree 1) at tail_rows 0 / 256 / 1024 / 4096:
what the one-launch tail kernel is worth against the launch sequence on the same levels.  MG_TAIL_MAX_ROWS is set from the
2000^2 row.

  python tools/mg_probe.py                                  # everything; one JSON line per system
  python tools/mg_probe.py --systems poisson2000 --reps 1 --configs mg1 --applies 0      # one solve (for rocprofv3 --kernel-trace)

`--graph`: `AggregationMultigridPreconditioner.from_graph` (aggregates from the matrix graph, degrees 1 and 2: gmg1, gmg2) beside the
grid class (mg1) and plain cg on the same systems and on an anisotropic 5-point operator (y-coupling x 0.01, 2000^2); the level sizes,
the handshake rounds, the longest row of any level and the set-up time of the graph hierarchy are recorded, and the tail_rows sweep
times the GRAPH hierarchy's apply.  profiles/mg_graph_probe.txt is its output.

  python tools/mg_probe.py --graph --reps 2

`--graph` also runs `from_graph(degree=1, coarse_rows=K)` for K = 256 / 512 / 1024 / 2048 (gmg1c256 ... gmg1c2048: the hierarchy cut
at a dense coarsest level) next to gmg1 in the same alternation, and records per configuration the levels, the launches of an apply
and `tail_from`, and the device time of the dense step alone in both forms: the launch `hipk_mg_dense_apply` and, up to 512 rows,
the one-workgroup tail `hipk_mg_gtail_dense_apply` on that level alone.  A last line times both forms on random matrices of
256 / 512 / 1024 / 2048 rows.  profiles/mg_dense_probe.txt is the output of

  python tools/mg_probe.py --graph --reps 2 --applies 0 --configs plain mg1 gmg1 gmg1c256 gmg1c512 gmg1c1024 gmg1c2048

`--refresh`: `update()` against a fresh construction, on Poisson 2000^2, variable diffusion 2000^2 and 7-point 128^3 (`--systems`)
under the grid class, `from_graph()` and `from_graph(coarse_rows=2048)` (`--configs grid graph graph_c2048`).  Per line: the wall
clock of a fresh construction in the same process (the yardstick), of the first `update` (the plan's build included), the mean of
five later ones, and the split of one later update into Galerkin sums, scans, handles, dense inverse and norm estimate (measured
with a synchronised clock around each step, so its total is above an unclocked update).  Then ten steps of changing coefficients
(D A D for a moving diagonal D) three ways: rebuild + solve, update + solve, and the stale object + solve (capped at 500
iterations), with the iteration counts.  The lines also go to profiles/mg_refresh_probe.txt (`--out`), stamped with the build id.

  python tools/mg_probe.py --refresh

`--cycle W`: every multigrid configuration is built with `cycle="W"`; a configuration name that ends in `w` (mg1w, gmg1c2048w) is the
W-cycle whatever `--cycle` says, so V and W of one hierarchy are solved in the same alternation of the same process.  Every
multigrid configuration records its cycle, `launches_per_apply` and `tail_from`.  profiles/mg_wcycle_probe.txt is the output of

  python tools/mg_probe.py --graph --reps 2 --applies 0 --configs plain mg1 mg1w gmg1c2048 gmg1c2048w --out profiles/mg_wcycle_probe.txt
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
TAILS = (0, 256, 1024, 4096)
CUTS = (256, 512, 1024, 2048)


def _event_us(fn, calls=50):
    """Device time of one call of fn (HIP events around `calls` calls, the best of three)."""
    for _ in range(3):
        fn()
    best = float("inf")
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, 1e3 * e0.elapsed_time(e1) / calls)
    return round(best, 1)


def dense_step_us(cinv, n, ld):
    """{"launch": us, "tail": us or None}: z = cinv r alone as hipk_mg_dense_apply and as hipk_mg_gtail_dense_apply with one level."""
    from pytorch_sparse_solver import _hipk
    r, z = torch.randn(n, dtype=cinv.dtype, device=DEV), torch.empty(n, dtype=cinv.dtype, device=DEV)
    out = {"n": n, "launch": _event_us(lambda: _hipk.mg_dense_apply(cinv, ld, 1.0, r, z)), "tail": None}
    ref = z.clone()
    if n <= _hipk.MG_DENSE_TAIL_N:
        tail = _hipk.MgGTail([{"n": n}], 1, cinv=cinv, ld=ld)
        work = torch.empty(tail.work_bytes, dtype=torch.uint8, device=DEV)
        out["tail"] = _event_us(lambda: _hipk.mg_gtail_dense_apply(tail, 1.8, 1.0, r, z, work=work))
        assert torch.equal(z, ref), "the two forms of the dense step differ"
    return out


def poisson_3d_csr(n0, n1, n2, device):
    """7-point Dirichlet Laplacian on an n0 x n1 x n2 box, row (i0 n1 + i1) n2 + i2: diagonal 6, neighbours -1, sorted rows."""
    idx = torch.arange(n0 * n1 * n2, device=device).reshape(n0, n1, n2)
    rows, cols = [idx.reshape(-1)], [idx.reshape(-1)]
    for d in range(3):
        lo, hi = idx.narrow(d, 0, idx.shape[d] - 1).reshape(-1), idx.narrow(d, 1, idx.shape[d] - 1).reshape(-1)
        rows += [lo, hi]
        cols += [hi, lo]
    r, c = torch.cat(rows), torch.cat(cols)
    v = torch.where(r == c, 6.0, -1.0).to(torch.float64)
    n = n0 * n1 * n2
    return torch.sparse_coo_tensor(torch.stack([r, c]), v, (n, n)).coalesce().to_sparse_csr()


def systems():
    from pytorch_sparse_solver.utils.matrix_utils import create_poisson_2d_csr, create_variable_diffusion_2d_csr
    return {
        "poisson1000": (lambda: create_poisson_2d_csr(1000, 1000, device=DEV), (1000, 1000)),
        "poisson2000": (lambda: create_poisson_2d_csr(2000, 2000, device=DEV), (2000, 2000)),
        "poisson4000": (lambda: create_poisson_2d_csr(4000, 4000, device=DEV), (4000, 4000)),
        "vardiff2000": (lambda: create_variable_diffusion_2d_csr(2000, 2000, device=DEV), (2000, 2000)),
        "poisson3d128": (lambda: poisson_3d_csr(128, 128, 128, DEV), (128, 128, 128)),
    }


def anisotropic_2d_csr(nx, ny, eps, device):
    """5-point Dirichlet operator on an nx x ny grid, row i ny + j: coupling -1 along i, -eps along j, diagonal 2 + 2 eps."""
    idx = torch.arange(nx * ny, device=device).reshape(nx, ny)
    rows, cols, vals = [idx.reshape(-1)], [idx.reshape(-1)], [torch.full((nx * ny,), 2.0 + 2.0 * eps, dtype=torch.float64, device=device)]
    for d, w in ((0, -1.0), (1, -eps)):
        lo, hi = idx.narrow(d, 0, idx.shape[d] - 1).reshape(-1), idx.narrow(d, 1, idx.shape[d] - 1).reshape(-1)
        rows += [lo, hi]
        cols += [hi, lo]
        vals += [torch.full((2 * lo.numel(),), w, dtype=torch.float64, device=device)]
    n = nx * ny
    return torch.sparse_coo_tensor(torch.stack([torch.cat(rows), torch.cat(cols)]), torch.cat(vals), (n, n)).coalesce().to_sparse_csr()


def graph_systems():
    table = systems()
    table["aniso2000"] = (lambda: anisotropic_2d_csr(2000, 2000, 0.01, DEV), (2000, 2000))
    return table


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def _cycle_of(cfg, default):
    """(the configuration's name without a trailing `w`, its cycle)."""
    return (cfg[:-1], "W") if cfg.endswith("w") else (cfg, default)


def run_system(name, make, grid, reps, configs, applies, graph=False, cycle="V"):
    from pytorch_sparse_solver.module_a import AggregationMultigridPreconditioner, ChebyshevPreconditioner, cg, get_last_stats
    A = make()
    n = A.shape[0]
    b = torch.ones(n, dtype=torch.float64, device=DEV)
    bn = float(torch.linalg.vector_norm(b))
    row = {"system": name, "n": n, "grid": list(grid), "nnz": int(A.values().numel())}
    Ms, setup = {"plain": None}, {}
    for cfg in configs:
        if cfg == "cheb3":
            Ms[cfg], setup[cfg] = _timed(lambda: ChebyshevPreconditioner(A, degree=3))
        elif cfg.startswith("mg"):
            base, cyc = _cycle_of(cfg, cycle)
            Ms[cfg], setup[cfg] = _timed(lambda: AggregationMultigridPreconditioner(A, grid, degree=int(base[2:]), cycle=cyc))
        elif cfg.startswith("gmg"):
            base, cyc = _cycle_of(cfg, cycle)
            degree, _, cut = base[3:].partition("c")
            try:
                Ms[cfg], setup[cfg] = _timed(lambda: AggregationMultigridPreconditioner.from_graph(A, degree=int(degree), cycle=cyc,
                                                                                                     coarse_rows=int(cut) if cut else None))
            except ValueError as e:                       # the 48-level stall: recorded, the other configurations go on
                row[cfg] = {"refused": str(e)}
    configs = [c for c in configs if c == "plain" or c in Ms]
    if graph and not any(c.startswith("gmg") for c in configs):
        applies = 0                                       # no graph hierarchy to time
    row["setup_ms"] = {k: round(1e3 * v, 1) for k, v in setup.items()}
    mg = next((Ms[c] for c in configs if c.startswith("mg")), None)
    if mg is not None:
        row["levels"] = [lev.n for lev in mg.levels]
        row["tail_from"], row["launches_per_apply"] = mg.tail_from, mg.launches_per_apply
    gmg = next((Ms[c] for c in configs if c.startswith("gmg")), None)
    if gmg is not None:
        row["graph_levels"] = [lev.n for lev in gmg.levels]
        row["graph_tail_from"], row["graph_launches_per_apply"] = gmg.tail_from, gmg.launches_per_apply
        row["graph_handshake_rounds_max"] = max(max(r) for r in gmg.handshake_rounds)
        row["graph_longest_row"] = max(lev.max_row for lev in gmg.levels)
    row["hierarchy"] = {}
    for cfg in configs:
        M = Ms[cfg]
        if cfg.startswith("mg"):
            row["hierarchy"][cfg] = {"levels": len(M.levels), "cycle": M.cycle, "launches": M.launches_per_apply, "tail_from": M.tail_from}
        if cfg.startswith("gmg"):
            row["hierarchy"][cfg] = {"levels": len(M.levels), "last": M.levels[-1].n, "cycle": M.cycle, "launches": M.launches_per_apply,
                                     "tail_from": M.tail_from,
                                     "longest_row_above_the_last": max([lev.max_row for lev in M.levels[:-1]] or [0])}
            if M.dense:
                M(b)                                       # builds the device state
                row["hierarchy"][cfg]["dense_step_us"] = dense_step_us(M._dev_state()[-1]["cinv"], M.levels[-1].n, M.levels[-1].ld)
    for cfg in configs:                                   # warm-up: code objects, allocator, the handle of A
        cg(A, b, tol=1e-6, M=Ms[cfg], maxiter=5)
    times = {cfg: [] for cfg in configs}
    for _ in range(reps):
        for cfg in configs:
            (x, info), t = _timed(lambda: cg(A, b, tol=1e-6, M=Ms[cfg]))
            st = get_last_stats()
            times[cfg].append(t)
            row[cfg] = {"iterations": st.iterations, "info": int(info), "method": st.method,
                        "relres": float(torch.linalg.vector_norm(b - A @ x)) / bn}
    for cfg in configs:
        row[cfg]["ms_min_max"] = [round(1e3 * min(times[cfg]), 2), round(1e3 * max(times[cfg]), 2)]
        row[cfg]["ms_per_iteration"] = round(1e3 * min(times[cfg]) / max(row[cfg]["iterations"], 1), 4)
        if cfg != "plain" and "plain" in configs:
            row[cfg]["time_over_plain"] = round(min(times[cfg]) / min(times["plain"]), 3)
    if applies > 0:
        v = torch.randn(n, dtype=torch.float64, device=DEV)
        row["apply_us_by_tail_rows"] = {}
        ref = None
        for tail in TAILS:
            M = AggregationMultigridPreconditioner.from_graph(A, degree=1, tail_rows=tail, cycle=cycle) if graph else \
                AggregationMultigridPreconditioner(A, grid, degree=1, tail_rows=tail, cycle=cycle)
            for _ in range(3):
                z = M(v)
            ref = z if ref is None else ref
            assert torch.equal(z, ref), "the tail kernel changed the result"
            best = float("inf")
            for _ in range(3):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(applies):
                    M(v)
                e1.record()
                torch.cuda.synchronize()
                best = min(best, 1e3 * e0.elapsed_time(e1) / applies)
            row["apply_us_by_tail_rows"][str(tail)] = {"us": round(best, 1), "tail_from": M.tail_from, "launches": M.launches_per_apply}
            del M
    return row


REFRESH_KINDS = {"grid": lambda P, A, grid: P(A, grid), "graph": lambda P, A, grid: P.from_graph(A),
                 "graph_c2048": lambda P, A, grid: P.from_graph(A, coarse_rows=2048)}
REFRESH_SYSTEMS = ("poisson2000", "vardiff2000", "poisson3d128")
STALE_MAXITER = 500


def _rescaled(A, t):
    """D A D on A's pattern, D = diag(exp(1.5 sin(2 pi (3 i / n + t)))): the coefficients of step t of the sequence (SPD with A)."""
    import math
    n = A.shape[0]
    crow, col = A.crow_indices(), A.col_indices()
    d = torch.exp(1.5 * torch.sin(2.0 * math.pi * (3.0 * torch.arange(n, device=A.device, dtype=torch.float64) / n + t)))
    rows = torch.repeat_interleave(torch.arange(n, device=A.device), crow[1:] - crow[:-1])
    return torch.sparse_csr_tensor(crow, col, A.values() * d[rows] * d[col], size=A.shape)


def _update_split(P, M, A):
    """One `update` with a synchronised clock around its steps: ms of the Galerkin sums, the level scans (with the read-back and
    the coefficients), the dense inverse (with its copies), the handles and descriptors, and the norm estimate."""
    spent, saved = {}, {}

    def clocked(name):
        fn = getattr(P, name)
        saved[name] = fn

        def wrapper(*a, **kw):
            out, t = _timed(lambda: fn(*a, **kw))
            spent[name] = spent.get(name, 0.0) + t
            return out
        setattr(P, name, wrapper)

    for name in ("_segment_sum", "_scan_levels", "_invert_dense", "_dev_state", "_estimate_scale"):
        clocked(name)
    try:
        _, total = _timed(lambda: M.update(A))
    finally:
        for name, fn in saved.items():
            setattr(P, name, fn)
    g = lambda k: spent.get(k, 0.0)
    ms = lambda v: round(1e3 * v, 2)
    return {"total": ms(total), "galerkin_sums": ms(g("_segment_sum")), "scans": ms(g("_scan_levels") - g("_invert_dense")),
            "dense_inverse": ms(g("_invert_dense")), "handles": ms(g("_dev_state")), "norm_estimate": ms(g("_estimate_scale") - g("_dev_state"))}


def run_refresh(name, make, grid, kind):
    """Set-up against re-setup for one system and one kind of hierarchy, then ten steps of changing coefficients three ways."""
    from pytorch_sparse_solver.module_a import AggregationMultigridPreconditioner as P, cg, get_last_stats
    A = make()
    n = A.shape[0]
    b = torch.ones(n, dtype=torch.float64, device=DEV)
    build = lambda X: REFRESH_KINDS[kind](P, X, grid)
    try:
        build(A)                                              # warm-up: code objects, allocator
    except ValueError as e:                                   # the 48-level stall of a graph hierarchy without a cut
        return {"system": name, "kind": kind, "n": n, "refused": str(e)}
    M, fresh = _timed(lambda: build(A))
    row = {"system": name, "kind": kind, "n": n, "levels": [lev.n for lev in M.levels], "tail_from": M.tail_from,
           "fresh_build_ms": round(1e3 * fresh, 1)}
    steps = [_rescaled(A, 0.05 * (k + 1)) for k in range(10)]
    _, first = _timed(lambda: M.update(steps[0]))
    later = [_timed(lambda: M.update(steps[1 + k % 2]))[1] for k in range(5)]
    row.update(first_update_ms=round(1e3 * first, 1), later_update_ms_mean=round(1e3 * sum(later) / len(later), 1),
               later_update_ms_min_max=[round(1e3 * min(later), 1), round(1e3 * max(later), 1)], refresh_plan_bytes=M.refresh_plan_bytes,
               later_update_split_ms=_update_split(P, M, steps[0]))
    stale = build(A)
    M.update(A)
    ways = {"rebuild": [], "update": [], "stale": []}
    for Ak in steps:
        for way in ways:
            def step():
                Mk = build(Ak) if way == "rebuild" else M.update(Ak) if way == "update" else stale
                return cg(Ak, b, tol=1e-6, M=Mk, maxiter=STALE_MAXITER if way == "stale" else None)
            (x, info), t = _timed(step)
            ways[way].append((t, get_last_stats().iterations, int(info)))
    row["ten_steps"] = {way: {"ms_total": round(1e3 * sum(v[0] for v in r), 1), "iterations": [v[1] for v in r],
                              "not_converged": sum(v[2] != 0 for v in r)} for way, r in ways.items()}
    row["ten_steps"]["stale"]["maxiter"] = STALE_MAXITER
    return row


def main_refresh(a):
    from pytorch_sparse_solver import _hipk
    out = open(a.out or os.path.join(ROOT, "profiles", "mg_refresh_probe.txt"), "w")

    def emit(obj):
        line = json.dumps(obj)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    emit({"hipk_build_id": _hipk.lib().hipk_build_id().decode(), "device": torch.cuda.get_device_name(0), "mode": "refresh",
          "dtype": "float64", "tol": 1e-6, "sequence": "D A D, D = diag(exp(1.5 sin(2 pi (3 i / n + t)))), t = 0.05 .. 0.5"})
    table = systems()
    for name in a.systems or REFRESH_SYSTEMS:
        make, grid = table[name]
        for kind in a.configs or list(REFRESH_KINDS):
            emit(run_refresh(name, make, grid, kind))
            _hipk.clear_cache()
            torch.cuda.empty_cache()
    out.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--refresh", action="store_true", help="update() against a fresh construction: set-up times, their split, ten steps")
    ap.add_argument("--out", default=None, help="the file the lines also go to (--refresh: profiles/mg_refresh_probe.txt unless given)")
    ap.add_argument("--cycle", choices=["V", "W"], default="V", help="the cycle of every multigrid configuration whose name does not end in w")
    ap.add_argument("--systems", nargs="*", default=None)
    ap.add_argument("--configs", nargs="*", default=None, help="default: plain cheb3 mg1 mg2; with --graph: plain mg1 gmg1 gmg2 gmg1c256 gmg1c512 gmg1c1024 gmg1c2048; "
                    "a trailing w (mg1w, gmg1c2048w): the W-cycle of that configuration")
    ap.add_argument("--graph", action="store_true", help="from_graph beside the grid class; the tail_rows sweep on the graph hierarchy")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--applies", type=int, default=20)
    a = ap.parse_args()
    if a.refresh:
        return main_refresh(a)
    a.configs = a.configs or (["plain", "mg1", "gmg1", "gmg2"] + [f"gmg1c{k}" for k in CUTS] if a.graph else ["plain", "cheb3", "mg1", "mg2"])
    from pytorch_sparse_solver import _hipk
    from pytorch_sparse_solver.module_a import multigrid
    out = open(a.out, "w") if a.out else None

    def emit(obj):
        line = json.dumps(obj)
        print(line, flush=True)
        if out is not None:
            out.write(line + "\n")
            out.flush()

    emit({"hipk_build_id": _hipk.lib().hipk_build_id().decode(), "device": torch.cuda.get_device_name(0), "reps": a.reps,
          "applies": a.applies, "tol": 1e-6, "dtype": "float64", "MG_TAIL_MAX_ROWS": multigrid.MG_TAIL_MAX_ROWS,
          "mode": "graph" if a.graph else "grid", "cycle": a.cycle, "configs": a.configs})
    table = graph_systems() if a.graph else systems()
    for name in a.systems or list(table):
        make, grid = table[name]
        try:
            row = run_system(name, make, grid, a.reps, a.configs, a.applies, graph=a.graph, cycle=a.cycle)
        except torch.cuda.OutOfMemoryError as e:
            row = {"system": name, "skipped": f"does not fit: {str(e).splitlines()[0]}"}
        emit(row)
        _hipk.clear_cache()
        torch.cuda.empty_cache()
    if a.graph and a.systems is None:                     # the dense step alone on random matrices, both forms
        steps = []
        for n in CUTS:
            ld = (n + 3) & ~3
            steps.append(dense_step_us(torch.randn(n * ld, dtype=torch.float64, device=DEV), n, ld))
        emit({"dense_step_us_random_fp64": steps})


if __name__ == "__main__":
    main()
