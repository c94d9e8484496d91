#!/usr/bin/env python3
"""hipk_csr_update_values against hipk_csr_create on the same arrays, in one process on one MI355X.

Per system: 10 alternating repetitions create / update (the update gives the handle of the repetition before the other of two value
sets of the same form, so it always has work to do); each as wall clock (device synchronised before and after) and by HIP events
around the call, min / median / max in ms; the update's kind and its host synchronisations.

Systems: Poisson 2000^2 (pair-coded; fp64 and fp32), variable diffusion 2000^2 (offset-coded), a general CSR matrix of the same nnz
(5 random columns per row: plain), Poisson 64^2, and the first two coarse levels of the grid hierarchy of Poisson 2000^2 (1000^2 and
500^2 unknowns, 9-point).  For the offset-coded system the two forms of the value-plane rewrite (hipk_csr_revalue_probe: 1 one row
per lane, 2 staged through LDS) are timed by events over 20 launches each, alternating.

  python tools/handle_update_probe.py            # lines also go to profiles/handle_update_probe.txt (--out)
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytorch-sparse-linalg-torch-amgx.cg.bicg.gmres_amd"))

import torch  # noqa: E402

from pytorch_sparse_solver import _hipk  # noqa: E402
from pytorch_sparse_solver.utils.matrix_utils import create_poisson_2d_csr, create_variable_diffusion_2d_csr  # noqa: E402

DEV = "cuda:0"
REPS = 10


def _mmm(v):
    return [round(min(v), 3), round(statistics.median(v), 3), round(max(v), 3)]


def _timed(fn):
    """(result, wall ms, event ms) of fn(), the device idle before and after."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return out, 1e3 * (time.perf_counter() - t0), e0.elapsed_time(e1)


def _systems():
    def csr(A, dtype=torch.float64):
        return A.crow_indices(), A.col_indices(), A.values().to(dtype), tuple(A.shape)

    def poisson(nx, dtype=torch.float64):
        crow, col, val, shape = csr(create_poisson_2d_csr(nx, nx, device=DEV), dtype)
        return crow, col, val, val * 2, shape

    def vardiff(nx):
        crow, col, val, shape = csr(create_variable_diffusion_2d_csr(nx, nx, seed=1, device=DEV))
        return crow, col, val, create_variable_diffusion_2d_csr(nx, nx, seed=2, device=DEV).values(), shape

    def general(n, per_row):
        g = torch.Generator(device=DEV).manual_seed(3)
        col = torch.sort(torch.randint(0, n, (n, per_row), device=DEV, generator=g), dim=1)[0].reshape(-1)
        crow = torch.arange(n + 1, device=DEV) * per_row
        val = torch.randn(n * per_row, dtype=torch.float64, device=DEV, generator=g)
        return crow, col, val, val * 2, (n, n)

    def coarse(level):
        from pytorch_sparse_solver.module_a import AggregationMultigridPreconditioner as P
        M = P(create_poisson_2d_csr(2000, 2000, device=DEV), (2000, 2000), normalize=False)
        c = M.levels[level].csr
        crow, col, val = c.crow_indices().clone(), c.col_indices().clone(), c.values().clone()
        return crow, col, val, val * 2, tuple(c.shape)

    return [("poisson2000 fp64", lambda: poisson(2000)), ("poisson2000 fp32", lambda: poisson(2000, torch.float32)),
            ("vardiff2000 fp64", lambda: vardiff(2000)), ("general_csr 4M x 5 fp64", lambda: general(4_000_000, 5)),
            ("poisson64 fp64", lambda: poisson(64)), ("coarse level 1 of poisson2000 fp64", lambda: coarse(1)),
            ("coarse level 2 of poisson2000 fp64", lambda: coarse(2))]


def run(name, make):
    crow, col, v0, v1, shape = make()
    vals = (v0, v1)
    _hipk.CsrHandle(crow, col, v0, shape).close()            # warm-up: code objects
    h = _hipk.CsrHandle(crow, col, v0, shape)
    cw, ce, uw, ue, kinds, syncs = [], [], [], [], set(), set()
    for rep in range(REPS):
        f, w, e = _timed(lambda: _hipk.CsrHandle(crow, col, vals[rep % 2], shape))
        cw.append(w)
        ce.append(e)
        f.close()
        _, w, e = _timed(lambda: h.update_values(vals[(rep + 1) % 2]))
        uw.append(w)
        ue.append(e)
        kinds.add(_hipk.CsrHandle.last_update_kind())
        syncs.add(int(_hipk.lib().hipk_last_csr_update_syncs()))
    row = {"system": name, "n": shape[0], "nnz": int(v0.numel()), "path": h.path(), "create_wall_ms": _mmm(cw), "create_event_ms": _mmm(ce),
           "update_wall_ms": _mmm(uw), "update_event_ms": _mmm(ue), "update_kind": sorted(kinds), "update_host_syncs": sorted(syncs),
           "create_over_update_wall_median": round(statistics.median(cw) / statistics.median(uw), 2)}
    if h.path() == "offset_coded":
        L, stream = _hipk.lib(), torch.cuda.current_stream().cuda_stream
        forms = {1: [], 2: []}
        for _ in range(20):
            for form in (1, 2):
                _, _, e = _timed(lambda: _hipk._check(L.hipk_csr_revalue_probe(h._h, form, stream), "hipk_csr_revalue_probe"))
                forms[form].append(e)
        planes = h.format_bytes() - 2 * shape[0] * v0.element_size()
        row["revalue_rows_event_ms"], row["revalue_staged_event_ms"] = _mmm(forms[1]), _mmm(forms[2])
        row["revalue_bytes"] = int(v0.numel() * v0.element_size() * 2 + 4 * shape[0])
        row["planes_bytes"] = int(planes)
    h.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "handle_update_probe.txt"))
    ap.add_argument("--systems", nargs="*", default=None, help="substrings of the system names to run (default: all)")
    a = ap.parse_args()
    out = open(a.out, "w")

    def emit(obj):
        line = json.dumps(obj)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    emit({"hipk_build_id": _hipk.lib().hipk_build_id().decode(), "device": torch.cuda.get_device_name(0), "reps": REPS,
          "times": "min / median / max in ms"})
    for name, make in _systems():
        if a.systems and not any(s in name for s in a.systems):
            continue
        emit(run(name, make))
        torch.cuda.empty_cache()
    out.close()


if __name__ == "__main__":
    main()
