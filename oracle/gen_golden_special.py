#!/usr/bin/env python3
"""Generate tests/golden/special_values.json by RUNNING THE REFERENCE (imported from /root/reference/src) on the regimes of
tests/_special_cases.py: power-of-two scalings of A and b up to overflow, underflow and subnormal operands, and right-hand sides
with a NaN, an infinity or a run of zeros.

Runs only in the build container (the reference never travels to the GPU box).  The fixture is data: the two 35-row band systems
(CSR arrays and b, unscaled), and per run the exponents, the solver options and the reference's outputs -- x, info, the number of
operator applications, the NaN mask and the zero mask of x.  Floats are written as C99 hex strings so that every bit, the sign of
a zero and every non-finite value survive JSON.  Usage:  PYTHONDONTWRITEBYTECODE=1 python oracle/gen_golden_special.py

Both storage types are tried.  The reference promotes b to fp64 and then refuses an fp32 A ("expected scalar type Double but found
Float"): the refusal is recorded under "refused" instead of runs, and tests/test_special_cases.py says that the fp32 regimes have
no reference run."""
import json
import os
import sys
import warnings

import numpy as np
import torch

warnings.filterwarnings("ignore")
HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, os.path.join(REF, "src"))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
sys.dont_write_bytecode = True

from pytorch_sparse_solver.module_a import bicgstab, cg, gmres  # noqa: E402

import _special_cases as S  # noqa: E402
from _oracle_cases import _band  # noqa: E402

OUT = os.path.normpath(os.path.join(HERE, "..", "tests", "golden", "special_values.json"))
SOLVERS = {"cg": cg, "bicgstab": bicgstab, "gmres": gmres}
SYSTEMS = {"s5_n35": lambda: _band(35, (1, 2)), "n5_n35": lambda: _band(35, (1, 2), sym=False, seed=1)}
# (tag, solver, systems, options): the caps of tests/test_gpu_solve_special.py
RUNS = [("cg", "cg", ("s5_n35",), dict(tol=1e-8, maxiter=S.MAXITER_CAP)),
        ("bicgstab", "bicgstab", ("s5_n35", "n5_n35"), dict(tol=1e-8, maxiter=S.MAXITER_CAP)),
        ("gmres_batched", "gmres", ("s5_n35", "n5_n35"), dict(tol=1e-8, restart=20, maxiter=S.GMRES_CYCLE_CAP, solve_method="batched")),
        ("gmres_incremental", "gmres", ("s5_n35", "n5_n35"),
         dict(tol=1e-8, restart=20, maxiter=S.GMRES_CYCLE_CAP, solve_method="incremental"))]


class Counting:
    def __init__(self, A):
        self.A = A
        self.count = 0

    def __call__(self, v):
        self.count += 1
        return torch.matmul(self.A, v)


def hexes(a):
    return [float(v).hex() for v in np.asarray(a, dtype=np.float64)]


def main():
    torch.set_num_threads(1)
    out = {"generator": "oracle/gen_golden_special.py", "torch": torch.__version__,
           "reference": "Litianyu141/Pytorch-Sparse-Linalg-torch-amgx.cg.bicg.gmres", "systems": {}, "runs": [], "refused": {}}
    for key, make in SYSTEMS.items():
        M = make()
        b = np.random.default_rng(35).standard_normal(35)
        out["systems"][key] = {"crow": M.indptr.tolist(), "col": M.indices.tolist(), "val": hexes(M.data), "b": hexes(b)}
    for dtn in (S.F64, S.F32):
        dt, tdt = (np.float64, torch.float64) if dtn == S.F64 else (np.float32, torch.float32)
        for tag, sname, systems, kw in RUNS:
            for key in systems:
                M = SYSTEMS[key]()
                M.data = M.data.astype(dt)
                b = np.array([float.fromhex(v) for v in out["systems"][key]["b"]]).astype(dt)
                for name in ["plain"] + S.REGIME_NAMES[dtn]:
                    reg = ("plain", dtn, 0, 0, None, None) if name == "plain" else S.regime(name, dtn)
                    kind = sname                         # the golden runs are unpreconditioned
                    ea, eb = S.SOLVER_EXPONENTS.get((kind, name, dtn), (reg[2], reg[3], ""))[:2]
                    vals, bs, _, _ = S.operands(M, b, None, False, reg, ea, eb)
                    kwr = dict(kw)
                    if name == "nan-b" and sname != "gmres":
                        kwr["maxiter"] = S.NAN_MAXITER
                    A = torch.sparse_csr_tensor(torch.from_numpy(M.indptr.astype(np.int64)), torch.from_numpy(M.indices.astype(np.int64)),
                                                torch.from_numpy(vals), size=M.shape)
                    op = Counting(A)
                    try:
                        x, info = SOLVERS[sname](op, torch.from_numpy(bs), **kwr)
                    except Exception as e:    # noqa: BLE001  (a storage type the reference refuses)
                        r = out["refused"].setdefault(dtn, {"runs": 0, "errors": []})
                        r["runs"] += 1
                        if f"{type(e).__name__}: {e}"[:300] not in r["errors"]:
                            r["errors"].append(f"{type(e).__name__}: {e}"[:300])
                        continue
                    assert x.dtype == tdt, (x.dtype, tdt)
                    x = x.numpy()
                    out["runs"].append({"tag": tag, "solver": sname, "system": key, "dtype": dtn, "regime": name, "ea": ea, "eb": eb,
                                        "special": reg[4], "kwargs": kwr, "info": int(info), "matvecs": int(op.count), "x": hexes(x),
                                        "nan": np.flatnonzero(np.isnan(x)).tolist(), "zero": np.flatnonzero(x == 0).tolist()})
                    print(f"{dtn} {tag:18s} {key} {name:12s} info={int(info):2d} matvecs={op.count:3d} nan={int(np.isnan(x).sum()):2d} "
                          f"zero={int((x == 0).sum()):2d}")
    with open(OUT, "w") as f:
        json.dump(out, f, indent=0)
    print(f"wrote {len(out['runs'])} runs, {sum(v['runs'] for v in out['refused'].values())} refused, {os.path.getsize(OUT)} bytes to {OUT}")


if __name__ == "__main__":
    main()
