"""The case table of cg_batch / bicgstab_batch with a BatchedBlockJacobiPreconditioner (tests/test_bj_batch_cases.py checks it on
the CPU oracle and mirror, tests/test_gpu_bj_batch.py runs every case through hipk_cg_bjbatch_kernel / hipk_bi_bjbatch_kernel).

A case is a case of tests/_batch_cases.py (its generators build the systems) plus the block size `bs`; `identity`: binv is given
as identity blocks, so M is the identity (the breakdown fixtures).  The reference per system is orc_pcg_blockjacobi (cg) or the
mirror of tests/_bj_mirror.py (bicgstab), with the blocks the preconditioner holds.

Shapes: the smallest at which a block straddles what the kernel partitions by -- thread ownership (VEC = 2 and 4), the 256-row
tile (n = 257, bs = 3: block 85 holds rows 255 .. 257), the 2048-element chunk (n = 2049, bs = 3: block 682 holds rows 2046 ..
2048) -- a ragged last block, n < bs, bs = 1 and bs = 32, and n = 4096 (the largest binv)."""
from dataclasses import dataclass, field

import numpy as np

import _batch_cases as BC
import _bj_mirror as MI

# fp32 BiCGStab stagnates above 1e-5 on several of these systems (breakdown -11, info -1 on the mirror), as on the pattern cases of
# tests/_batch_cases.py (PATTERN_TOL32); at 1e-4 every system that is not stopped by maxiter and does not break down ends with info 0
# (tests/test_bj_batch_cases.py asserts it)
TOL = {("cg", "f64"): 1e-8, ("cg", "f32"): 1e-5, ("bicgstab", "f64"): 1e-8, ("bicgstab", "f32"): 1e-4}


@dataclass
class Case:
    id: str
    solver: str
    dtype: str
    bs: int
    grid: tuple = None
    dense: str = None
    pattern: tuple = None
    transform: str = None
    S: int = 4
    x0: str = "none"
    kwargs: dict = field(default_factory=dict)
    env: dict = field(default_factory=dict)
    zero_b: int = None
    identity: bool = False

    @property
    def path(self):
        return "hipk_%s_bjbatch_kernel<%s>" % ("cg" if self.solver == "cg" else "bi", "double" if self.dtype == "f64" else "float")

    @property
    def solve_kwargs(self):
        kw = {"tol": TOL[(self.solver, self.dtype)]}
        kw.update(self.kwargs)
        return kw

    @property
    def base(self):
        """The case of tests/_batch_cases.py whose generator builds the systems (seeded by this case's id)."""
        return BC.Case(id=self.id, solver=self.solver, dtype=self.dtype, pre=False, grid=self.grid, dense=self.dense,
                       pattern=self.pattern, transform=self.transform, S=self.S, x0=self.x0, kwargs=self.kwargs, zero_b=self.zero_b)


def _c(solver, dtype, bs, grid, S=4, x0="none", tag="", **kw):
    return Case(id=f"{solver}-bj{bs}-{dtype}-{grid[0]}x{grid[1]}-S{S}-x0{x0}{tag}", solver=solver, dtype=dtype, bs=bs, grid=grid, S=S,
                x0=x0, **kw)


def _d(solver, dtype, bs, dense, S=2, **kw):
    return Case(id=f"{solver}-bj{bs}-{dtype}-{dense}", solver=solver, dtype=dtype, bs=bs, dense=dense, S=S, **kw)


CASES = [
    # ---- 7 x 5 (n = 35): a ragged last block (bs = 4: 3 rows; bs = 3: 2 rows), bs = 1, S = 1, 2, 5 and 1030
    _c("cg", "f64", 4, (7, 5)), _c("cg", "f32", 3, (7, 5), S=5, x0="random"), _c("cg", "f64", 1, (7, 5), S=1),
    _c("cg", "f64", 4, (7, 5), S=1030, x0="random"),                       # more workgroups than are resident
    _c("bicgstab", "f64", 4, (7, 5), S=5, x0="random"), _c("bicgstab", "f32", 1, (7, 5), S=2), _c("bicgstab", "f64", 3, (7, 5), S=1),
    # ---- n = 77 with bs = 32 (blocks of 32, 32, 13 rows)
    _c("cg", "f32", 32, (11, 7)), _c("bicgstab", "f64", 32, (11, 7), x0="exact"),
    # ---- 257 x 1, bs = 3: a block across the 256-row tile edge and across thread ownership in both VECs
    _c("cg", "f64", 3, (257, 1), x0="exact"), _c("cg", "f32", 3, (257, 1)), _c("bicgstab", "f64", 3, (257, 1)),
    _c("bicgstab", "f32", 3, (257, 1), x0="random"),
    # ---- 32 x 32, bs = 4 at S = 300; exits by maxiter, atol and b = 0
    _c("bicgstab", "f64", 4, (32, 32), S=300, x0="random"), _c("cg", "f32", 4, (32, 32), x0="random"),
    _c("cg", "f64", 4, (32, 32), x0="exact", tag="-maxiter5", kwargs={"maxiter": 5}),
    _c("bicgstab", "f64", 4, (32, 32), tag="-maxiter5", kwargs={"maxiter": 5}),
    _c("cg", "f64", 4, (17, 15), tag="-atol", kwargs={"atol": 1e-2}), _c("bicgstab", "f64", 8, (17, 15), tag="-atol", kwargs={"atol": 1e-2}),
    _c("cg", "f64", 8, (16, 16), S=5, tag="-b0", zero_b=2), _c("bicgstab", "f32", 4, (16, 16), S=5, tag="-b0", zero_b=0),
    # ---- 64 x 64 (n = 4096): bs = 32 (the largest binv) and bs = 7 (ragged: 4096 = 585 * 7 + 1)
    _c("cg", "f64", 32, (64, 64)), _c("bicgstab", "f64", 7, (64, 64), x0="random"), _c("cg", "f32", 7, (64, 64), S=2),
    _c("bicgstab", "f32", 32, (64, 64), S=2),
    # ---- rag31, n = 2049, bs = 3: a block across the 2048-element chunk edge; rows unsorted, a column stored twice
    Case(id="cg-bj3-f64-rag31n2049-dup_shuf", solver="cg", dtype="f64", bs=3, pattern=("rag31", 2049), transform="dup_shuf"),
    Case(id="bicgstab-bj3-f64-rag31n2049-dup_diag", solver="bicgstab", dtype="f64", bs=3, pattern=("rag31", 2049), transform="dup_diag",
         x0="random"),
    Case(id="cg-bj3-f32-rag31n2049-shuf", solver="cg", dtype="f32", bs=3, pattern=("rag31", 2049), transform="shuf", S=2),
    # ---- dense patterns: n = 1 with bs = 1 and bs = 4, n = 3 with bs = 32 (n < bs)
    _d("cg", "f64", 1, "spd1"), _d("bicgstab", "f64", 4, "spd1"), _d("cg", "f32", 4, "spd1"),
    _d("cg", "f64", 32, "spd3"), _d("bicgstab", "f32", 32, "spd3"),
    # ---- the breakdown fixtures with M = identity (identity binv), next to a partner that converges
    _d("bicgstab", "f64", 2, "bd-10", identity=True), _d("bicgstab", "f64", 2, "bd-11", identity=True),
]
BY_ID = {c.id: c for c in CASES}
# the cases that also run with HIPK_BATCH_LAUNCH_ITS = 7 and = 1: every instantiation's save / resume path, more than one launch each
BUDGET_IDS = ["cg-bj4-f64-7x5-S4-x0none", "cg-bj3-f32-7x5-S5-x0random", "cg-bj3-f32-257x1-S4-x0none", "cg-bj32-f64-64x64-S4-x0none",
              "bicgstab-bj4-f64-7x5-S5-x0random", "bicgstab-bj4-f32-16x16-S5-x0none-b0", "bicgstab-bj32-f64-11x7-S4-x0exact",
              "bicgstab-bj3-f64-rag31n2049-dup_diag"]


def build(case):
    return BC.build(case.base)


def identity_binv(S, n, bs, dt):
    nb = (n + bs - 1) // bs
    return np.ascontiguousarray(np.broadcast_to(np.eye(bs, dtype=dt), (S, nb, bs, bs)))


def cpu_binv(case, data):
    """(S, nb, bs, bs): the blocks BatchedBlockJacobiPreconditioner holds for CPU tensors (identity cases: identity blocks)."""
    import torch
    from pytorch_sparse_solver.module_a import BatchedBlockJacobiPreconditioner, BatchedCSR
    if case.identity:
        return identity_binv(case.S, data["n"], case.bs, data["vals"].dtype)
    A = BatchedCSR(torch.from_numpy(data["crow"]), torch.from_numpy(data["col"]), torch.from_numpy(data["vals"]))
    return BatchedBlockJacobiPreconditioner(A, block_size=case.bs).binv.numpy()


def oracle_run(case, data, O, binv):
    """The reference per system (a list of OracleResult) with the blocks binv (S, nb, bs, bs)."""
    fn = MI.pcg_blockjacobi if case.solver == "cg" else MI.bicgstab_block
    out = []
    for s in range(case.S):
        x0 = None if data["X0"] is None else data["X0"][s]
        out.append(fn(O, data["crow"], data["col"], data["vals"][s], binv[s], data["B"][s], x0, dtype=data["vals"].dtype,
                      **case.solve_kwargs))
    return out


_cache = {}


def reference(case, O):
    """build + cpu_binv + oracle_run once per case and process (shared by the tests; never modified)."""
    if case.id not in _cache:
        data = build(case)
        binv = cpu_binv(case, data)
        _cache[case.id] = (data, binv, oracle_run(case, data, O, binv))
    return _cache[case.id]
