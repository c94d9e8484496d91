"""Shared by tests/test_gpu_spmv_instantiations.py and run by it as a child process: the references of one (matrix, storage type)
of tests/_spmv_cases.py, and the run of one case -- switches, THEN the handle, hipk_spmv_ex per mode, the kernel note read right
after the call, every output compared bit for bit with the oracle.  y lies in a guarded arena of exactly n elements
(tests/_arena.py) and, for hipk_spmv_dot, the scratch in one of exactly hipk_scratch_bytes() filled with 0xFF: the guards are
checked after every launch.

As a program: python _spmv_inst_worker.py GROUP OUT.json CASE...  runs the cases of one fresh-process group (switches that
hipk_launch_spmv reads once per process) in this process and writes {case: {"notes": [...], "failures": [...]}}.  GROUP
"order:NAME" takes the cases from tests/_order_cases.py (tests/test_gpu_entry_order.py: unsorted and duplicate rows) instead."""
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "pytorch-sparse-linalg-torch-amgx.cg.bicg.gmres_amd"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import _spmv_cases as C  # noqa: E402

DEV = "cuda:0"


def _bits(a):
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def differs(z, ref, unit=256, what="rows", group="tiles"):
    """None if z has the reference's bits, else where it does not: count, first positions, their tiles."""
    bad = np.flatnonzero(_bits(z) != _bits(ref))
    if bad.size == 0:
        return None
    n = ref.size
    where = f" ({group} {(bad[:8] // unit).tolist()} of {(n + unit - 1) // unit}, the last has {n - (n - 1) // unit * unit} {what})" if unit else ""
    return (f"{bad.size} of {n} {what} differ; first {bad[:8].tolist()}{where}, last {int(bad[-1])}; got {z[bad[:3]].tolist()} "
            f"oracle {ref[bad[:3]].tolist()}")


class References:
    """x, w, b and the oracle's outputs for one matrix in one storage type: y = A x and b - A x, and per reduction chunk of `ch`
    rows the fused dots <w, y>, <x, A x> (w is x) and <y, y>."""

    def __init__(self, oracle, name, dtype, ch, arrays=None, vectors=None):
        """arrays, vectors: (crow, col, val) and (x, w, b) of a matrix that is not one of tests/_spmv_cases.py: MATRICES."""
        self.name, self.dtype, self.ch = name, dtype, ch
        self.f = np.float64 if dtype == C.DOUBLE else np.float32
        self.crow, self.col, val = C.matrix(name) if arrays is None else arrays
        self.val = val.astype(self.f)
        self.n = len(self.crow) - 1
        self.x, self.w, self.b = C.vectors(name, dtype) if vectors is None else vectors
        spmv = oracle.spmv if dtype == C.DOUBLE else oracle.spmv32
        oracle.set_threads(16)
        try:
            self.y = {False: spmv(self.crow, self.col, self.val, self.x), True: spmv(self.crow, self.col, self.val, self.x, bsub=self.b)}
            # part0[(residual form, w is x)], part1[residual form]
            self.part0 = {(r, wx): self._dot(oracle, self.x if wx else self.w, self.y[r]) for r, wx in ((False, False), (True, False), (False, True))}
            self.part1 = {r: self._dot(oracle, self.y[r], self.y[r]) for r in (False, True)}
        finally:
            oracle.set_threads(1)

    def _dot(self, oracle, a, b):
        if self.dtype == C.DOUBLE:
            return oracle.dot_tiled_parts_ch(a, b, self.ch)
        g = (self.n + self.ch - 1) // self.ch
        return np.array([oracle.dot_tiled32(a[c * self.ch:(c + 1) * self.ch], b[c * self.ch:(c + 1) * self.ch]) for c in range(g)])

    def check_against_high_precision(self):
        """The oracle ports the kernels' summation order; here its outputs are held against products and sums in np.longdouble.
        Derived bounds, u = 2^-53 (2^-24 for fp32 storage): a row of k entries  |y - y_ld| <= (k + 2) u (sum |a_ij x_j| + |b_i|),
        a chunk of m rows  |part - sum_ld| <= (m + 2) u sum |w_i y_i|.  Returns the largest error / bound met."""
        Ld = np.longdouble
        assert np.finfo(Ld).nmant > 60
        u = 2.0 ** -53 if self.dtype == C.DOUBLE else 2.0 ** -24
        lens = np.diff(self.crow)
        worst = 0.0
        step = 1 << 18
        for r0 in range(0, self.n, step):
            r1 = min(self.n, r0 + step)
            e0, e1 = int(self.crow[r0]), int(self.crow[r1])
            k = lens[r0:r1]
            s, a = np.zeros(r1 - r0, Ld), np.zeros(r1 - r0, Ld)
            if e1 > e0:
                p = self.val[e0:e1].astype(Ld) * self.x[self.col[e0:e1]].astype(Ld)
                idx = np.minimum(self.crow[r0:r1] - e0, e1 - e0 - 1)
                s, a = np.add.reduceat(p, idx), np.add.reduceat(np.abs(p), idx)
                s[k == 0], a[k == 0] = 0, 0
            for resid in (False, True):
                b = self.b[r0:r1].astype(Ld)
                y_ld = b - s if resid else s
                bound = (k + 2) * Ld(u) * (a + (np.abs(b) if resid else 0))
                err = np.abs(self.y[resid][r0:r1].astype(Ld) - y_ld)
                bad = np.flatnonzero(err > bound)
                assert bad.size == 0, f"{self.name} {self.dtype} resid={resid}: oracle rows {(r0 + bad[:5]).tolist()} beyond the bound"
                worst = max(worst, float(np.max(err / np.where(bound > 0, bound, 1))))
        starts = np.arange(0, self.n, self.ch)
        m = np.minimum(self.ch, self.n - starts)
        for parts, a, b in ([(self.part0[key], self.x if key[1] else self.w, self.y[key[0]]) for key in self.part0] +
                            [(self.part1[r], self.y[r], self.y[r]) for r in self.part1]):
            p = a.astype(Ld) * b.astype(Ld)
            s_ld, abs_ld = np.add.reduceat(p, starts), np.add.reduceat(np.abs(p), starts)
            bound = (m + 2) * Ld(u) * abs_ld
            err = np.abs(parts.astype(Ld) - s_ld)
            bad = np.flatnonzero(err > bound)
            assert bad.size == 0, f"{self.name} {self.dtype}: oracle chunk partials {bad[:5].tolist()} beyond the bound"
            worst = max(worst, float(np.max(err / np.where(bound > 0, bound, 1))))
        return worst


class OnDevice:
    """The device copies of one References, and clones to see that a launch left its inputs alone."""

    def __init__(self, ref):
        import torch
        to = lambda a: torch.from_numpy(a).to(DEV)   # noqa: E731
        self.crow, self.col, self.val = to(ref.crow), to(ref.col), to(ref.val)
        self.crow32, self.col32 = None, None         # int32 copies, made when a case asks for them (idx_bytes 4)
        self.x, self.w, self.b = to(ref.x), to(ref.w), to(ref.b)
        self.x0, self.w0, self.b0 = self.x.clone(), self.w.clone(), self.b.clone()
        self.y_arena, self.scratch_arena = None, None   # made by the first launch, kept for the matrix

    def arenas(self, scratch_bytes):
        from _arena import Arena, guard_bytes_for
        if self.y_arena is None:
            n, item = self.x.numel(), self.x.element_size()
            self.y_arena = Arena(DEV, n * item, 16, guard_bytes_for(n, item))
            self.scratch_arena = Arena(DEV, scratch_bytes, 256, guard_bytes_for(n, item))
        return self.y_arena, self.scratch_arena

    def unchanged(self):
        import torch
        return torch.equal(self.x, self.x0) and torch.equal(self.w, self.w0) and torch.equal(self.b, self.b0)


def _launch(hipk, h, ref, dev, mode, wx):
    import torch
    L = hipk.lib()
    n, G = ref.n, int(L.hipk_chunk_count(ref.n))
    ya, _ = dev.arenas(int(L.hipk_scratch_bytes()))
    y = ya.view(dev.x.dtype, n)
    y.fill_(float("nan"))
    p0 = torch.full((G,), float("nan"), dtype=torch.float64, device=DEV)
    p1 = torch.full((G,), float("nan"), dtype=torch.float64, device=DEV)
    w = dev.x if wx else dev.w
    hipk._check(L.hipk_spmv_ex(h._h, dev.x.data_ptr(), y.data_ptr(), mode, w.data_ptr(), dev.b.data_ptr(), p0.data_ptr(), p1.data_ptr(),
                               None, 0, torch.cuda.current_stream().cuda_stream), "hipk_spmv_ex")
    note = hipk.CsrHandle.last_spmv_kernel()
    return note, y.cpu().numpy(), p0.cpu().numpy(), p1.cpu().numpy(), ya.guards_intact() or ya.touched()


def _launch_dot(hipk, h, ref, dev):
    """hipk_spmv_dot (y = A x with <w, y>): y and the scratch in guarded arenas, the scratch filled with 0xFF."""
    import torch
    L = hipk.lib()
    ya, sa = dev.arenas(int(L.hipk_scratch_bytes()))
    y = ya.view(dev.x.dtype, ref.n)
    y.fill_(float("nan"))
    sa.fill(0xFF)
    out = torch.full((1,), float("nan"), dtype=torch.float64, device=DEV)
    hipk._check(L.hipk_spmv_dot(h._h, dev.x.data_ptr(), y.data_ptr(), dev.w.data_ptr(), out.data_ptr(), sa.data_ptr(),
                                torch.cuda.current_stream().cuda_stream), "hipk_spmv_dot")
    note = hipk.CsrHandle.last_spmv_kernel()
    return note, y.cpu().numpy(), float(out.cpu()), [a.guards_intact() or a.touched() for a in (ya, sa)]


def run_case(hipk, name, ref, dev, setenv, case=None):
    """Run one case of the table (`case`: a row of another table in the same layout; "idx32": crow / col as int32 tensors).
    setenv(name, value or None) changes the environment (the caller restores it).
    Returns (notes, failures): [step, mode, w is x, note] per launch, and every mismatch found -- none stops the run."""
    import torch
    if case is None:
        case = C.CASES[name]
        assert (case["matrix"], case["dtype"]) == (ref.name, ref.dtype)
    assert case["dtype"] == ref.dtype
    assert int(hipk.lib().hipk_chunk_size(ref.n)) == ref.ch
    notes, failures, outs = [], [], {}
    for k, v in case["env"].items():
        setenv(k, v)
    crow, col = dev.crow, dev.col
    if case.get("idx32"):
        if dev.crow32 is None:
            dev.crow32, dev.col32 = dev.crow.to(torch.int32), dev.col.to(torch.int32)
        crow, col = dev.crow32, dev.col32
    h = hipk.CsrHandle(crow, col, dev.val, (ref.n, ref.n))     # after the switches: the handle caches its kernel choice
    try:
        if case["plain_only"]:
            h.set_path(plain_only=True)

        def check(tag, got, mode, wx, y, p0, p1):
            resid = bool(mode & 4)
            d = differs(y, ref.y[resid])
            if d is not None:
                failures.append(f"{tag} [{got}] y: {d}")
            if mode & 1:
                d = differs(p0, ref.part0[(resid, wx)], unit=0, what="chunk partials of <w, y>")
                if d is not None:
                    failures.append(f"{tag} [{got}] part0: {d}")
            if mode & 2:
                d = differs(p1, ref.part1[resid], unit=0, what="chunk partials of <y, y>")
                if d is not None:
                    failures.append(f"{tag} [{got}] part1: {d}")

        for si, (delta, want) in enumerate(case["steps"]):
            for k, v in delta.items():
                setenv(k, v)
            for mode, wx in case["runs"]:
                tag = f"{name} step {si} mode {mode}" + (" w=x" if wx else "")
                got, y, p0, p1, intact = _launch(hipk, h, ref, dev, mode, wx)
                if intact is not True:
                    failures.append(f"{tag} [{got}]: a write outside y[0..n) (first, last offset, bytes: {intact})")
                notes.append([si, mode, wx, got])
                if got != want[mode]:
                    failures.append(f"{tag}: kernel {got}, expected {want[mode]}")
                check(tag, got, mode, wx, y, p0, p1)
                outs[(mode, wx)] = (y, p0, p1)
            # hipk_spmv_dot with the step's switches: the bits of y, a finite <w, y> whatever the scratch held, no byte outside
            tag = f"{name} step {si} hipk_spmv_dot"
            got, y, dot, intact = _launch_dot(hipk, h, ref, dev)
            d = differs(y, ref.y[False])
            if d is not None:
                failures.append(f"{tag} [{got}] y: {d}")
            # <w, y> is the fp64 fold of the g chunk partials that mode 1 is pinned to bit for bit (ref.part0): g doubles summed in
            # whatever order lie within g 2^-53 sum |part| of their exact sum, in both storage types
            parts = ref.part0[(False, False)]
            want_dot = math.fsum(parts)
            bound = len(parts) * 2.0 ** -53 * math.fsum(np.abs(parts))
            if not abs(dot - want_dot) <= bound:
                failures.append(f"{tag} [{got}]: <w, y> = {dot!r}, {want_dot!r} expected within {bound:.3e}")
            for what, ok in zip(("y[0..n)", "scratch[0..hipk_scratch_bytes)"), intact):
                if ok is not True:
                    failures.append(f"{tag} [{got}]: a write outside {what} (first, last offset, bytes: {ok})")
        if case["also_plain"]:
            h.set_path(plain_only=True)
            for mode, wx in case["runs"]:
                tag = f"{name} plain CSR kernels mode {mode}" + (" w=x" if wx else "")
                got, y, p0, p1, intact = _launch(hipk, h, ref, dev, mode, wx)
                if intact is not True:
                    failures.append(f"{tag} [{got}]: a write outside y[0..n) (first, last offset, bytes: {intact})")
                if not got.startswith("hipk_spmv_kernel<"):
                    failures.append(f"{tag}: kernel {got}, expected hipk_spmv_kernel<...>")
                cy, c0, c1 = outs[(mode, wx)]
                for what, a, c, on in (("y", y, cy, True), ("part0", p0, c0, mode & 1), ("part1", p1, c1, mode & 2)):
                    if on and not np.array_equal(_bits(a), _bits(c)):
                        failures.append(f"{tag} [{got}] {what}: not the bits of the case's own kernel")
                check(tag, got, mode, wx, y, p0, p1)
    finally:
        h.close()
    if not dev.unchanged():
        failures.append(f"{name}: x, w or b changed")
    return notes, failures


def main():
    group, out, names = sys.argv[1], sys.argv[2], sys.argv[3:]
    import torch  # noqa: F401
    from oracle import oracle as O
    from pytorch_sparse_solver import _hipk as hipk
    O.build()
    hipk.lib()
    touched = {}

    def setenv(k, v):
        touched.setdefault(k, os.environ.get(k))
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v

    table = C
    if group.startswith("order:"):
        import _order_cases as table
        group = group[len("order:"):]
    results, held = {}, {}
    for name in names:
        case = table.CASES[name]
        assert case["fresh"] == group, (name, case["fresh"], group)
        key = (case["matrix"], case.get("transform"), case["dtype"])
        if key not in held:
            held.clear()
            if table is C:
                ref = References(O, key[0], key[2], int(hipk.lib().hipk_chunk_size(C.MATRICES[key[0]][0])))
            else:
                arrays = table.arrays(*key)
                ref = References(O, key[0], key[2], int(hipk.lib().hipk_chunk_size(len(arrays[0]) - 1)), arrays=arrays,
                                 vectors=table.vectors(key[0], key[2]))
            held[key] = (ref, OnDevice(ref))
        print(name, flush=True)
        notes, failures = run_case(hipk, name, *held[key], setenv, case=case)
        results[name] = {"notes": notes, "failures": failures}
        for k, v in touched.items():     # the next case sets its own switches, the group's among them
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        touched.clear()
    with open(out, "w") as f:
        json.dump(results, f)


if __name__ == "__main__":
    main()
