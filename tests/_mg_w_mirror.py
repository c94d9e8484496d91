"""Numpy mirror of `AggregationMultigridPreconditioner(cycle="W")` (module_a/multigrid.py), shared by tests/test_mg_wcycle.py and
tests/test_gpu_mg_wcycle.py.  None of it uses the class's code: the cycle is written here as a recursion of its own over the level
steps of the three existing mirrors --
  the smoother          _cheb_mirror.mirror on the oracle's SpMV (the kernels' one summation order);
  the transfers         _mg_mirror.restrict / prolong_add on a level of boxes, _mg_graph_mirror.restrict_np / prolong_add_np (the
                        vectorised forms, checked there against the scalar loops) on a level of index arrays;
  the last level        dinv * r, or _mg_dense_mirror.segmented on the stored inverse --
on the level matrices, maps and coefficients the object under test holds.

    W(l, r):  z = S(r);  t = r - A z;  rc = restrict(t)
              e = W(l + 1, rc)
              where level l + 1 is smoothed (not the last):  rc2 = rc - A_{l+1} e;  e2 = W(l + 1, rc2);  e = e + e2
              z = z + (omega * e[agg]);  t = r - A z;  z = z + S(t)

Every step is a separate rounding in the storage dtype.  `cycle="V"` leaves the doubled step out: the V-cycle of the other mirrors."""
import numpy as np

import _mg_dense_mirror as DM
import _mg_graph_mirror as GM
import _mg_mirror as MM
from _cheb_mirror import mirror as cheb_mirror
from _mg_mirror import bits, csr_tensor, same_bits  # noqa: F401  (re-exported for the tests)


class Mirror:
    """M(r) of the object `M` with the cycle `cycle` (the object's unless given); `visits[l]` counts the visits of level l."""

    def __init__(self, oracle, M, cycle=None):
        self.oracle, self.M = oracle, M
        self.cycle = M.cycle if cycle is None else cycle
        assert self.cycle in ("V", "W")
        self.levels = []
        for l, lev in enumerate(M.levels):
            c = lev.csr.cpu()
            d = {"csr": (c.crow_indices().numpy(), c.col_indices().numpy(), c.values().numpy())}
            if lev.agg is not None:
                d["agg"] = lev.agg.cpu().numpy()
                d["aptr"], d["amem"] = GM.csr_members(d["agg"], M.levels[l + 1].n)
            if lev.cinv is not None:
                d["C"] = DM.inverse_of(lev)
            self.levels.append(d)
        self.visits = [0] * len(M.levels)

    def _spmv(self, l, x, b):
        spmv = self.oracle.spmv if x.dtype == np.float64 else self.oracle.spmv32
        return spmv(*self.levels[l]["csr"], x, bsub=b)

    def cycle_at(self, l, r):
        lev, d, last = self.M.levels[l], self.levels[l], len(self.levels) - 1
        self.visits[l] += 1
        if l == last:
            return DM.segmented(d["C"], r) if "C" in d else lev.dinv.cpu().numpy().astype(r.dtype) * r
        S = lambda v: cheb_mirror(self.oracle, *d["csr"], lev.smoother, v, dtype=r.dtype.type)
        z = S(r)
        t = self._spmv(l, z, r)
        rc = GM.restrict_np(t, d["aptr"], d["amem"]) if "agg" in d else MM.restrict(t, lev.dims)
        e = self.cycle_at(l + 1, rc)
        if self.cycle == "W" and l + 1 < last:
            rc2 = self._spmv(l + 1, e, rc)
            e2 = self.cycle_at(l + 1, rc2)
            e = e + e2
        z = GM.prolong_add_np(z, e, self.M.omega, d["agg"]) if "agg" in d else MM.prolong_add(z, e, self.M.omega, lev.dims)
        t = self._spmv(l, z, r)
        z = z + S(t)
        assert z.dtype == r.dtype
        return z

    def __call__(self, r, level=0, scale=None):
        """scale * W(level, r) when scale != 1 (scale: the object's unless given)."""
        r = np.ascontiguousarray(r)
        z = self.cycle_at(level, r)
        s = self.M.scale if scale is None else scale
        return r.dtype.type(s) * z if s != 1.0 else z


def apply(oracle, M, r, cycle=None, scale=None):
    return Mirror(oracle, M, cycle)(r, scale=scale)


def launches(M):
    """`launches_per_apply` by walking the cycle and counting: k = 2 degree + 7 per visit of a level above the end (the tail, or the
    last level), two more (steps 4a and 4c) per second visit, one per visit of the end."""
    k, last = 2 * M.degree + 7, len(M.levels) - 1
    end = last if M.tail_from is None else M.tail_from
    count = 0

    def visit(l):
        nonlocal count
        if l == end:
            count += 1
            return
        count += k
        visit(l + 1)
        if M.cycle == "W" and l + 1 < last:
            count += 2
            visit(l + 1)

    visit(0)
    return count
