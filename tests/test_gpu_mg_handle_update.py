"""AggregationMultigridPreconditioner.update on a device object keeps its CsrHandles: the coarse levels' handles live in `_keep` and
take the new values through CsrHandle.update_values, level 0's cached handle moves to the new matrix through refresh_matrix(A_new,
like=A_old) when A_new is a CSR tensor on A_old's index tensors.

Poisson and variable diffusion on a 64 x 64 grid, for the three kinds of hierarchy (grid, from_graph(), coarse_rows=...), each with
the tail kernel (the levels of at most 1024 unknowns are one launch: level 0 has a handle, and level 1 of a graph hierarchy) and with tail_rows=0 (every level above the
last has a handle).  The reference is an object built with normalize=False -- a constructor that estimates the norm applies the
hierarchy and so makes its handles -- that is never applied before its update and is updated with a matrix on index tensors of its
own: every handle it uses is constructed fresh, after the update, on the same aggregates; its norm estimate then runs on those
(tests/test_gpu_mg_refresh.py builds its never-applied object the same way and pins a refreshed object to the CPU object and the
mirror)."""
import numpy as np
import pytest
import torch

import _mg_mirror as MM
from pytorch_sparse_solver.module_a import AggregationMultigridPreconditioner as MG
from pytorch_sparse_solver.module_a import cg, get_last_stats
from pytorch_sparse_solver.utils.matrix_utils import create_poisson_2d_csr, create_variable_diffusion_2d_csr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NX = 64
KINDS = {"grid": {}, "grid_no_tail": {"tail_rows": 0}, "graph": {}, "graph_no_tail": {"tail_rows": 0},
         "dense": {"coarse_rows": 64}, "dense_no_tail": {"coarse_rows": 64, "tail_rows": 0}}


def _np(A):
    return A.crow_indices().numpy(), A.col_indices().numpy(), A.values().numpy()


def _arrays(system):
    """(the arrays the object is built from, other values on the same pattern)."""
    p, v1, v2 = (_np(create_poisson_2d_csr(NX, NX)), _np(create_variable_diffusion_2d_csr(NX, NX, contrast=3.0, seed=7)),
                 _np(create_variable_diffusion_2d_csr(NX, NX, contrast=2.0, seed=9)))
    assert np.array_equal(p[0], v1[0]) and np.array_equal(p[1], v1[1]) and np.array_equal(p[1], v2[1])
    return (p, v1) if system == "poisson" else (v1, v2)


def _build(kind, A, **more):
    kw = dict(KINDS[kind], **more)
    return MG(A, (NX, NX), **kw) if kind.startswith("grid") else MG.from_graph(A, **kw)


def _count_inits(hipk, monkeypatch):
    made = []
    init = hipk.CsrHandle.__init__

    def counted(self, *a, **kw):
        made.append(self)
        return init(self, *a, **kw)
    monkeypatch.setattr(hipk.CsrHandle, "__init__", counted)
    return made


def _bits(t):
    return t.detach().cpu().numpy().tobytes()


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("system", ["poisson", "variable"])
def test_an_update_constructs_no_handle_and_is_the_object_with_fresh_handles(hipk, monkeypatch, system, kind):
    first, other = _arrays(system)
    n = NX * NX
    r = torch.from_numpy(np.random.default_rng(5).standard_normal(n)).to(DEV)
    b = torch.ones(n, dtype=torch.float64, device=DEV)
    hipk.clear_cache()
    A = MM.csr_tensor(*first, device=DEV)
    M = _build(kind, A)
    M(r)
    x0, info0 = cg(A, b, tol=1e-8, M=M)
    assert info0 == 0
    level_handles = {k: h for k, h in M._keep.items() if k[1] == "h"}
    # (with the tail kernel a grid hierarchy has level 0's handle alone; a graph hierarchy's level 1, 1241 rows, is above the tail too)
    assert level_handles or not kind.endswith("no_tail"), (sorted(level_handles), len(M.levels), M.tail_from)
    h0 = hipk.handle_for(A)
    B = torch.sparse_csr_tensor(A.crow_indices(), A.col_indices(), torch.from_numpy(other[2]).to(DEV), size=A.shape)   # A's index tensors
    made = _count_inits(hipk, monkeypatch)
    assert M.update(B) is M
    z = M(r)
    x, info = cg(B, b, tol=1e-8, M=M)
    it = get_last_stats().iterations
    assert info == 0
    assert made == [], f"{len(made)} CsrHandle(s) constructed by an update, its apply and the solve after it"
    assert hipk.handle_for(B) is h0 and all(M._keep[k] is h for k, h in level_handles.items())
    monkeypatch.undo()
    # the reference: no handle before its update, a matrix on index tensors of its own -- every handle fresh, the same aggregates
    hipk.clear_cache()
    N = _build(kind, MM.csr_tensor(*first, device=DEV), normalize=False)
    assert not [k for k in N._keep if k[1] == "h"] and hipk.cache_info()[0] == 0
    B2 = MM.csr_tensor(*other, device=DEV)
    made = _count_inits(hipk, monkeypatch)
    N.update(B2)
    assert made == []                                              # nothing is applied by an update without a norm estimate
    N._estimate_scale()                                            # the constructor's estimate, on handles made now
    zN = N(r)
    xN, infoN = cg(B2, b, tol=1e-8, M=N)
    assert len(made) == 1 + len(level_handles)
    assert N.scale == M.scale and _bits(zN) == _bits(z), "M(r) differs from the object with fresh handles"
    assert infoN == info and get_last_stats().iterations == it and _bits(xN) == _bits(x), "the solve differs from the one with fresh handles"
    print(f"{system} {kind}: {len(M.levels)} levels, tail from {M.tail_from}, {len(level_handles)} kept coarse handles, {it} iterations")


@pytest.mark.parametrize("kind", ["graph_no_tail", "grid_no_tail"])
def test_an_update_that_raises_after_the_handles_took_the_new_values_changes_nothing(hipk, monkeypatch, kind):
    """Crafted values reach the late raise: the matrix scaled by 1e-310 has a positive (subnormal) diagonal on every level and the
    same Gershgorin bounds, so the level scans pass and the coefficients exist, but 1 / d overflows: the norm estimate, which applies
    the NEW hierarchy through the kept handles before the swap, sees a ||M v|| that is not finite and raises."""
    first, other = _arrays("poisson")
    n = NX * NX
    r = torch.from_numpy(np.random.default_rng(6).standard_normal(n)).to(DEV)
    b = torch.ones(n, dtype=torch.float64, device=DEV)
    hipk.clear_cache()
    A = MM.csr_tensor(*first, device=DEV)
    M = _build(kind, A)
    z0 = _bits(M(r))
    x0, _ = cg(A, b, tol=1e-8, M=M)
    it0 = get_last_stats().iterations
    h0 = hipk.handle_for(A)
    tiny = torch.sparse_csr_tensor(A.crow_indices(), A.col_indices(), A.values() * 1e-310, size=A.shape)
    assert float(tiny.values().abs().min()) > 0.0
    touched = []
    update_values = hipk.CsrHandle.update_values

    def counted(self, values):
        touched.append(self)
        return update_values(self, values)
    monkeypatch.setattr(hipk.CsrHandle, "update_values", counted)
    with pytest.raises(ValueError, match="norm estimate"):
        M.update(tiny)
    monkeypatch.undo()
    coarse = [h for k, h in M._keep.items() if k[1] == "h"]
    assert h0 in touched and all(h in touched for h in coarse) and coarse, "the update raised before a handle was touched"
    assert M.updates == 0 and hipk.handle_for(A) is h0
    assert _bits(M(r)) == z0
    x1, info1 = cg(A, b, tol=1e-8, M=M)
    assert info1 == 0 and get_last_stats().iterations == it0 and _bits(x1) == _bits(x0)
    # and the handles are those of their values again: the object with fresh handles gives the same bits
    hipk.clear_cache()
    N = _build(kind, MM.csr_tensor(*first, device=DEV))
    assert _bits(N(r)) == z0
