"""Without a GPU: the layout builders of tests/_layout_cases.py give what their table claims, and `_hipk.aligned` -- the one rule
every Python entry applies to an operand whose address goes to libhipk.so -- returns an aligned contiguous tensor with the same
values, the operand ITSELF when it already is one, and never writes to what it was given.  Pure torch, on CPU tensors."""
import pytest
import torch

import _layout_cases as lc

# odd lengths (a slab of them starts off the boundary in either element size), the sizes of tests/test_gpu_operand_layout.py
SIZES = (1, 35, 2051)
DTYPES = (torch.float64, torch.float32, torch.int64, torch.int32)
IDS_DT = ("f64", "f32", "i64", "i32")


def _values(n, dtype, seed=7):
    if dtype.is_floating_point:
        return lc.payload(n, dtype, seed)
    shape = (n,) if isinstance(n, int) else tuple(n)
    return torch.randint(0, 1 << 20, shape, generator=torch.Generator().manual_seed(seed), dtype=torch.int64).to(dtype)


def _cases_1d():
    for dt, name in zip(DTYPES, IDS_DT):
        for n in SIZES:
            for layout in lc.layouts_1d(dt):
                yield pytest.param(layout, n, dt, id=f"{layout}-{name}-n{n}")


def _cases_2d():
    for dt, name in zip(DTYPES[:2], IDS_DT[:2]):
        for shape in ((35, 3), (8, 35), (2051, 3)):
            for layout in lc.LAYOUTS_2D:
                yield pytest.param(layout, shape, dt, id=f"{layout}-{name}-{shape[0]}x{shape[1]}")


ALL = list(_cases_1d()) + list(_cases_2d())


def _want_values(layout, values):
    return values.to(lc.other_float(values.dtype)) if layout == "dtype" else values


@pytest.mark.parametrize("layout,n,dt", ALL)
def test_builder_gives_the_layout_its_table_claims(layout, n, dt):
    values = _values(n, dt)
    view, owner, snap = lc.build(layout, values)
    contiguous, mod16 = lc.expected(layout, values)
    assert view.is_contiguous() == contiguous and view.data_ptr() % 16 == mod16, (view.stride(), view.data_ptr() % 16)
    assert view.shape == values.shape
    want = _want_values(layout, values)
    assert view.dtype == want.dtype and torch.equal(view, want)
    if dt.is_floating_point and layout == "dtype":      # ... and no value was rounded on the way to the other float type
        assert torch.equal(view.to(dt), values)
    assert (owner.dim() == 1 or layout == "fresh") and owner.is_contiguous() and owner.data_ptr() % 16 == 0 and lc.shares_storage(view, owner)
    assert torch.equal(lc.owner_bytes(owner), snap)
    if layout != "fresh":
        # GUARD sentinel elements before the first and after the last element of the view, none of them a payload value
        first = (view.data_ptr() - owner.data_ptr()) // owner.element_size()
        span = 1 + sum((s - 1) * st for s, st in zip(view.shape, view.stride()))
        assert first >= lc.GUARD and owner.numel() - (first + span) >= lc.GUARD
        for g in (owner[:lc.GUARD], owner[-lc.GUARD:]):
            assert not torch.isin(g, want.reshape(-1)).any()


def test_every_slab_size_used_starts_off_the_boundary():
    for n in (35, 2051, 16637, 17 * 13):
        for dt in (torch.float64, torch.float32):
            assert lc.expected("slab", torch.empty(n, dtype=dt))[1] != 0, (n, dt)


@pytest.mark.parametrize("layout,n,dt", ALL)
def test_aligned_is_the_operand_itself_or_an_aligned_copy(layout, n, dt):
    from pytorch_sparse_solver import _hipk
    values = _values(n, dt)
    view, owner, snap = lc.build(layout, values)
    got = _hipk.aligned(view)
    if view.is_contiguous() and view.data_ptr() % 16 == 0:
        # no copy for an operand the library can take as it is (bench.py's operands, every fresh tensor)
        assert got is view
        assert layout in ("fresh", "dtype") or view.numel() <= 1 or lc.expected(layout, values) == (True, 0)
    else:
        assert got is not view and not lc.shares_storage(got, owner)
        assert got.is_contiguous() and got.data_ptr() % 16 == 0
        assert got.dtype == view.dtype and got.shape == view.shape and torch.equal(got, view)
        got.add_(1)                                     # a copy: writing to it leaves the operand alone
    assert torch.equal(view, _want_values(layout, values))
    assert torch.equal(lc.owner_bytes(owner), snap), "aligned() wrote to its operand's allocation"


def test_aligned_with_another_boundary():
    from pytorch_sparse_solver import _hipk
    buf = torch.zeros(256, dtype=torch.uint8)
    assert buf.data_ptr() % 64 == 0
    v = buf[16:48]
    assert _hipk.aligned(v) is v and _hipk.aligned(v, 16) is v
    w = _hipk.aligned(v, 64)
    assert w is not v and w.data_ptr() % 64 == 0 and torch.equal(w, v)
    e = buf[3:3]
    assert _hipk.aligned(e).numel() == 0


def test_csr_tensor_keeps_a_values_view():
    """What makes the helper necessary where a matrix is handed over: torch keeps the view, and .contiguous() keeps it too."""
    n, nnz = 3, 5
    vals, owner, _ = lc.build("off1", _values(nnz, torch.float64))
    A = torch.sparse_csr_tensor(torch.tensor([0, 2, 3, 5]), torch.tensor([0, 1, 1, 0, 2]), vals, size=(n, n))
    assert A.values().data_ptr() == vals.data_ptr() and A.values().data_ptr() % 16 == 8
    assert vals.contiguous().data_ptr() == vals.data_ptr()
