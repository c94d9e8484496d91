"""Operand layouts a caller may hand to the Python entry points, for tests/test_layout_cases.py (CPU) and
tests/test_gpu_operand_layout.py: views that are contiguous but start off a 16-byte boundary, strided views, a column of a
row-major matrix, the other float type.

Every builder takes `(values, device)` and returns `(view, owner, owner_snapshot)`: `view` holds exactly `values` (the `dtype`
layout: `values` in the other float type), `owner` is the ONE allocation the view lives in, with GUARD seeded sentinel elements
before and after the span the view covers (and between the view's elements where it is strided), and `owner_snapshot` the
owner's bytes (`owner_bytes`) before anything ran.  A callee that writes to its operand, or next to it, changes those bytes.

  fresh       a new tensor (the reference arm): contiguous, 16-byte aligned
  off1        owner[G + 1 : G + 1 + n]           contiguous; 8 mod 16 for 8-byte elements, 4 mod 16 for 4-byte ones
  off2, off3  owner[G + k : G + k + n]           4-byte elements only: 8 and 12 mod 16
  slab        state[n : 2 n] of a 3 n-element state = owner[G : G + 3 n]: off the boundary exactly when n * itemsize % 16 != 0
  stride2     owner[G : G + 2 n : 2]             not contiguous, starts aligned
  column      owner[G : G + 3 n].view(n, 3)[:, 1]  a column of a row-major matrix: not contiguous, itemsize mod 16
  dtype       the values in the other float type, aligned and contiguous inside its guards
and for 2-D values of shape (r, c):
  flat_off1   owner[G + 1 : G + 1 + r c].view(r, c)   contiguous, off the boundary
  transposed  the .T of a (c, r) tensor                not contiguous, starts aligned
"""
import zlib

import torch

GUARD = 64      # sentinel elements on each side; GUARD * itemsize is a multiple of 16 for every dtype used here
LAYOUTS_2D = ("fresh", "flat_off1", "transposed")


def layouts_1d(dtype):
    """The 1-D layouts that exist for `dtype` (off2 / off3 need 4-byte elements; `dtype` needs a float type)."""
    es = torch.empty(0, dtype=dtype).element_size()
    names = ["fresh", "off1"] + (["off2", "off3"] if es == 4 else []) + ["slab", "stride2", "column"]
    return tuple(names + (["dtype"] if dtype.is_floating_point else []))


def owner_bytes(owner: torch.Tensor) -> torch.Tensor:
    """The whole owner as bytes on the host (a copy)."""
    return owner.detach().cpu().contiguous().view(-1).view(torch.uint8).clone()


def _sentinels(numel: int, dtype, name: str) -> torch.Tensor:
    """`numel` seeded sentinel elements (host): large floats / large negative integers no payload here holds."""
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    if dtype.is_floating_point:
        return (torch.rand(numel, generator=g, dtype=torch.float64) + 1.0).mul_(-3.0e33).to(dtype)
    return torch.randint(-(1 << 30), -(1 << 20), (numel,), generator=g, dtype=torch.int64).to(dtype)


def _owner(numel: int, like: torch.Tensor, device, name: str) -> torch.Tensor:
    return _sentinels(numel, like.dtype, name).to(device)


def other_float(dtype):
    return torch.float32 if dtype == torch.float64 else torch.float64


def _finish(view, owner, values):
    view.copy_(values.to(device=view.device, dtype=view.dtype))
    return view, owner


def fresh(values, device):
    t = values.detach().to(device=device).clone(memory_format=torch.contiguous_format)
    return t, t


def _off(k):
    def build(values, device):
        n = values.numel()
        owner = _owner(2 * GUARD + k + n, values, device, f"off{k}")
        return _finish(owner[GUARD + k:GUARD + k + n], owner, values)
    return build


def slab(values, device):
    n = values.numel()
    owner = _owner(2 * GUARD + 3 * n, values, device, "slab")
    state = owner[GUARD:GUARD + 3 * n]
    return _finish(state[n:2 * n], owner, values)


def stride2(values, device):
    n = values.numel()
    owner = _owner(2 * GUARD + 2 * n, values, device, "stride2")
    return _finish(owner[GUARD:GUARD + 2 * n][::2][:n], owner, values)


def column(values, device):
    n = values.numel()
    owner = _owner(2 * GUARD + 3 * n, values, device, "column")
    return _finish(owner[GUARD:GUARD + 3 * n].view(n, 3)[:, 1], owner, values)


def other_dtype(values, device):
    n = values.numel()
    owner = _owner(2 * GUARD + n, values.to(other_float(values.dtype)), device, "dtype")
    return _finish(owner[GUARD:GUARD + n], owner, values)


def flat_off1(values, device):
    r, c = values.shape
    owner = _owner(2 * GUARD + 1 + r * c, values, device, "flat_off1")
    return _finish(owner[GUARD + 1:GUARD + 1 + r * c].view(r, c), owner, values)


def transposed(values, device):
    r, c = values.shape
    owner = _owner(2 * GUARD + r * c, values, device, "transposed")
    return _finish(owner[GUARD:GUARD + r * c].view(c, r).T, owner, values)


BUILDERS = {"fresh": fresh, "off1": _off(1), "off2": _off(2), "off3": _off(3), "slab": slab, "stride2": stride2, "column": column,
            "dtype": other_dtype, "flat_off1": flat_off1, "transposed": transposed}


def build(layout: str, values: torch.Tensor, device="cpu", snapshot: bool = True):
    """(view, owner, owner_snapshot) of `values` in `layout` on `device`; snapshot=False: None for the snapshot (no copy to the
    host: for a callable that builds its result inside a solve)."""
    view, owner = BUILDERS[layout](values, device)
    return view, owner, (owner_bytes(owner) if snapshot else None)


def expected(layout: str, values: torch.Tensor):
    """(is_contiguous, data_ptr % 16) the table above claims for `values` in `layout`."""
    es, n = values.element_size(), values.numel()
    if layout in ("fresh", "dtype"):
        return True, 0
    if layout in ("off1", "off2", "off3", "flat_off1"):
        return True, (int(layout[-1]) * es) % 16
    if layout == "slab":
        return True, (n * es) % 16
    if layout == "stride2":
        return n <= 1, 0
    if layout == "column":
        return n <= 1, es % 16
    if layout == "transposed":
        return min(values.shape) <= 1, 0
    raise KeyError(layout)


def payload(n, dtype, seed: int) -> torch.Tensor:
    """Seeded host values that every float type here holds exactly (drawn in fp32), so that the `dtype` layout and the fresh arm
    give a wrapper the same numbers.  `n`: an int or a shape."""
    g = torch.Generator().manual_seed(seed)
    shape = (n,) if isinstance(n, int) else tuple(n)
    return torch.randn(shape, generator=g, dtype=torch.float32).to(dtype)


def shares_storage(t: torch.Tensor, owner: torch.Tensor) -> bool:
    return t.untyped_storage().data_ptr() == owner.untyped_storage().data_ptr()
