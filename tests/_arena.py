"""Guarded memory for the tests of the library's memory contract (include/hipk.h: "`work` >= *_work_bytes", "`b` is not modified").

An Arena is ONE uint8 tensor laid out as [guard | payload | guard].  The payload starts at an `align`-aligned address and is exactly
`payload_bytes` long: the byte after the last element is guard, not padding.  Both guards hold a seeded byte stream (not a constant:
a copy of a neighbouring vector cannot pass for it) and lie inside the arena's own allocation, so an overrun of up to `guard_bytes`
lands in memory the test owns: it is seen, it never faults.  Works on any torch device (tests/test_arena.py runs it on the CPU).

run_states() is the four-state protocol of the solve tables: the same call with the workspace filled with 0x00, 0xFF (every fp word a
NaN, every flag ~0, every counter -1), 0x5A (large finite doubles, large positive flags) and NOT refilled (as the previous run left
it); guards and read-only operands are checked after every run, and every later run must reproduce the first one bit for bit."""
import itertools

import numpy as np
import torch

MIN_GUARD = 4096
FILLS = (0x00, 0xFF, 0x5A, None)       # None: no refill, the workspace as the run before left it
FILLS_SHORT = (0x00, 0xFF)             # what a case whose solve alone takes more than 0.5 s keeps
_serial = itertools.count(1)


def align_up(v, a):
    return (int(v) + a - 1) // a * a


def guard_bytes_for(n, itemsize):
    """The guard of a case with vectors of n elements: one 256-aligned vector (what the libraries' carving steps by), at least 4096."""
    return max(MIN_GUARD, align_up(int(n) * int(itemsize), 256))


def fill_name(fill):
    return "no refill" if fill is None else f"0x{fill:02X} fill"


class Arena:
    def __init__(self, device, payload_bytes, align, guard_bytes):
        payload_bytes, align, guard_bytes = int(payload_bytes), int(align), int(guard_bytes)
        assert payload_bytes >= 0 and align >= 1 and (align & (align - 1)) == 0
        assert guard_bytes >= MIN_GUARD, "a guard is at least 4096 bytes (and at least one vector of the case)"
        self.align, self.payload_bytes, self.guard_bytes = align, payload_bytes, guard_bytes
        self.buf = torch.empty(guard_bytes + align + payload_bytes + guard_bytes, dtype=torch.uint8, device=device)
        base = self.buf.data_ptr()
        self.lo = guard_bytes + (-(base + guard_bytes)) % align
        self.hi = self.lo + payload_bytes
        assert self.lo >= guard_bytes and self.buf.numel() - self.hi >= guard_bytes
        # the per-arena sentinel: a seeded byte stream over the whole buffer (the payload's part of it is never compared)
        rng = np.random.default_rng([0x41524E41, next(_serial), payload_bytes])
        self._sentinel = torch.from_numpy(rng.integers(0, 256, self.buf.numel(), dtype=np.uint8)).to(device)
        self.buf.copy_(self._sentinel)
        self.payload = self.buf[self.lo:self.hi]
        self._snap = None

    def data_ptr(self):
        return self.buf.data_ptr() + self.lo

    def fill(self, byte):
        self.payload.fill_(int(byte))
        return self

    def view(self, dtype, n):
        """The first n elements of the payload as `dtype` (n elements must fit; an arena made for n elements holds exactly n)."""
        nb = int(n) * torch.empty(0, dtype=dtype).element_size()
        assert nb <= self.payload_bytes, (nb, self.payload_bytes)
        return self.payload[:nb].view(dtype)

    def put(self, src):
        """Copy a numpy array or tensor into the payload (it must fill it exactly) and return the typed view."""
        t = torch.from_numpy(np.ascontiguousarray(src)) if isinstance(src, np.ndarray) else src.contiguous()
        v = self.view(t.dtype, t.numel())
        assert t.numel() * t.element_size() == self.payload_bytes
        v.copy_(t.reshape(-1))
        return v

    def guards_intact(self):
        return bool(torch.equal(self.buf[:self.lo], self._sentinel[:self.lo]) and
                    torch.equal(self.buf[self.hi:], self._sentinel[self.hi:]))

    def touched(self):
        """Where the guards differ from the sentinel: offsets relative to the payload's first byte (negative: before it)."""
        d = (self.buf != self._sentinel)
        d[self.lo:self.hi] = False
        idx = torch.nonzero(d).flatten().cpu().numpy()
        return [] if idx.size == 0 else [int(idx.min()) - self.lo, int(idx.max()) - self.lo, int(idx.size)]

    def snapshot(self):
        self._snap = self.payload.clone()
        return self

    def unchanged(self):
        assert self._snap is not None, "snapshot() first"
        return bool(torch.equal(self.payload, self._snap))


def check_memory(guarded, readonly, when):
    """Every arena of `guarded` (name -> Arena) has its guards intact, every one of `readonly` equals its snapshot."""
    for name, a in guarded.items():
        assert a.guards_intact(), (f"{when}: a write outside `{name}` "
                                   f"(first, last offset from its payload, bytes: {a.touched()}; payload {a.payload_bytes} bytes)")
    for name, a in readonly.items():
        assert a.unchanged(), f"{when}: read-only operand `{name}` was modified"


def run_states(work, guarded, readonly, run, fills=FILLS, label=""):
    """run(i) -> dict name -> bytes: one call of the code under test per workspace state (it restores its own in/out operands from
    the same start every time).  After every run: check_memory.  Runs after the first must return the same bytes under every name.
    Returns the list of results (results[0] feeds the caller's reference comparison)."""
    assert fills[0] == 0x00
    guarded = dict(guarded, work=work)
    for a in readonly.values():
        a.snapshot()
    results = []
    for i, fill in enumerate(fills):
        if fill is not None:
            work.fill(fill)
        when = f"{label} run {i + 1} ({fill_name(fill)})"
        try:
            res = run(i)
        except Exception as e:   # an error status of the library, or an assertion of run's own: say in which state
            raise AssertionError(f"{when}: {type(e).__name__}: {e}") from e
        check_memory(guarded, readonly, when)
        if results:
            for k, v in results[0].items():
                assert res[k] == v, f"{when}: `{k}` depends on what the workspace held (differs from the 0x00-fill run)"
        results.append(res)
    return results
