"""tests/_arena.py on CPU tensors (no GPU): the layout (aligned payload start, payload end NOT padded, guards of the asked size
inside one allocation) and that the harness tells five mutant "solves" apart from a correct one.  The solves are numpy stand-ins
with the calling shape of a library solve: work, b read-only, x in/out."""
import numpy as np
import pytest
import torch

from _arena import FILLS, MIN_GUARD, Arena, align_up, check_memory, guard_bytes_for, run_states

SIZES = (1, 63, 255, 2049, 18495)
DTYPES = (torch.float32, torch.float64)
N = 255


def _np(arena):
    """The arena's whole buffer as a numpy array sharing its memory, and the payload's first offset in it."""
    return arena.buf.numpy(), arena.lo


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("align", (16, 256))
def test_layout(n, dtype, align):
    item = torch.empty(0, dtype=dtype).element_size()
    g = guard_bytes_for(n, item)
    assert g >= MIN_GUARD and g >= align_up(n * item, 256) and g >= n * item
    a = Arena("cpu", n * item, align, g)
    v = a.view(dtype, n)
    assert v.data_ptr() % align == 0 and v.data_ptr() == a.data_ptr() and v.numel() == n
    # one allocation; the payload is exactly n elements: the byte after x[n-1] is the first guard byte, not padding
    assert a.payload.numel() == n * item and a.hi - a.lo == n * item
    assert a.lo >= g and a.buf.numel() - a.hi >= g
    assert v.data_ptr() + n * item == a.buf.data_ptr() + a.hi
    assert a.guards_intact()
    buf, lo = _np(a)
    buf[a.hi] ^= 0xFF                      # the very next byte after the payload
    assert not a.guards_intact() and a.touched() == [n * item, n * item, 1]
    buf[a.hi] ^= 0xFF
    v.fill_(3.0)                           # writing every element of the payload touches no guard
    a.fill(0xFF)
    assert a.guards_intact()
    with pytest.raises(AssertionError):    # a view of n + 1 elements does not fit
        a.view(dtype, n + 1)


def test_guard_size_is_a_condition():
    with pytest.raises(AssertionError):
        Arena("cpu", 64, 16, MIN_GUARD - 1)
    assert guard_bytes_for(18495, 8) == align_up(18495 * 8, 256)
    assert guard_bytes_for(1, 4) == MIN_GUARD


def test_sentinel_is_a_seeded_stream_per_arena():
    a, b = Arena("cpu", 1024, 256, MIN_GUARD), Arena("cpu", 1024, 256, MIN_GUARD)
    ga, gb = a.buf[:a.lo][-MIN_GUARD:].numpy(), b.buf[:b.lo][-MIN_GUARD:].numpy()
    assert len(np.unique(ga)) > 200 and not np.array_equal(ga, gb)
    # a copy of a neighbouring vector (or of a constant) over a guard cannot pass
    buf, _ = _np(a)
    buf[a.hi:a.hi + 64] = 0x5A
    assert not a.guards_intact()


# ------------------------------------------------------------------------------------------------ stand-ins for a solve
def _setup():
    item, g = 8, guard_bytes_for(N, 8)
    rng = np.random.default_rng(5)
    xa, ba = Arena("cpu", N * item, 16, g), Arena("cpu", N * item, 16, g)
    x0 = rng.standard_normal(N)
    ba.put(rng.standard_normal(N))
    xa.put(x0)
    work = Arena("cpu", 2 * align_up(N * item, 256), 256, g)
    return work, xa, ba, x0


def _good(work, xa, ba):
    """x += 2 b through a workspace vector that is written before it is read."""
    w = work.view(torch.float64, N).numpy()
    b, x = ba.view(torch.float64, N).numpy(), xa.view(torch.float64, N).numpy()
    w[:] = 2.0 * b
    x += w


def _before_payload(work, xa, ba):
    _good(work, xa, ba)
    buf, lo = _np(xa)
    buf[lo - 1] ^= 1


def _after_payload(work, xa, ba):
    _good(work, xa, ba)
    buf, _ = _np(xa)
    buf[xa.hi] ^= 1


def _vector_after_work(work, xa, ba):
    _good(work, xa, ba)
    buf, _ = _np(work)                    # one whole 256-aligned vector past the end of the workspace
    buf[work.hi:work.hi + align_up(N * 8, 256)] = 0


def _reads_before_write(work, xa, ba):
    w = work.payload.numpy()
    stale = w[N * 8 + 5] == 0xFF          # one byte of the second work vector, read before anything wrote it
    _good(work, xa, ba)
    if stale:
        xa.view(torch.float64, N).numpy()[N - 1] += 1.0


def _modifies_b(work, xa, ba):
    _good(work, xa, ba)
    ba.view(torch.float64, N).numpy()[0] *= -1.0


def _drive(solve):
    work, xa, ba, x0 = _setup()

    def run(i):
        xa.view(torch.float64, N).numpy()[:] = x0
        solve(work, xa, ba)
        return {"x": xa.payload.numpy().tobytes()}
    return run_states(work, {"x": xa, "b": ba}, {"b": ba}, run, FILLS, label=solve.__name__)


def test_correct_solve_passes():
    res = _drive(_good)
    assert len(res) == 4 and all(r == res[0] for r in res)


MUTANTS = [
    ("write one byte before the payload", _before_payload, r"a write outside `x` \(first, last offset from its payload, bytes: \[-1, -1, 1\]"),
    ("write one byte after the payload", _after_payload, rf"a write outside `x` \(first, last offset from its payload, bytes: \[{N * 8}, {N * 8}, 1\]"),
    ("write one whole vector after the workspace", _vector_after_work, r"a write outside `work`"),
    ("result depends on a payload byte read before it is written", _reads_before_write,
     r"run 2 \(0xFF fill\): `x` depends on what the workspace held"),
    ("solve modifies b", _modifies_b, r"read-only operand `b` was modified"),
]


@pytest.mark.parametrize("name, solve, message", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_mutant_is_told_apart(name, solve, message):
    with pytest.raises(AssertionError, match=message):
        _drive(solve)


def test_stale_read_passes_under_zero_fill_alone():
    """Mutant 4 is invisible to a single run on a zeroed workspace: what the other three states are for."""
    work, xa, ba, x0 = _setup()

    def run(i):
        xa.view(torch.float64, N).numpy()[:] = x0
        _reads_before_write(work, xa, ba)
        return {"x": xa.payload.numpy().tobytes()}
    run_states(work, {"x": xa, "b": ba}, {"b": ba}, run, (0x00,))


def test_an_error_of_the_call_names_the_state():
    """A call that ends with an error under one fill only (a library status, a path assertion of the runner) is reported with
    the run and the fill it happened in."""
    work, xa, ba, _ = _setup()

    def run(i):
        if work.payload[7] == 0x5A:
            raise RuntimeError("a resident workgroup stopped arriving")
        return {}
    with pytest.raises(AssertionError, match=r"lbl run 3 \(0x5A fill\): RuntimeError: a resident workgroup stopped arriving"):
        run_states(work, {"x": xa}, {}, run, FILLS, label="lbl")


def test_check_memory_names_the_arena():
    work, xa, ba, _ = _setup()
    ba.snapshot()
    check_memory({"x": xa, "b": ba, "work": work}, {"b": ba}, "clean")
    buf, lo = _np(ba)
    buf[lo - 7] ^= 0x80
    with pytest.raises(AssertionError, match="`b`"):
        check_memory({"x": xa, "b": ba, "work": work}, {"b": ba}, "dirty")


def test_wrappers_check_a_callers_workspace():
    """_hipk._workspace (behind every wrapper's `work=`): the caller's tensor itself when it is a contiguous uint8 tensor on the
    device, aligned and at least as long as the library's figure; HipkError otherwise; a fresh allocation for None."""
    from pytorch_sparse_solver import _hipk
    a = Arena("cpu", 1024, 256, MIN_GUARD)
    assert _hipk._workspace(a.payload, "cpu", 1024) is a.payload
    assert _hipk._workspace(a.buf[a.lo:], "cpu", 1024).data_ptr() == a.data_ptr()     # longer than asked: accepted
    assert _hipk._workspace(None, "cpu", 1000).shape == (1000,)
    for bad in (a.payload[:1023], a.buf[a.lo + 16:a.lo + 16 + 1024], a.payload.view(torch.int32), a.buf[a.lo:a.lo + 2048][::2], [0] * 1024):
        with pytest.raises(_hipk.HipkError):
            _hipk._workspace(bad, "cpu", 1024)
    assert _hipk._workspace(a.buf[a.lo + 16:a.lo + 16 + 1024], "cpu", 1024, 16).numel() == 1024   # the Chebyshev work vectors: 16
