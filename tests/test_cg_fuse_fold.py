"""The eight collectors of the fused CG launch split the spec's fold of chunk partials eight ways (csrc/hipk_cg_fuse.h, steps 4
and 8).  No GPU: the numpy mirror of the two-level fold (tests/_cg_fuse_fold_mirror.py) against a transcription of
hipk_reduce_parts + hipk_block_sum, byte for byte, over the envelope of the form (512 < g <= 2048)."""
import numpy as np
import pytest

from _cg_fuse_fold_mirror import class_sum, line_fold, spec_fold, two_level_fold

GS = sorted(set(range(513, 531)) | {519, 520, 591, 768, 769, 958, 1023, 1024, 1025, 1954, 2047, 2048})


def _value_sets(g, seed):
    """Partials as a solve can produce them and as it cannot: 24 decades of magnitude with mixed and with all-positive signs, sums
    that cancel (exactly and almost), signed zeros, and the all-ones case whose sum is exact in any order."""
    rng = np.random.default_rng(seed)
    mag = 10.0 ** rng.uniform(-12.0, 12.0, g)
    mixed = mag * rng.choice([-1.0, 1.0], g)
    yield "24 decades, mixed signs", mixed
    yield "24 decades, positive", mag
    yield "standard normal", rng.standard_normal(g)
    cancel = rng.standard_normal(g) * 1e8
    cancel[1::2] = -cancel[0:2 * (g // 2):2]
    yield "pairs that cancel exactly", cancel
    near = cancel.copy()
    near[::3] *= 1.0 + 2.0 ** -50
    yield "pairs that almost cancel", near
    zeros = np.where(rng.random(g) < 0.5, 0.0, -0.0)
    yield "signed zeros", zeros
    sparse = np.where(rng.random(g) < 0.9, zeros, mixed)
    yield "signed zeros and a few values", sparse
    yield "minus zero everywhere", np.full(g, -0.0)
    yield "ones", np.ones(g)


@pytest.mark.parametrize("g", GS)
def test_the_two_level_fold_has_the_bits_of_the_spec_fold(g):
    for name, parts in _value_sets(g, g):
        assert parts.size == g
        want, got = spec_fold(parts), two_level_fold(parts)
        assert np.float64(want).tobytes() == np.float64(got).tobytes(), (g, name, float(want).hex(), float(got).hex())


def test_the_transcription_is_the_spec():
    """The transcription against the fold written out thread by thread, scalar by scalar, as csrc/hipk_common.h has it."""
    rng = np.random.default_rng(1)
    for g in (513, 1954, 2048):
        parts = rng.standard_normal(g) * 10.0 ** rng.uniform(-6.0, 6.0, g)
        v = [np.float64(0.0)] * 256
        for t in range(256):
            acc = np.float64(0.0)
            for k in range(8):
                if t + 256 * k < g:
                    acc = acc + parts[t + 256 * k]
            v[t] = acc
        for t in range(128):
            v[t] = v[t] + v[t + 128]
        d = [v[t] + v[t + 64] for t in range(64)]
        for s in (32, 16, 8, 4, 2, 1):
            for t in range(s):
                d[t] = d[t] + d[t + s]
        assert np.float64(d[0]).tobytes() == np.float64(spec_fold(parts)).tobytes(), g


def test_a_class_takes_exactly_its_words():
    """Collector s reads the words s, s + 8, ...: a value planted in word i reaches class i % 8 alone, and with one word the
    folds return it unchanged (minus zero becomes plus zero in both: the chain starts from 0.0)."""
    g = 1954
    for i in (0, 7, 8, 255, 256, 1023, 1948, 1953):
        parts = np.zeros(g)
        parts[i] = 3.5
        sums = [class_sum(parts, s) for s in range(8)]
        assert sums[i % 8] == 3.5 and sum(1 for c in sums if c != 0.0) == 1, (i, sums)
        assert two_level_fold(parts) == 3.5 == spec_fold(parts)
    assert np.float64(line_fold([-0.0] * 8)).tobytes() == np.float64(-0.0).tobytes()   # (the lane reads add nothing of their own)
    assert np.float64(two_level_fold(np.full(513, -0.0))).tobytes() == np.float64(0.0).tobytes()
