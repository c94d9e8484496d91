"""numpy mirrors of the two folds of chunk partials that the fused CG launch must keep bit-identical (csrc/hipk_cg_fuse.h):

spec_fold       -- a transcription of hipk_reduce_parts + hipk_block_sum (csrc/hipk_common.h), the fold every separate kernel runs:
                   thread t of 256 sums words t, t + 256, ... ascending from 0.0, then the tree with strides 128, 64, 32 ... 1.
two_level_fold  -- the eight collectors' fold: collector s sums residue class s (threads t = s + 8 j, j = 0 .. 31: the chain of
                   each, then the halving tree over j, strides 16 .. 1), and every workgroup folds the eight class sums as
                   ((c0 + c4) + (c2 + c6)) + ((c1 + c5) + (c3 + c7)).

Every addition is one IEEE double addition in the order the device code performs it; numpy adds element-wise, so a vectorised
step is the same additions as the lanes' own."""
import numpy as np

THREADS = 256
MAX_PARTS = 2048
COLLECTORS = 8


def _chains(parts, first, stride_t, count):
    """acc[k] = 0.0, then acc[k] = acc[k] + parts[i] for i = first + stride_t * k + 256 * m < g, m ascending."""
    g = parts.size
    idx = first + stride_t * np.arange(count)
    acc = np.zeros(count, dtype=np.float64)
    for m in range(MAX_PARTS // THREADS):
        i = idx + THREADS * m
        have = i < g
        acc[have] = acc[have] + parts[i[have]]
    return acc


def _halve(v, strides):
    """v[t] = v[t] + v[t + s] for t < s, for each stride s in turn; the sum ends in v[0]."""
    v = v.copy()
    for s in strides:
        v[:s] = v[:s] + v[s:2 * s]
    return v[0]


def spec_fold(parts):
    parts = np.ascontiguousarray(parts, dtype=np.float64)
    assert 0 < parts.size <= MAX_PARTS
    return _halve(_chains(parts, 0, 1, THREADS), (128, 64, 32, 16, 8, 4, 2, 1))


def class_sum(parts, s):
    """What collector s hands out."""
    parts = np.ascontiguousarray(parts, dtype=np.float64)
    return _halve(_chains(parts, s, COLLECTORS, THREADS // COLLECTORS), (16, 8, 4, 2, 1))


def line_fold(c):
    """What a workgroup makes of the eight slots of its line."""
    c = [np.float64(v) for v in c]
    return ((c[0] + c[4]) + (c[2] + c[6])) + ((c[1] + c[5]) + (c[3] + c[7]))


def two_level_fold(parts):
    return line_fold([class_sum(parts, s) for s in range(COLLECTORS)])
