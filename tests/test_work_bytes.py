"""The workspace sizes of the single-device cg, pcg, bicgstab and pbicgstab solves (csrc: hipk_cg_layout, hipk_bi_layout) are part of
the interface: _hipk.py, the arenas of the memory-contract tests and users size buffers by them.  tests/golden/work_bytes.json holds
what the library returned before the layouts existed, on both sides of every size at which a layout condition flips.  Pure host
code: no GPU needed."""
import json
import os

from conftest import GOLDEN


def test_work_bytes_are_the_recorded_ones():
    import torch  # noqa: F401  (HIP runtime first)
    from pytorch_sparse_solver import _hipk
    if not os.path.exists(_hipk.LIB_PATH):
        _hipk.build()
    L = _hipk.lib()
    with open(os.path.join(GOLDEN, "work_bytes.json")) as f:
        fx = json.load(f)
    assert "recorded from the library built at commit" in fx["header"]
    cols = fx["columns"]
    assert cols[0] == "n" and len(cols) == 9
    ns = [row[0] for row in fx["rows"]]
    for c in (8, 32, 150, 256, 512):   # the last row of one chunk count and the first of the next
        assert c * 2048 in ns and c * 2048 + 1 in ns
    for n in (1, 1000, 4_000_000, 64_000_000, 12_582_912, 12_582_913, 25_165_824, 25_165_825):
        assert n in ns
    for row in fx["rows"]:
        assert len(row) == len(cols)
        for col, want in zip(cols[1:], row[1:]):
            name, dt = col.rsplit("_", 1)
            got = int(getattr(L, f"hipk_{name}_work_bytes")(row[0], _hipk.HIPK_F64 if dt == "f64" else _hipk.HIPK_F32))
            assert got == want, (col, row[0], got, want)
