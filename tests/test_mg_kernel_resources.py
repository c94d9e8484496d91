"""Register and scratch budgets of the multigrid kernels of csrc/hipk_mg.hip (compiled for gfx950 here, the compiler's own resource
report read as tests/test_bj_batch_kernel_resources.py does; no GPU needed).

The tail kernel is one workgroup that walks every small level: the degree and the level count are run-time values, so the loops over
the Chebyshev steps and the levels must stay loops and the per-level pointers must stay in registers.  Both instantiations have no
scratch and at most 128 VGPRs; so do the streaming transfer kernels."""
import os
import shutil

import pytest

from test_kernel_resources import HIPCC, _vgprs

TAIL = [f"void hipk_mg_tail_kernel<{t}>" for t in ("double", "float")]
STREAM = [f"void hipk_mg_{k}_kernel<{t}>" for k in ("restrict", "prolong_add", "correct", "diag") for t in ("double", "float")]


@pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("c++filt") is None, reason="hipcc / c++filt not installed")
def test_mg_kernels_have_no_scratch_and_at_most_128_vgprs():
    got = _vgprs("hipk_mg.hip")
    ours = {k: v for k, v in got.items() if "hipk_mg_" in k}
    assert sorted(k.split("(")[0] for k in ours) == sorted(TAIL + STREAM), sorted(got)
    for k, v in ours.items():
        print(f"{k}: {v} VGPRs, {_vgprs.sgprs[k]} SGPRs, {_vgprs.scratch[k]} bytes of scratch")
        assert _vgprs.scratch[k] == 0, f"{k}: {_vgprs.scratch[k]} bytes of scratch per lane"
        assert v <= 128, f"{k}: {v} VGPRs"
