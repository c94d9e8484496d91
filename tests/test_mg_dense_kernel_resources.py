"""Register and scratch budgets of the dense-level kernels of csrc/hipk_mg_dense.hip (compiled for gfx950 here, the compiler's own
resource report read as tests/test_mg_kernel_resources.py does; no GPU needed).

The launch of its own keeps 16 loads of the inverse in flight per thread; the tail walks up to 32 levels with a run-time degree
around the dense step.  Their four instantiations have no scratch and at most 128 VGPRs, and they are the only kernels of the
translation unit."""
import os
import shutil

import pytest

from test_kernel_resources import HIPCC, _vgprs

KERNELS = [f"void hipk_mg_{k}_kernel<{t}>" for k in ("dense", "gtail_dense") for t in ("double", "float")]


@pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("c++filt") is None, reason="hipcc / c++filt not installed")
def test_mg_dense_kernels_have_no_scratch_and_at_most_128_vgprs():
    got = _vgprs("hipk_mg_dense.hip")
    assert sorted(k.split("(")[0] for k in got) == sorted(KERNELS), sorted(got)
    for k, v in got.items():
        print(f"{k}: {v} VGPRs, {_vgprs.sgprs[k]} SGPRs, {_vgprs.scratch[k]} bytes of scratch")
        assert _vgprs.scratch[k] == 0, f"{k}: {_vgprs.scratch[k]} bytes of scratch per lane"
        assert v <= 128, f"{k}: {v} VGPRs"
