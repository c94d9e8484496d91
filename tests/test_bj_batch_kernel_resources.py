"""Register and scratch budgets of the block-Jacobi batch kernels of csrc/hipk_batch_bj.hip (compiled for gfx950 here, the compiler's
own resource report read as tests/test_batch_kernel_resources.py does; no GPU needed).

block_size is a run-time value: the loop over a block's columns must stay a loop (a per-thread array indexed with it would go to
scratch).  As for the other batch kernels, residency is to be decided by LDS, so every instantiation has no scratch, at most 128
VGPRs and at most 80 SGPRs."""
import os
import shutil

import pytest

from test_kernel_resources import HIPCC, _vgprs

KERNELS = [f"void hipk_{k}_bjbatch_kernel<{t}>" for k in ("cg", "bi") for t in ("double", "float")]


@pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("c++filt") is None, reason="hipcc / c++filt not installed")
def test_bj_batch_kernels_fit_four_workgroups_per_cu_without_scratch():
    got = _vgprs("hipk_batch_bj.hip")
    ours = {k: v for k, v in got.items() if "_bjbatch_kernel<" in k}
    assert sorted(ours) == sorted(KERNELS), sorted(got)
    for k, v in ours.items():
        print(f"{k}: {v} VGPRs, {_vgprs.sgprs[k]} SGPRs, {_vgprs.scratch[k]} bytes of scratch")
        assert _vgprs.scratch[k] == 0, f"{k}: {_vgprs.scratch[k]} bytes of scratch per lane"
        assert v <= 128, f"{k}: {v} VGPRs (> 128: fewer than four workgroups per CU)"
        assert _vgprs.sgprs[k] <= 80, f"{k}: {_vgprs.sgprs[k]} SGPRs"
