"""Register and scratch budgets of the batch kernels of csrc/hipk_batch.hip (compiled for gfx950 here, the compiler's own resource
report read as tests/test_kernel_resources.py does; no GPU needed).

One 256-thread workgroup owns one small system, and how many systems share a CU should be decided by their LDS (sized by n), not by
registers.  So every instantiation of hipk_cg_batch_kernel<T, PRE> and hipk_bi_batch_kernel<T, PRE> has
  * no scratch (its per-thread arrays are register arrays with compile-time indices),
  * at most 128 VGPRs: four 256-thread workgroups per CU,
  * at most 80 SGPRs (beyond that the hardware admits fewer workgroups than the occupancy figure says).
"""
import os
import shutil

import pytest

from test_kernel_resources import HIPCC, _vgprs

KERNELS = [f"void hipk_{k}_batch_kernel<{t}, {pre}>" for k in ("cg", "bi") for t in ("double", "float") for pre in ("false", "true")]


@pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("c++filt") is None, reason="hipcc / c++filt not installed")
def test_batch_kernels_fit_four_workgroups_per_cu_without_scratch():
    got = _vgprs("hipk_batch.hip")
    ours = {k: v for k, v in got.items() if "_batch_kernel<" in k}
    assert sorted(ours) == sorted(KERNELS), sorted(got)
    for k, v in ours.items():
        print(f"{k}: {v} VGPRs, {_vgprs.sgprs[k]} SGPRs, {_vgprs.scratch[k]} bytes of scratch")
        assert _vgprs.scratch[k] == 0, f"{k}: {_vgprs.scratch[k]} bytes of scratch per lane"
        assert v <= 128, f"{k}: {v} VGPRs (> 128: fewer than four workgroups per CU)"
        assert _vgprs.sgprs[k] <= 80, f"{k}: {_vgprs.sgprs[k]} SGPRs"
