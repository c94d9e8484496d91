"""Register and scratch budgets of hipk_gm_batch_kernel<T, PRE> (csrc/hipk_batch_gm.hip, compiled for gfx950 here, the compiler's own
resource report read as tests/test_kernel_resources.py does; no GPU needed).

As for the other batch kernels, how many systems share a CU should be decided by their LDS (sized by n), not by registers: every
instantiation has no scratch, at most 128 VGPRs (four 256-thread workgroups per CU) and at most 80 SGPRs."""
import os
import shutil

import pytest

from test_kernel_resources import HIPCC, _vgprs

KERNELS = [f"void hipk_gm_batch_kernel<{t}, {pre}>" for t in ("double", "float") for pre in ("false", "true")]


@pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("c++filt") is None, reason="hipcc / c++filt not installed")
def test_gmres_batch_kernels_fit_four_workgroups_per_cu_without_scratch():
    got = _vgprs("hipk_batch_gm.hip")
    ours = {k: v for k, v in got.items() if "_batch_kernel<" in k}
    assert sorted(ours) == sorted(KERNELS), sorted(got)
    assert sorted(got) == sorted(KERNELS), "hipk_batch_gm.hip holds exactly these four kernels"
    for k, v in ours.items():
        print(f"{k}: {v} VGPRs, {_vgprs.sgprs[k]} SGPRs, {_vgprs.scratch[k]} bytes of scratch")
        assert _vgprs.scratch[k] == 0, f"{k}: {_vgprs.scratch[k]} bytes of scratch per lane"
        assert v <= 128, f"{k}: {v} VGPRs (> 128: fewer than four workgroups per CU)"
        assert _vgprs.sgprs[k] <= 80, f"{k}: {_vgprs.sgprs[k]} SGPRs"
