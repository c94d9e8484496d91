"""Register and scratch budgets of the value-plane rewrite of hipk_csr_update_values (csrc/hipk_coded.h: hipk_csr_revalue_rows_kernel,
hipk_csr_revalue_staged_kernel; compiled for gfx950 here, the compiler's own resource report read as tests/test_kernel_resources.py
does; no GPU needed).

Both forms are streaming kernels, one workgroup per 256-row tile, whose occupancy is to be bounded by LDS (the staged form) or by
nothing (the row form): no scratch, at most 64 VGPRs and 80 SGPRs -- eight 256-thread workgroups per CU as far as registers go.  The
two forms exist in both storage types and nowhere else: the re-encode of the pair-coded layouts runs the creation's own kernels."""
import os
import shutil

import pytest

from test_kernel_resources import HIPCC, _vgprs

KERNELS = [f"void hipk_csr_revalue_{form}_kernel<{t}>" for form in ("rows", "staged") for t in ("double", "float")]


@pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("c++filt") is None, reason="hipcc / c++filt not installed")
def test_revalue_kernels_have_no_scratch_and_keep_eight_workgroups_per_cu():
    got = _vgprs("hipk_api.hip")
    mine = sorted(k for k in got if "hipk_csr_revalue" in k)
    assert sorted(k.split("(")[0] for k in mine) == sorted(KERNELS), mine
    for k in mine:
        print(f"{k}: {got[k]} VGPRs, {_vgprs.sgprs[k]} SGPRs, {_vgprs.scratch[k]} bytes of scratch")
        assert _vgprs.scratch[k] == 0, f"{k}: {_vgprs.scratch[k]} bytes of scratch per lane"
        assert got[k] <= 64, f"{k}: {got[k]} VGPRs"
        assert _vgprs.sgprs[k] <= 80, f"{k}: {_vgprs.sgprs[k]} SGPRs"
