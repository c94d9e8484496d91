"""The Chebyshev step kernels are budgeted like the product kernels they sit beside (tests/test_kernel_resources.py): at most 64
VGPRs and 80 SGPRs, so that eight 256-thread workgroups stay resident per CU, and no scratch.  Compiles csrc/hipk_api.hip for gfx950
and reads the compiler's resource report (no GPU needed).  The product instantiations themselves are pinned by
tests/test_kernel_resources.py: the epilogue is a template flag (tile kernel) / a compiled-in MODE value (two-rows-per-lane
kernel), so they compile to what they were."""
import os
import shutil

import pytest

from test_kernel_resources import HIPCC, _vgprs

CHEB = ["void hipk_spmv_sell_wide_kernel<5, 28, 0>", "void hipk_spmv_sell_wide_kernel<5, 28, 1>",      # the headline matrix's
        "void hipk_spmv_sell_wide_kernel<4, 28, 0>", "void hipk_spmv_sell_wide_kernel<4, 28, 1>",
        "void hipk_spmv_sell_wide_kernel<8, 28, 0>", "void hipk_spmv_sell_wide_kernel<8, 28, 1>",
        "void hipk_spmv_cheb_kernel<double, 1280>", "void hipk_spmv_cheb_kernel<double, 2048>",
        "void hipk_spmv_cheb_kernel<float, 2048>",
        "void hipk_cheb_step_kernel<double>", "void hipk_cheb_step_kernel<float>",
        "void hipk_cheb_init_kernel<double>", "void hipk_cheb_init_kernel<float>"]


@pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("c++filt") is None, reason="hipcc / c++filt not installed")
def test_chebyshev_kernels_keep_eight_workgroups_per_cu():
    got = _vgprs("hipk_api.hip")
    for k in CHEB:
        assert k in got, (k, sorted(got)[:80])
        assert got[k] <= 64, f"{k}: {got[k]} VGPRs"
        assert _vgprs.sgprs[k] <= 80, f"{k}: {_vgprs.sgprs[k]} SGPRs"
        assert _vgprs.scratch[k] == 0, f"{k}: {_vgprs.scratch[k]} bytes of scratch per lane"
