"""Register and scratch budgets of the block kernels of csrc/hipk_multi.hip (compiled for gfx950 here, the compiler's own resource
report read as tests/test_kernel_resources.py does; no GPU needed).

Budgets:
  * no scratch in any of them: a spill would put per-lane stack traffic on kernels that exist to stream the block once;
  * at most 128 VGPRs (four wavefronts per SIMD) for the instantiations of up to 8 columns of the block SpMV, the CG update and
    direction steps and the BiCGStab s-step: they hide gather and stream latency with resident wavefronts, and the k = 8 block
    is the case the block path is measured on (fp64 at 8 columns compiles to 70 / 90 / 112 / 103);
  * at most 256 VGPRs for every instantiation (16 columns of fp64 in flight per row: two wavefronts per SIMD, still no spill).
"""
import os
import shutil

import pytest

from test_kernel_resources import HIPCC, _vgprs

FOUR_WAVES = ["void hipk_mspmv_kernel<double, 8, false>", "void hipk_mspmv_kernel<double, 4, false>",
              "void hipk_mspmv_kernel<double, 2, false>", "void hipk_mspmv_kernel<double, 8, true>",
              "void hipk_mcg_update_kernel<double, 8, false>", "void hipk_mcg_update_kernel<double, 8, true>",
              "void hipk_mcg_direction_kernel<double, 8, false>", "void hipk_mcg_update_kernel<float, 8, false>",
              "void hipk_mcg_direction_kernel<float, 8, false>", "void hipk_mbi_supdate_kernel<double, 8, false>",
              "void hipk_mbi_direction_kernel<double, 8, false>", "void hipk_mcombine_kernel<8>", "void hipk_mdot_kernel<double, 8>"]


@pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("c++filt") is None, reason="hipcc / c++filt not installed")
def test_block_kernels_fit_their_register_budgets_without_scratch():
    got = _vgprs("hipk_multi.hip")
    ours = {k: v for k, v in got.items() if "hipk_m" in k}
    assert len(ours) >= 100, sorted(got)   # 4 widths x 2 dtypes x (SpMV, CG, BiCGStab, dots, folds)
    for k, v in ours.items():
        assert _vgprs.scratch[k] == 0, f"{k}: {_vgprs.scratch[k]} bytes of scratch per lane"
        assert v <= 256, f"{k}: {v} VGPRs"
    for k in FOUR_WAVES:
        assert got[k] <= 128, f"{k}: {got[k]} VGPRs (> 128: fewer than four wavefronts per SIMD)"
