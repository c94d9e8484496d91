"""The kernels of the row-partitioned Chebyshev CG (csrc/hipk_dist_cheb.h, compiled into csrc/hipk_cg.hip) in the gfx950 code
object: the fused update + step 0 kernel is budgeted like the CG vector kernels it replaces (tests/test_kernel_resources.py: at
most 64 VGPRs and 80 SGPRs, eight workgroups per CU), neither new kernel uses scratch.  The apply reuses the SpMV instantiations:
that csrc/hipk_api.hip keeps its 128 hipk_spmv_* kernels is pinned by tests/test_spmv_cases.py.  Reads the compiler's resource
report, no GPU needed."""
import os
import shutil

import pytest

from test_kernel_resources import HIPCC, _vgprs

NEW = ["void hipk_cheb_update_kernel<double>", "void hipk_cheb_ghost0_kernel<double>"]


@pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("c++filt") is None, reason="hipcc / c++filt not installed")
def test_row_partitioned_chebyshev_kernels_fit_without_scratch():
    got = _vgprs("hipk_cg.hip")
    for k in NEW:
        assert k in got, (k, sorted(got)[:80])
        assert got[k] <= 64, f"{k}: {got[k]} VGPRs"
        assert _vgprs.sgprs[k] <= 80, f"{k}: {_vgprs.sgprs[k]} SGPRs"
        assert _vgprs.scratch[k] == 0, f"{k}: {_vgprs.scratch[k]} bytes of scratch per lane"

