"""Register and scratch budgets of the level-scan kernels of csrc/hipk_mg_refresh.hip (compiled for gfx950 here, the compiler's own
resource report read as tests/test_mg_kernel_resources.py does; no GPU needed).

The scan streams a level's CSR arrays with a thread on VEC consecutive rows; the fold is one workgroup over at most 2048 pairs.  The
two instantiations of the scan and the fold have no scratch and at most 128 VGPRs, and they are the only kernels of the translation
unit: the Galerkin sums of a refresh go through hipk_mg_restrict_agg of hipk_mg_graph.hip, not through a second kernel here."""
import os
import shutil

import pytest

from test_kernel_resources import HIPCC, _vgprs

KERNELS = [f"void hipk_mg_level_scan_kernel<{t}>" for t in ("double", "float")] + ["hipk_mg_level_fold_kernel"]


@pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("c++filt") is None, reason="hipcc / c++filt not installed")
def test_mg_refresh_kernels_have_no_scratch_and_at_most_128_vgprs():
    got = _vgprs("hipk_mg_refresh.hip")
    assert sorted(k.split("(")[0] for k in got) == sorted(KERNELS), sorted(got)
    for k, v in got.items():
        print(f"{k}: {v} VGPRs, {_vgprs.sgprs[k]} SGPRs, {_vgprs.scratch[k]} bytes of scratch")
        assert _vgprs.scratch[k] == 0, f"{k}: {_vgprs.scratch[k]} bytes of scratch per lane"
        assert v <= 128, f"{k}: {v} VGPRs"
