"""Register, scratch and LDS budgets of the W-cycle kernels of csrc/hipk_mg_w.hip (compiled for gfx950 here, the compiler's own
resource report read as tests/test_mg_kernel_resources.py does; no GPU needed).

The W tails are the V tails' steps under an iterative walk whose level and visit bits are uniform scalars: like their V twins they
have no scratch and at most 128 VGPRs, and they take no more LDS than those -- the gather vector of 4096 elements (32 KiB fp64,
16 KiB fp32), plus the 512 elements of r of a dense last level.  They and hipk_mg_add_kernel are the only kernels of the
translation unit."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from test_kernel_resources import CSRC, HIPCC, ROOT

LDS_TODAY = {   # bytes per workgroup of the V twins: hipk_mg_tail_kernel / hipk_mg_gtail_kernel, and hipk_mg_gtail_dense_kernel
    "void hipk_mg_tail_w_kernel<double, hipk_mg_level, hipk_mg_box_xf>": 4096 * 8,
    "void hipk_mg_tail_w_kernel<float, hipk_mg_level, hipk_mg_box_xf>": 4096 * 4,
    "void hipk_mg_tail_w_kernel<double, hipk_mg_glevel, hipk_mg_index_xf>": 4096 * 8,
    "void hipk_mg_tail_w_kernel<float, hipk_mg_glevel, hipk_mg_index_xf>": 4096 * 4,
    "void hipk_mg_gtail_dense_w_kernel<double>": (4096 + 512) * 8,
    "void hipk_mg_gtail_dense_w_kernel<float>": (4096 + 512) * 4,
    "void hipk_mg_add_kernel<double>": 0,
    "void hipk_mg_add_kernel<float>": 0,
}


def _report(src):
    """{demangled kernel name up to '(': {"vgprs", "sgprs", "scratch", "lds"}} from hipcc's -Rpass-analysis=kernel-resource-usage."""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", f"-I{os.path.join(ROOT, 'include')}", f"-I{CSRC}",
               "-Wno-unused-function", "-fno-gpu-rdc", "--cuda-device-only", "-c", os.path.join(CSRC, src), "-o", os.path.join(tmp, "x.o"),
               "-Rpass-analysis=kernel-resource-usage"]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    fields = {"vgprs": r"\bVGPRs: (\d+)", "sgprs": r"TotalSGPRs: (\d+)", "scratch": r"ScratchSize \[bytes/lane\]: (\d+)",
              "lds": r"LDS Size \[bytes/block\]: (\d+)"}
    got, name = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            got[name] = {}
        for key, pat in fields.items():
            m = re.search(pat, line)
            if m and name:
                got[name][key] = int(m.group(1))
    names = subprocess.run([shutil.which("c++filt")], input="\n".join(got), capture_output=True, text=True).stdout.splitlines()
    return {d.split("(")[0]: v for d, v in zip(names, got.values())}


@pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("c++filt") is None, reason="hipcc / c++filt not installed")
def test_w_kernels_have_no_scratch_at_most_128_vgprs_and_their_v_twins_lds():
    got = _report("hipk_mg_w.hip")
    assert sorted(got) == sorted(LDS_TODAY), sorted(got)
    for k, v in got.items():
        print(f"{k}: {v['vgprs']} VGPRs, {v['sgprs']} SGPRs, {v['scratch']} bytes of scratch, {v['lds']} bytes of LDS")
        assert v["scratch"] == 0, f"{k}: {v['scratch']} bytes of scratch per lane"
        assert v["vgprs"] <= 128, f"{k}: {v['vgprs']} VGPRs"
        assert v["lds"] <= LDS_TODAY[k], f"{k}: {v['lds']} bytes of LDS, the V twin has {LDS_TODAY[k]}"
