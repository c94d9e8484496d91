"""Resources of hipk_csr_vgrad_kernel (csrc/hipk_vgrad.hip), compiled for gfx950 here and read from the compiler's own report as
tests/test_kernel_resources.py does; no GPU needed.

The kernel is an entry-parallel stream, so it is to run eight 256-thread workgroups per CU: no scratch (the four (row, col) pairs a
thread keeps are unrolled registers, not an indexed array), at most 64 VGPRs and 80 SGPRs, and the LDS the design states: the tile's
257 row pointers (1028 bytes, rounded to the alignment of T) and the lam tiles of a slice of 8 systems (8 x 256 values)."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from test_kernel_resources import CSRC, HIPCC, ROOT

LDS = {"double": 1032 + 8 * 256 * 8, "float": 1028 + 8 * 256 * 4}


def _report(src):
    """{demangled kernel name up to '(': {'vgprs', 'sgprs', 'scratch', 'lds'}} of one translation unit."""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", f"-I{os.path.join(ROOT, 'include')}", f"-I{CSRC}",
               "-Wno-unused-function", "-fno-gpu-rdc", "--cuda-device-only", "-c", os.path.join(CSRC, src), "-o", os.path.join(tmp, "x.o"),
               "-Rpass-analysis=kernel-resource-usage"]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    keys = {"vgprs": r"\bVGPRs: (\d+)", "sgprs": r"TotalSGPRs: (\d+)", "scratch": r"ScratchSize \[bytes/lane\]: (\d+)",
            "lds": r"LDS Size \[bytes/block\]: (\d+)"}
    out, name = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
        for k, pat in keys.items():
            m = re.search(pat, line)
            if m and name:
                out[name][k] = int(m.group(1))
    names = subprocess.run([shutil.which("c++filt")], input="\n".join(out), capture_output=True, text=True).stdout.splitlines()
    return {d.split("(")[0]: v for d, v in zip(names, out.values())}


@pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("c++filt") is None, reason="hipcc / c++filt not installed")
def test_vgrad_kernels_run_eight_workgroups_per_cu_without_scratch():
    got = _report("hipk_vgrad.hip")
    assert sorted(got) == sorted(f"void hipk_csr_vgrad_kernel<{t}>" for t in LDS), sorted(got)
    for t, lds in LDS.items():
        r = got[f"void hipk_csr_vgrad_kernel<{t}>"]
        print(f"hipk_csr_vgrad_kernel<{t}>: {r}")
        assert r["scratch"] == 0, f"{t}: {r['scratch']} bytes of scratch per lane"
        assert r["vgprs"] <= 64, f"{t}: {r['vgprs']} VGPRs (> 64: fewer than eight workgroups per CU)"
        assert r["sgprs"] <= 80, f"{t}: {r['sgprs']} SGPRs (> 80: the hardware admits fewer than eight workgroups per CU)"
        assert r["lds"] == lds, f"{t}: {r['lds']} bytes of LDS, the design states {lds}"
        assert 8 * r["lds"] <= 160 * 1024
