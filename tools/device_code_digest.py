#!/usr/bin/env python3
"""Digest of the device code of a libhipk build: one line `symbol sha1 vgprs sgprs scratch lds` per gfx950 kernel, and
`symbol sha1 device function` per device function a kernel calls.

    python tools/device_code_digest.py LIB.so            # the lines, sorted by symbol
    python tools/device_code_digest.py LIB.so OTHER.so   # compare: the symbols that differ, then "N kernels and M device functions, K differ"

For a change that is meant to touch host code only: build the library before and after, compare.  The sha1 is taken over the
instruction encodings (llvm-objdump -d), pc-relative references resolved to the symbol they reach, so neither the order of the
kernels in a file nor their addresses enter; the four figures are the kernel's entry in the code object's metadata (what the
compiler's resource report prints).  Needs llvm-objdump and llvm-readelf of the ROCm LLVM directory (ROCM_LLVM_BIN; the offload
bundles are read directly), no GPU."""
import hashlib
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM_BIN", "/opt/rocm/llvm/bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def code_objects(lib, arch="gfx950"):
    """The `arch` ELF images of every offload bundle in `lib` (one bundle per translation unit)."""
    blob = open(lib, "rb").read()
    out, at = [], blob.find(MAGIC)
    while at >= 0:
        (count,) = struct.unpack_from("<Q", blob, at + len(MAGIC))
        pos = at + len(MAGIC) + 8
        for _ in range(count):
            off, size, tlen = struct.unpack_from("<QQQ", blob, pos)
            triple = blob[pos + 24:pos + 24 + tlen].decode()
            pos += 24 + tlen
            if arch in triple and size:
                out.append(blob[at + off:at + off + size])
        at = blob.find(MAGIC, at + len(MAGIC))
    if not out:
        raise SystemExit(f"{lib}: no uncompressed {arch} code object found")
    return out


def digest(lib):
    """{symbol: (sha1 of its instruction encodings, vgprs, sgprs, scratch bytes, lds bytes)}; a device function: (sha1, "device function")"""
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        for i, image in enumerate(code_objects(lib)):
            path = os.path.join(tmp, f"co{i}.elf")
            open(path, "wb").write(image)
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", path], capture_output=True, text=True, check=True).stdout
            meta = {}
            for blk in re.split(r"\n\s*- \.agpr_count:|\n\s*- \.args:", notes)[1:]:
                f = {k: v for k, v in re.findall(r"\.(symbol|vgpr_count|sgpr_count|private_segment_fixed_size|group_segment_fixed_size):\s*'?([^'\n]+)'?", blk)}
                if "symbol" in f:
                    meta[f["symbol"].removesuffix(".kd")] = tuple(int(f.get(k, -1)) for k in ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size"))
            # functions (kernels and the device functions they call) and data objects by address: a pc-relative reference
            # (s_getpc_b64 + s_add_u32 literal) is hashed as the symbol it reaches, not as the distance to it
            tab = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "-s", "-W", path], capture_output=True, text=True, check=True).stdout
            syms = sorted({(int(m.group(1), 16), int(m.group(2)), m.group(4)) for m in
                           re.finditer(r"^\s*\d+:\s+([0-9a-f]+)\s+(\d+)\s+(FUNC|OBJECT)\s+\S+\s+\S+\s+\d+\s+(\S+)$", tab, re.M)})
            funcs = {n for _, _, n in syms}

            def reach(addr):
                for lo, size, name in syms:
                    if lo <= addr < lo + max(size, 1):
                        return f"<{name}+{addr - lo}>"
                return f"<{addr:#x}>"

            dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", path], capture_output=True, text=True, check=True).stdout
            h, getpc = None, None
            for line in dis.splitlines():
                m = re.match(r"^[0-9a-f]+ <([^>]+)>:$", line)
                if m:
                    if m.group(1) in funcs:       # (branch-target labels inside a function, <L0> ..., are not symbols)
                        h = hashlib.sha1()
                        res[m.group(1)] = (h,) + meta.get(m.group(1), ("device function",))
                    continue
                m = re.search(r"^\s*(\S+).*//\s*([0-9A-Fa-f]+):\s*((?:[0-9A-Fa-f]{8}\s*)+)$", line)
                if not m or h is None:
                    continue
                op, addr, words = m.group(1), int(m.group(2), 16), m.group(3).split()
                if op == "s_add_u32" and getpc is not None and len(words) == 2:
                    lit = int(words[1], 16)
                    words[1] = reach(getpc + 4 + lit - (1 << 32 if lit >> 31 else 0))
                getpc = addr if op == "s_getpc_b64" else None
                h.update("".join(words).encode())
            missing = set(meta) - set(res)
            if missing:
                raise SystemExit(f"{lib}: kernels without disassembly: {sorted(missing)[:3]} ...")
    return {k: (v[0].hexdigest(),) + v[1:] for k, v in res.items()}


def main(argv):
    if len(argv) not in (2, 3):
        raise SystemExit(__doc__)
    a = digest(argv[1])
    if len(argv) == 2:
        for k in sorted(a):
            print(k, *a[k])
        return 0
    b = digest(argv[2])
    differ = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
    for k in differ:
        print(k, a.get(k, "absent"), b.get(k, "absent"))
    n = set(a) | set(b)
    print(f"{sum(len(a.get(k) or b[k]) > 2 for k in n)} kernels and {sum(len(a.get(k) or b[k]) == 2 for k in n)} device functions, {len(differ)} differ")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
