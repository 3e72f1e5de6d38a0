#!/usr/bin/env python3
"""Per-kernel comparison of the gfx950 code objects of two builds of libputslam_hip.so: which symbols exist in one only and
which common symbols differ in their disassembly (addresses, raw bytes and comments dropped).  For a change that only moves
code every common symbol must come out identical.

    python3 profiles/scripts/kernel_diff.py A.so B.so
"""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/lib/llvm/bin")


def kernels(lib):
    with tempfile.TemporaryDirectory() as d:
        fat, co = os.path.join(d, "fat.bin"), os.path.join(d, "dev.co")
        subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, lib, os.path.join(d, "copy.so")])
        subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat,
                               "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co])
        asm = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co], text=True)
    out, name = {}, None
    for line in asm.splitlines():
        m = re.match(r"^[0-9a-f]+ <([^>]+)>:", line)
        if m:
            name = m.group(1)
            out[name] = []
        elif name is not None:
            text = line.split("//")[0].strip()
            if text:
                out[name].append(text)
    return out


def demangle(names):
    if not names:
        return []
    return subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")[:len(names)]


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    common = sorted(set(a) & set(b))
    differ = [n for n in common if a[n] != b[n]]
    print("symbols: %d in A, %d in B, %d common, %d identical, %d differ" % (len(a), len(b), len(common), len(common) - len(differ), len(differ)))
    for title, names in (("only in A", only_a), ("only in B", only_b), ("differ", differ)):
        for n in demangle(names):
            print("  %s: %s" % (title, n))
    return 0


if __name__ == "__main__":
    sys.exit(main())
