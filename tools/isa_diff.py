#!/usr/bin/env python
"""Which device functions of a kernel file compile to other instructions in another copy of the sources: compiles FILE.hip of two csrc directories for
gfx950 (device side, the product's flags, extra flags after --) and compares every function instruction by instruction, registers included
(labels and comments stripped).  A function that is identical computes the same bits at the same speed.
    python tools/isa_diff.py OTHER_CSRC_DIR pv_wg_kernel.hip [pv_wave_kernel.hip ...] [-- -DPV_FP64_FLAVOUR=1]"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def functions(csrc, source, extra):
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "a.s")
        subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "--offload-arch=gfx950", "--cuda-device-only", "-I.", "-S", *extra, source, "-o", out],
                       cwd=csrc, check=True, stderr=subprocess.DEVNULL)
        text = open(out).read()
    found = {}
    for m in re.finditer(r"\n(_Z\w+):[^\n]*\n(.*?)\.Lfunc_end", text, re.S):
        body = []
        for line in m.group(2).split("\n"):
            line = re.sub(r"\s*;.*", "", line).strip()
            if line and (not line.startswith(".") or line.startswith(".LBB")):
                body.append(re.sub(r"\.LBB\d+_\d+", ".L", line))
        found[m.group(1)] = body
    return found


def main():
    args, extra = sys.argv[1:], []
    if "--" in args:
        extra, args = args[args.index("--") + 1:], args[:args.index("--")]
    other, total, same = args[0], 0, 0
    for source in args[1:]:
        a, b = functions(other, source, extra), functions(os.path.join(ROOT, "phaze_amd", "csrc"), source, extra)
        differ = sorted(k for k in a if k in b and a[k] != b[k])
        total, same = total + len(a), same + len([k for k in a if k in b and a[k] == b[k]])
        print(f"{source}: {len(a)} functions, {len(differ)} differ, {len(set(a) - set(b))} only there, {len(set(b) - set(a))} only here")
        for k in differ:
            print(f"   {k}: {len(a[k])} -> {len(b[k])} instructions")
    print(f"{same} of {total} functions are instruction-identical")


if __name__ == "__main__":
    main()
