#!/usr/bin/env python3
"""Device code of two checkouts, kernel by kernel: every given .hip compiled in both trees with csrc/Makefile's flags plus --cuda-device-only -S and the same -cuid=,
then the instruction lines of every kernel / device function compared (comments and directives dropped, the per-function number of local labels .LBB<k>_<n> dropped).
A host-only change leaves every file identical.  Exit code 1 if one differs.

    python tools/isa_equal.py PARENT_TREE NEW_TREE sim3.hip keyframe.hip ...      (names under eao_fusion_amd/csrc/)
"""
import os
import re
import subprocess
import sys
import tempfile

FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-Wall", "-Wno-unused-function", "--cuda-device-only", "-S", "-cuid=isa_equal"]


def kernels(tree, name):
    """{symbol: [instruction lines]} of one source"""
    with tempfile.NamedTemporaryFile(suffix=".s") as f:
        subprocess.check_call(["/opt/rocm/bin/hipcc"] + FLAGS + [os.path.join(tree, "eao_fusion_amd", "csrc", name), "-o", f.name], stderr=subprocess.DEVNULL)
        lines = open(f.name).read().split("\n")
    out, cur = {}, None
    for l in lines:
        if re.match(r"_Z\w+:", l):
            cur = out.setdefault(l.split(":")[0], [])
        elif l.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None and l.startswith("\t") and not l.strip().startswith((".", ";")):
            cur.append(re.sub(r"\.LBB\d+_", ".LBB_", l.split(";")[0].strip()))
    return out


def main():
    parent, new, names = sys.argv[1], sys.argv[2], sys.argv[3:]
    differing = 0
    for name in sorted(names):
        a, b = kernels(parent, name), kernels(new, name)
        bad = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
        differing += bool(bad)
        print("%-22s %3d kernels / device functions, %7d instruction lines: %s" % (name, len(b), sum(len(v) for v in b.values()), "DIFFERENT: " + ", ".join(bad) if bad else "identical"))
    print("files with a difference: %d of %d" % (differing, len(names)))
    return 1 if differing else 0


if __name__ == "__main__":
    sys.exit(main())
