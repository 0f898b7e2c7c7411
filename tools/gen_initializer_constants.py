#!/usr/bin/env python3
"""Reads the literals of Initializer (src/Initializer.cc) out of the reference text into tests/golden/initializer_constants.json: name, literal and file:line only.
tests/test_initializer_reference_cpu.py holds the kernel's constant block (eao_fusion_amd/csrc/initializer.hip), the yardstick (tests/initializer_reference.py, which
reads the fixture) and the adapter's defaults (include/eaofusion/Initializer.h) to that file.

    python tools/gen_initializer_constants.py <reference tree>          # writes the fixture
    python tools/gen_initializer_constants.py <reference tree> --check  # compares, writes nothing
"""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "initializer_constants.json")
REL = "src/Initializer.cc"
# (name, line, the expression around the literal with ONE capture group)
SPEC = [
    ("RATIO_H", 115, r"if\(RH>([0-9.]+)\)"),
    ("MIN_PARALLAX", 116, r"ReconstructH\(.*vbTriangulated,([0-9.]+),[0-9]+\)"),
    ("MIN_TRIANGULATED", 116, r"ReconstructH\(.*vbTriangulated,[0-9.]+,([0-9]+)\)"),
    ("MIN_PARALLAX", 118, r"ReconstructF\(.*vbTriangulated,([0-9.]+),[0-9]+\)"),
    ("MIN_TRIANGULATED", 118, r"ReconstructF\(.*vbTriangulated,[0-9.]+,([0-9]+)\)"),
    ("CHI2_H", 333, r"const float th = ([0-9.]+);"),
    ("CHI2_F", 408, r"const float th = ([0-9.]+);"),
    ("CHI2_SCORE", 409, r"const float thScore = ([0-9.]+);"),
    ("REPROJ_FACTOR", 494, r"vP3D1, ([0-9.]+)\*mSigma2"),
    ("MIN_GOOD_FRACTION", 504, r"static_cast<int>\(([0-9.]+)\*N\)"),
    ("SIMILAR", 507, r"nGood1>([0-9.]+)\*maxGood"),
    ("DEGENERATE", 597, r"d1/d2<([0-9.]+) \|\| d2/d3<\1\)"),
    ("REPROJ_FACTOR", 703, r"vP3Di, ([0-9.]+)\*mSigma2"),
    ("SECOND_BEST", 721, r"secondBestGood<([0-9.]+)\*bestGood"),
    ("MIN_GOOD_FRACTION", 721, r"bestGood>([0-9.]+)\*N\)"),
    ("COS_PARALLAX", 857, r"cosParallax<([0-9.]+)\)"),
    ("COS_PARALLAX", 863, r"cosParallax<([0-9.]+)\)"),
    ("COS_PARALLAX", 892, r"cosParallax<([0-9.]+)\)"),
    ("PARALLAX_RANK", 900, r"min\(([0-9]+),int\(vCosParallax\.size\(\)-1\)\)"),
]


def parse(ref):
    lines = open(os.path.join(ref, REL), errors="replace").read().split("\n")
    out = []
    for name, line, rx in SPEC:
        m = re.search(rx, lines[line - 1])
        if not m:
            raise SystemExit("%s:%d does not read `%s`" % (REL, line, rx))
        out.append({"name": name, "literal": m.group(1), "where": "%s:%d" % (REL, line)})
    by = {}
    for c in out:
        if by.setdefault(c["name"], c["literal"]) != c["literal"]:
            raise SystemExit("%s is spelled two ways in the reference text" % c["name"])
    return out


def main():
    if len(sys.argv) < 2:
        raise SystemExit(__doc__)
    got = {"constants": parse(sys.argv[1])}
    if "--check" in sys.argv:
        want = json.load(open(OUT))
        if want != got:
            raise SystemExit("fixture and reference text differ")
        print("ok")
        return
    with open(OUT, "w") as f:
        json.dump(got, f, indent=1)
        f.write("\n")
    print("wrote", OUT)


if __name__ == "__main__":
    main()
