#!/usr/bin/env python3
"""Reads the four literals of the triangulation loop of LocalMapping::CreateNewMapPoints out of the reference text into
tests/golden/triangulation_constants.json: name, literal and file:line only.  tests/test_triangulation_reference_cpu.py holds the kernel's constant block
(eao_fusion_amd/csrc/triangulate.hip), the yardstick (tests/triangulation_reference.py) and the adapter (include/eaofusion/LocalMapping.h) to that file.

    python tools/gen_triangulation_constants.py <reference tree>          # writes the fixture
    python tools/gen_triangulation_constants.py <reference tree> --check  # compares, writes nothing
"""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "triangulation_constants.json")
REL = "src/LocalMapping.cc"
# (name, line, the expression around the literal with ONE capture group)
SPEC = [
    ("RATIO_FACTOR_BASE", 236, r"ratioFactor = ([0-9.]+)f\*mpCurrentKeyFrame->mfScaleFactor"),
    ("LOW_PARALLAX_COS", 323, r"cosParallaxRays<([0-9.]+)\)"),
    ("CHI2_MONO", 378, r"\(errX1\*errX1\+errY1\*errY1\)>([0-9.]+)\*sigmaSquare1"),
    ("CHI2_STEREO", 389, r"\+errX1_r\*errX1_r\)>([0-9.]+)\*sigmaSquare1"),
    ("CHI2_MONO", 404, r"\(errX2\*errX2\+errY2\*errY2\)>([0-9.]+)\*sigmaSquare2"),
    ("CHI2_STEREO", 415, r"\+errX2_r\*errX2_r\)>([0-9.]+)\*sigmaSquare2"),
]


def parse(ref):
    lines = open(os.path.join(ref, REL), errors="replace").read().split("\n")
    out = []
    for name, line, rx in SPEC:
        m = re.search(rx, lines[line - 1])
        if not m:
            raise SystemExit("%s:%d does not read `%s`" % (REL, line, rx))
        out.append({"name": name, "literal": m.group(1), "where": "%s:%d" % (REL, line)})
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
