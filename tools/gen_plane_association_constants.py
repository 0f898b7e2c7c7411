#!/usr/bin/env python3
"""Reads the three literals of the plane association out of the reference text into tests/golden/plane_association_constants.json: name, literal and file:line
only.  tests/test_plane_association_reference_cpu.py holds the header (include/eao_fusion.h), the kernel's constants (eao_fusion_amd/csrc/plane_map_internal.h),
the yardstick (tests/plane_association_reference.py), the Python mirror and the adapter (include/eaofusion/MapPlanes.h) to that file.

    python tools/gen_plane_association_constants.py <reference tree>          # writes the fixture
    python tools/gen_plane_association_constants.py <reference tree> --check  # compares, writes nothing
"""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "plane_association_constants.json")
REL = "src/Map.cc"
# (name, line, the expression around the literal with ONE capture group)
SPEC = [
    ("DIS_TH", 22, r"mfDisTh = ([0-9.]+);"),
    ("ANGLE_TH", 23, r"mfAngleTh = ([0-9.]+);"),
    ("NO_DISTANCE", 219, r"double res = ([0-9.]+);"),
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
