#!/usr/bin/env python3
"""Reads the literals of Object_2D::NoParaDataAssociation out of the reference text into tests/golden/object_association_constants.json: name, literal and
file:line only.  tests/test_object_association_reference_cpu.py holds the header (include/eao_fusion.h), the host logic
(eao_fusion_amd/csrc/object_assoc_internal.h), the yardstick (tests/object_association_reference.py) and the scenes to that file.

    python tools/gen_object_association_constants.py <reference tree>          # writes the fixture
    python tools/gen_object_association_constants.py <reference tree> --check  # compares, writes nothing
"""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "object_association_constants.json")
REL = "src/Object.cc"
R1 = r"float r1 = %s \* m \* \(m \+ n \+ 1\) - %s \* sqrt\(m \* n \* \(m \+ n \+ 1\) / %s\);"
R2 = r"float r2 = %s \* m \* \(m \+ n \+ 1\) \+ %s \* sqrt\(m \* n \* \(m \+ n \+ 1\) / %s\);"
NUM, GRP = r"[0-9.]+", r"([0-9.]+)"
# (name, line, the expression around the literal with ONE capture group)
SPEC = [
    ("MIN_DET_POINTS", 760, r"if \(m < (\d+)\)"),
    ("MIN_MAP_POINTS", 764, r"if \(n < (\d+)\)"),
    ("SAMPLE_RATIO", 776, r"if \(n > (\d+) \* m\)"),
    ("SAMPLE_RATIO_N", 778, r"n = (\d+) \* m;"),
    ("HALF", 942, R1 % (GRP, NUM, NUM)),
    ("CRITICAL", 942, R1 % (NUM, GRP, NUM)),
    ("VARIANCE_DIVISOR", 942, R1 % (NUM, NUM, GRP)),
    ("HALF_R2", 943, R2 % (GRP, NUM, NUM)),
    ("CRITICAL_R2", 943, R2 % (NUM, GRP, NUM)),
    ("VARIANCE_DIVISOR_R2", 943, R2 % (NUM, NUM, GRP)),
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
