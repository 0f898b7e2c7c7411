#!/usr/bin/env python3
"""Reads the literals of Object_Map::IsolationForestDeleteOutliers out of the reference text into tests/golden/isolation_forest_constants.json: name, literal
and file:line only.  tests/test_isolation_forest_reference_cpu.py holds the header (include/eao_fusion.h), the host logic (eao_fusion_amd/csrc/iforest_internal.h),
the yardstick (tests/isolation_forest_reference.py) and the scenes to that file.

    python tools/gen_isolation_forest_constants.py <reference tree>          # writes the fixture
    python tools/gen_isolation_forest_constants.py <reference tree> --check  # compares, writes nothing
"""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "isolation_forest_constants.json")
REL = "src/Object.cc"
# (name, line, the expression around the literal with ONE capture group)
SPEC = [
    ("EXEMPT_CLASS_A", 1245, r"\(this->mnClass == (\d+)\) \|\| \(this->mnClass == \d+\) \|\| \(this->mnClass == \d+\)"),
    ("EXEMPT_CLASS_B", 1245, r"\(this->mnClass == \d+\) \|\| \(this->mnClass == (\d+)\) \|\| \(this->mnClass == \d+\)"),
    ("EXEMPT_CLASS_C", 1245, r"\(this->mnClass == \d+\) \|\| \(this->mnClass == \d+\) \|\| \(this->mnClass == (\d+)\)"),
    ("THRESHOLD", 1248, r"float th = ([0-9.]+);"),
    ("THRESHOLD_CLASS", 1249, r"if \(this->mnClass == (\d+)\)"),
    ("THRESHOLD_OF_CLASS", 1250, r"th = ([0-9.]+);"),
    ("MIN_POINTS", 1256, r"mvpMapObjectMappoints.size\(\) < (\d+)\)"),
    ("TREE_COUNT", 1296, r"forest.Build\((\d+), \d+, data,"),
    ("SEED", 1296, r"forest.Build\(\d+, (\d+), data,"),
    ("SAMPLE_DIVISOR", 1296, r"\(\(int\)mvpMapObjectMappoints.size\(\) / (\d+)\)"),
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
