#!/usr/bin/env python3
"""Reads the literals of PnPsolver (src/PnPsolver.cc, include/PnPsolver.h) and of its call in Tracking::Relocalization (src/Tracking.cc) out of the reference text
into tests/golden/pnp_solver_constants.json: name, literal and file:line only.  tests/test_pnp_solver_reference_cpu.py holds the kernel's constant block
(eao_fusion_amd/csrc/pnp_internal.h), the yardstick (tests/pnp_solver_reference.py, tests/pnp_solver_scenes.py) and the adapter's defaults
(include/eaofusion/PnPsolver.h) to that file.

    python tools/gen_pnp_solver_constants.py <reference tree>          # writes the fixture
    python tools/gen_pnp_solver_constants.py <reference tree> --check  # compares, writes nothing
"""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "pnp_solver_constants.json")
NUM = r"([0-9.]+f?)"
_DEFAULTS = r"double probability = %s, int minInliers = %s , int maxIterations = %s, int minSet = %s, float epsilon = %s," % ((NUM,) * 5)
_RELOC = r"SetRansacParameters\(%s, %s, %s, %s, %s, %s\);" % ((NUM,) * 6)
# (name, file, line, the expression around the literal, the capture group that holds it)
SPEC = [
    ("GN_ITERATIONS", "src/PnPsolver.cc", 843, r"const int iterations_number = ([0-9]+);", 1),
    ("ALPHA_ONE", "src/PnPsolver.cc", 432, r"a\[0\] = " + NUM + r" - a\[1\] - a\[2\] - a\[3\];", 1),
    ("L_TWO", "src/PnPsolver.cc", 790, r"row\[1\] = " + NUM + r" \* dot\(dv\[0\]\[i\], dv\[1\]\[i\]\);", 1),
    ("L_TWO", "src/PnPsolver.cc", 792, r"row\[3\] = " + NUM + r" \* dot", 1),
    ("L_TWO", "src/PnPsolver.cc", 793, r"row\[4\] = " + NUM + r" \* dot", 1),
    ("L_TWO", "src/PnPsolver.cc", 795, r"row\[6\] = " + NUM + r" \* dot", 1),
    ("L_TWO", "src/PnPsolver.cc", 796, r"row\[7\] = " + NUM + r" \* dot", 1),
    ("L_TWO", "src/PnPsolver.cc", 797, r"row\[8\] = " + NUM + r" \* dot", 1),
    ("DEFAULT_PROBABILITY", "include/PnPsolver.h", 67, _DEFAULTS, 1),
    ("DEFAULT_MIN_INLIERS", "include/PnPsolver.h", 67, _DEFAULTS, 2),
    ("DEFAULT_MAX_ITERATIONS", "include/PnPsolver.h", 67, _DEFAULTS, 3),
    ("DEFAULT_MIN_SET", "include/PnPsolver.h", 67, _DEFAULTS, 4),
    ("DEFAULT_EPSILON", "include/PnPsolver.h", 67, _DEFAULTS, 5),
    ("DEFAULT_TH2", "include/PnPsolver.h", 68, r"float th2 = " + NUM + r"\);", 1),
    ("RELOC_PROBABILITY", "src/Tracking.cc", 2831, _RELOC, 1),
    ("RELOC_MIN_INLIERS", "src/Tracking.cc", 2831, _RELOC, 2),
    ("RELOC_MAX_ITERATIONS", "src/Tracking.cc", 2831, _RELOC, 3),
    ("RELOC_MIN_SET", "src/Tracking.cc", 2831, _RELOC, 4),
    ("RELOC_EPSILON", "src/Tracking.cc", 2831, _RELOC, 5),
    ("RELOC_TH2", "src/Tracking.cc", 2831, _RELOC, 6),
]


def parse(ref):
    text = {}
    out = []
    for name, rel, line, rx, group in SPEC:
        if rel not in text:
            text[rel] = open(os.path.join(ref, rel), errors="replace").read().split("\n")
        m = re.search(rx, text[rel][line - 1])
        if not m:
            raise SystemExit("%s:%d does not read `%s`" % (rel, line, rx))
        out.append({"name": name, "literal": m.group(group), "where": "%s:%d" % (rel, line)})
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
