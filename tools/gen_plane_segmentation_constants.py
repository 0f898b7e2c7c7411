#!/usr/bin/env python3
"""Reads every literal of the plane segmentation out of the reference text into tests/golden/plane_segmentation_constants.json: name, literal and file:line only.
tests/test_plane_segmentation_reference_cpu.py holds the yardstick (tests/plane_segmentation_reference.py), the host header
(eao_fusion_amd/csrc/plane_seg_internal.h) and eao_plane_seg_cfg_default (eao_fusion_amd/csrc/plane_seg.hip) to that file.

    python tools/gen_plane_segmentation_constants.py <reference tree>          # writes the fixture
    python tools/gen_plane_segmentation_constants.py <reference tree> --check  # compares, writes nothing
"""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "plane_segmentation_constants.json")
FRAME, FITTER, PARAMS = "src/Frame.cc", "include/PEAC/AHCPlaneFitter.hpp", "include/PEAC/AHCParamSet.hpp"
N = r"([0-9.e+-]+)"
# (name, file, line, the expression around the literal with ONE capture group)
SPEC = [
    ("DEPTH_MAX", FRAME, 396, r"d > " + N + r" \|\|"),
    ("DEPTH_MIN", FRAME, 396, r"d < " + N + r" \)"),
    ("LEAF", FRAME, 436, r"setLeafSize\(" + N + r","),
    ("SEEN_DIST", FRAME, 362, r"d > " + N + r" \|\|"),
    ("SEEN_ANGLE", FRAME, 365, r"angle < " + N + r" &&"),
    ("MAX_STEP", FITTER, 153, r"maxStep\(" + N + r"\)"),
    ("MIN_SUPPORT", FITTER, 153, r"minSupport\(" + N + r"\)"),
    ("WINDOW", FITTER, 154, r"windowWidth\(" + N + r"\)"),
    ("WINDOW_HEIGHT", FITTER, 154, r"windowHeight\(" + N + r"\)"),
    ("TRAIL_STOP", FITTER, 443, r"trail<=(-[0-9]+)\)"),
    ("DIST_FACTOR", FITTER, 453, r"<([0-9]+)\*pl\.mse"),
    ("DIST_EPS", FITTER, 453, r"pl\.mse\+" + N + r"\)"),
    ("DEPTH_SIGMA", PARAMS, 68, r"depthSigma\(" + N + r"\)"),
    ("STD_TOL_INIT", PARAMS, 69, r"stdTol_init\(" + N + r"\)"),
    ("STD_TOL_MERGE", PARAMS, 69, r"stdTol_merge\(" + N + r"\)"),
    ("Z_NEAR", PARAMS, 70, r"z_near\(" + N + r"\)"),
    ("Z_FAR", PARAMS, 70, r"z_far\(" + N + r"\)"),
    ("ANGLE_NEAR_DEG", PARAMS, 71, r"angle_near\(MACRO_DEG2RAD\(" + N + r"\)\)"),
    ("ANGLE_FAR_DEG", PARAMS, 71, r"angle_far\(MACRO_DEG2RAD\(" + N + r"\)\)"),
    ("SIMILARITY_MERGE_DEG", PARAMS, 72, r"similarityTh_merge\(std::cos\(MACRO_DEG2RAD\(" + N + r"\)\)\)"),
    ("SIMILARITY_REFINE_DEG", PARAMS, 73, r"similarityTh_refine\(std::cos\(MACRO_DEG2RAD\(" + N + r"\)\)\)"),
    ("DEPTH_ALPHA", PARAMS, 74, r"depthAlpha\(" + N + r"\)"),
    ("DEPTH_CHANGE_TOL", PARAMS, 74, r"depthChangeTol\(" + N + r"\)"),
]


def parse(ref):
    text = {}
    out = []
    for name, rel, line, rx in SPEC:
        if rel not in text:
            text[rel] = open(os.path.join(ref, rel), errors="replace").read().split("\n")
        m = re.search(rx, text[rel][line - 1])
        if not m:
            raise SystemExit("%s:%d does not read `%s`" % (rel, line, rx))
        out.append({"name": name, "literal": m.group(1), "where": "%s:%d" % (rel, line)})
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
