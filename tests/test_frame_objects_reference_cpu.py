"""The yardstick of a frame's 2D objects (tests/frame_objects_reference.py) against itself and its recorded results, without a device and without a tolerance:
every scene reaches the branch it was made for, upstream's literal form (push_back, sort, erase) and the compact form the device runs agree, the recorded
results (tests/golden/frame_objects/results.npz, tools/gen_golden_frame_objects.py) are what the yardstick computes, the variant condition -- plain IEEE
sum / (float)n against the convertTo reading of cv::Mat / n -- is reported per scene, and the literals are the reference's."""
import os
import re
import sys

import numpy as np
import pytest

import frame_objects_reference as Y
import frame_objects_scenes as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden_frame_objects as GG  # noqa: E402
import reference_literals as RL  # noqa: E402

SCENES = SC.scenes()
NAMES = sorted(SCENES)
_res = {}


def results(name):
    if name not in _res:
        _res[name] = (Y.literal(SCENES[name][0]), Y.compact(SCENES[name][0]))
    return _res[name]


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "frame_objects", "results.npz"))


@pytest.mark.parametrize("name", NAMES)
def test_scene_reaches_its_branch_and_the_forms_agree(name, gold):
    lit, com = results(name)
    assert SCENES[name][1](lit) and SCENES[name][1](com)
    assert Y.same(lit, com, zero_signs=False)
    assert lit["variant"] == com["variant"]
    rec = GG.unpack(gold, name)
    assert Y.same(com, rec) and rec["variant"] == com["variant"]


def test_the_golden_file_holds_the_scenes_and_nothing_else(gold):
    assert {k.rsplit(".", 1)[0] for k in gold.files} == set(NAMES)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "frame_objects", "results.npz")) < 256 * 1024


def test_the_forms_differ_only_in_the_sign_of_a_zero_quartile():
    """where -0.0f and +0.0f tie at Q1 the sort takes one and the rank count the other; max_th and every `z > max_th` verdict are the same for either sign"""
    lit, com = results("zero_signs_at_quartile")
    assert not Y.same(lit, com) and Y.same(lit, com, zero_signs=False)
    assert np.signbit(com["records"]["q1"][0]) and not np.signbit(lit["records"]["q1"][0])
    assert [n for n in NAMES if not Y.same(*results(n))] == ["zero_signs_at_quartile"]
    fr = SCENES["zero_signs_at_quartile"][0]
    z = [Y.camera_row(np.asarray(fr["Tcw"], np.float32), 2, p) for p in np.asarray(fr["mp_xyz"], np.float32)]
    assert any(np.signbit(v) and v == 0 for v in z) and any(not np.signbit(v) and v == 0 for v in z)
    for res in (lit, com):
        assert Y.zero_sign_invariant(z, res["records"]["q1"][0], res["records"]["q3"][0])
    zero, one = np.float32(0.0), np.float32(1.0)
    for q1, q3 in ((zero, zero), (-zero, zero), (zero, one), (-one, zero), (-one, -zero)):      # every place a zero can take
        assert Y.zero_sign_invariant([-one, -zero, zero, one, np.float32(1.5), np.float32(2.5)], q1, q3)


def test_the_variant_condition_is_reported(gold):
    """the scenes in which plain IEEE division gives another _Pos than src * (float)(1.0 / n): recorded, so that a change of either reading shows"""
    differing = [n for n in NAMES if any(results(n)[1]["variant"])]
    assert differing == [n for n in NAMES if gold[n + ".variant"].any()]
    assert "timing_shape" in differing and "ties_to_even" not in differing      # both outcomes occur
    print("plain sum / (float)n differs from the convertTo reading in %d of %d scenes: %s" % (len(differing), len(NAMES), ", ".join(differing)))
    # a power-of-two count cannot differ: 1.0 / n is exact
    for n in NAMES:
        lit = results(n)[0]
        for k, v in enumerate(lit["variant"]):
            c = int(lit["records"]["n"][k])
            if c > 0 and c & (c - 1) == 0:
                assert not v, (n, k)


def test_the_inner_boxplot_gate():
    """src/Object.cc:131 returns for n = 1 .. 4 and lets 5 .. 7 through; behind the `>= 8` gate of src/Tracking.cc:1782 it never fires"""
    assert [Y.boxplot_gate(n) for n in range(1, 8)] == [True] * 4 + [False] * 3
    assert not any(Y.boxplot_gate(n) for n in range(Y.BOXPLOT_MIN_POINTS, Y.MAX_KEYPOINTS + 1))


def test_the_literals_are_the_references():
    lit = RL.literals("frame_objects")
    mine = dict(BOXPLOT_MIN_POINTS=Y.BOXPLOT_MIN_POINTS, QUARTILE_DIVISOR=Y.QUARTILE_DIVISOR, IQR_FACTOR=Y.IQR_FACTOR, CROWD_RATIO=Y.CROWD_RATIO,
                CROWD_MAX=Y.CROWD_MAX, LARGE_AREA_RATIO=Y.LARGE_AREA_RATIO, FEW_POINTS=Y.FEW_POINTS, FEW_POINTS_ON_EDGE=Y.FEW_POINTS_ON_EDGE,
                FEW_POINTS_EDGE_PIXELS=Y.FEW_POINTS_EDGE_PIXELS, ON_EDGE_PIXELS=Y.ON_EDGE_PIXELS, SAME_OBJECT_IOU=Y.SAME_OBJECT_IOU, SURROUND_IOU=Y.SURROUND_IOU,
                SURROUND_RATIO=Y.SURROUND_RATIO, FEATURE_RECT_MIN_POINTS=Y.FEATURE_RECT_MIN_POINTS)
    assert set(mine) == set(lit) and all(float(lit[k]) == float(v) for k, v in mine.items())
    # the host header spells them as the reference does
    h = open(os.path.join(ROOT, "eao_fusion_amd", "csrc", "frame_objects_internal.h")).read()
    camel = {k: "k" + "".join(w.capitalize() for w in k.split("_")) for k in lit}
    for k, name in camel.items():
        m = re.search(r"constexpr (?:int32_t|double) %s = ([0-9.]+);" % name, h)
        assert m and m.group(1) == lit[k], (k, name)


def test_refusal_bounds_are_the_headers():
    hdr = open(os.path.join(ROOT, "include", "eao_fusion.h")).read()
    assert "#define EAO_FRAME_OBJECTS_MAX_KEYPOINTS %d\n" % Y.MAX_KEYPOINTS in hdr and "#define EAO_FRAME_OBJECTS_MAX_BOXES %d\n" % Y.MAX_BOXES in hdr
