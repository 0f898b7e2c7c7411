"""The yardstick of a map object's cuboid (tests/object_cuboid_reference.py) against itself: the literal form (sorts, push_backs, early returns) equals the
device's form (extrema, whole-list passes) on every scene; every scene reaches the branch it claims; the fields in which a tie between -0.0f and +0.0f shows are
named, and differ in the sign of zeros only; the recorded results are the yardstick's; the literals are the reference text's."""
import os
import re
import sys

import numpy as np
import pytest

import object_cuboid_reference as Y
import object_cuboid_scenes as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden_object_cuboid as GG  # noqa: E402
import reference_literals as RL  # noqa: E402

SCENES = SC.scenes()
NAMES = sorted(SCENES)
OVERLAPS = SC.overlap_scenes()


@pytest.fixture(scope="module")
def results():
    """both forms of every scene, computed once"""
    out = {}
    for name in NAMES:
        info = []
        out[name] = dict(literal=Y.literal(SCENES[name], info=info), device=Y.device(SCENES[name]), info=info, zero_sign=Y.zero_sign_fields(SCENES[name]))
    return out


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "object_cuboid", "results.npz"))


@pytest.mark.parametrize("name", NAMES)
def test_both_forms_agree_and_the_scene_reaches_its_branch(results, name):
    o, r = SCENES[name], results[name]
    lit, dev, c = r["literal"], r["device"], o["claims"]
    assert Y.same_records(lit, dev, drop=r["zero_sign"]), Y.differing_fields(lit, dev)
    assert (len(o["points"]), len(o["centroids"])) == (c["n"], c["m"])
    assert (int(dev["status"]), int(dev["bounds_written"])) == (c["status"], c["bounds_written"])
    if c["status"] == Y.EMPTY:      # nothing past mStandar_*: the sums are zero, the centre and deviations 0 / 0
        assert np.isnan(dev["center"]).all() and np.isnan(dev["standar"]).all() and not dev["sum_pos"].any()
        rest = [k for k in Y.RECORD_DTYPE.names if k not in ("status", "sum_pos", "center", "standar")]
        assert all(not np.asarray(dev[k]).any() for k in rest)
        return
    assert bool(np.isnan(dev["center_standar"]).all()) == (c["m"] == 0) and bool(np.isnan(dev["center_standar_dis"])) == (c["m"] == 0)
    if not c["bounds_written"]:
        assert not dev["bounds"].any()      # m >= 5: upstream leaves them alone
    if "branch" in c:
        assert r["info"][0][0] == c["branch"]
    if c.get("w_negative"):
        assert r["info"][0][0] >= 0 and r["info"][0][1]      # the expression CAN produce w < 0 before normalizeRotation: roll past pi
        assert dev["pose_q"][3] >= 0
    if c.get("zero_scale"):
        assert not dev["standar"].any() and (dev["lenth"], dev["width"], dev["height"]) == (0, 0, 0)
    if c.get("overflow"):
        assert np.isinf(dev["standar"]).all() and np.isinf(dev["rmax"])
    if c.get("far"):      # the first pose sits at prev_cuboid_center, the final one at the points
        assert np.abs(dev["cuboid_center"] - o["points"].mean(axis=0)).max() < 1.0 < np.abs(o["prev_cuboid_center"] - dev["cuboid_center"]).min()
    if c.get("zero_sign"):
        assert r["zero_sign"] != []


def test_the_branches_are_all_reached(results):
    reached = {r["info"][0] for r in results.values() if r["info"]}
    assert {b for b, _ in reached} == {-1, 0, 1, 2} and any(neg for _, neg in reached)


def test_the_zero_sign_rule_touches_the_bounds_alone(results):
    """-0.0f beside +0.0f at an extremum: on the two scenes that hold such a tie the choice shows in the world-frame bounds and in no other field (the world-frame
    scale and centre that inherit it are overwritten from the object frame before the record is stored); no other scene holds a tie that shows at all"""
    named = {name: r["zero_sign"] for name, r in results.items() if r["zero_sign"]}
    assert sorted(named) == ["zero_signs_at_the_maximum", "zero_signs_at_the_minimum"] and all(v == ["bounds"] for v in named.values())


def test_variants(results, gold):
    """which scenes' records change under the alternative readings: recorded per scene, and both kinds exist"""
    flags = {name: Y.variant(SCENES[name]) for name in NAMES}
    assert all(flags[name] == GG.unpack(gold, name)[1] for name in NAMES)
    assert any(flags.values()) and not all(flags.values())


def test_golden_files_are_the_yardsticks(gold):
    assert GG.same_as_recorded(gold, GG.build()) == []
    assert os.path.getsize(GG.PATH) < 1 << 20


@pytest.mark.parametrize("name", sorted(OVERLAPS))
def test_overlap_forms_agree(gold, name):
    rows, eligible = OVERLAPS[name]
    v, e = Y.overlaps_literal(rows, eligible)
    v2, e2 = Y.overlaps_vectorised(rows, eligible)
    gv, ge = GG.unpack_overlaps(gold, name)
    assert np.array_equal(v, v2) and np.array_equal(e.view(np.uint32), e2.view(np.uint32))
    assert np.array_equal(v, gv) and np.array_equal(e.view(np.uint32), ge.view(np.uint32))
    assert not np.diag(v).any() and np.array_equal(v, v.T)
    assert not v[eligible == 0].any() and not v[:, eligible == 0].any()


def test_overlap_scenes_reach_what_they_claim():
    v, _ = Y.overlaps_literal(*OVERLAPS["touching"])
    assert v[0, 1] == 0 and v[0, 2] == 1 and v[1, 2] == 1      # dis == sum_half: `<` is strict
    assert Y.overlap_pair(OVERLAPS["touching"][0][0], OVERLAPS["touching"][0][1])[1][0] == 0
    assert Y.overlaps_literal(*OVERLAPS["inside"])[0].tolist() == [[0, 1], [1, 0]]
    rows, eligible = OVERLAPS["ineligible_row"]
    assert Y.overlaps_literal(rows, np.ones(3, np.uint8))[0].sum() == 6 and Y.overlaps_literal(rows, eligible)[0].sum() == 2
    assert sorted(len(OVERLAPS[k][0]) for k in ("m1", "m2", "m64", "m65")) == [1, 2, 64, 65]
    assert Y.overlaps_literal(*OVERLAPS["m65"])[0].any()


def test_literals():
    lit = RL.literals("object_cuboid")
    assert int(lit["FEW_FRAMES"]) == Y.FEW_FRAMES
    assert (int(lit["CORNER_FAR_A"]), int(lit["CORNER_FAR_B"])) == Y.CORNER_FAR and int(lit["CENTER_DIVISOR"]) == 2 == int(lit["OVERLAP_HALF"])
    masks = {"X": 0, "Y": 0, "Z": 0}
    for key, v in lit.items():
        if key.startswith("CORNER_M"):
            for axis, which in zip("XYZ", key[len("CORNER_"):].split("_")):
                masks[axis] |= (which == "MAX") << (int(v) - 1)
    assert (masks["X"], masks["Y"], masks["Z"]) == (Y.CORNER_MAX_X, Y.CORNER_MAX_Y, Y.CORNER_MAX_Z)
    assert (lit["WITHOUT_YAW_X_FROM_CENTER3D"], lit["WITHOUT_YAW_Y_FROM_CUBOID_CENTER"], lit["WITHOUT_YAW_Z_FROM_CENTER3D"]) == ("0", "1", "2")
    h = open(os.path.join(ROOT, "eao_fusion_amd", "csrc", "object_cuboid_internal.h")).read()
    assert "constexpr int32_t kFewFrames = %s;" % lit["FEW_FRAMES"] in h
    assert "constexpr int32_t kCornerFarA = %s, kCornerFarB = %s;" % (lit["CORNER_FAR_A"], lit["CORNER_FAR_B"]) in h
    assert "kCornerMaxX = 0x%02X, kCornerMaxY = 0x%02X, kCornerMaxZ = 0x%02X;" % (masks["X"], masks["Y"], masks["Z"]) in h
    assert re.search(r"W\[3\] = r\.center\[0\];.*\n\s*W\[7\] = \(float\)r\.cuboid_center\[1\];\n\s*W\[11\] = r\.center\[2\];", h)
    a = open(os.path.join(ROOT, "include", "eaofusion", "ObjectMap.h")).read()
    assert "mObjectFrame.size() < %s" % lit["FEW_FRAMES"] not in a      # the adapter takes the path from the record, not from a literal of its own
