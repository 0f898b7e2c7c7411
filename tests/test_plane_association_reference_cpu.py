"""The yardstick of the plane association (tests/plane_association_reference.py) held to what every scene of tests/plane_association_scenes.py claims -- the
branch the scene was built for is the branch the reference's loops take --, its vectorised form held equal to the literal loops bit for bit, and the three
literals (mfDisTh, mfAngleTh, the 100 of PointDistanceFromPlane) held to the reference text through tests/golden/plane_association_constants.json."""
import os
import re
import sys

import numpy as np
import pytest

import plane_association_reference as Y
import plane_association_scenes as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from reference_literals import literals  # noqa: E402


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", sorted(SC.SCENES))
def test_scene_takes_the_branch_it_claims(name):
    sc, r = SC.get(name), SC.reference(name)
    e = sc["expect"]
    assert r["match"].tolist() == list(e["match"])
    for (i, j), v in e.get("dis", {}).items():
        assert bits(r["dis"][i, j]) == bits(v), (i, j, r["dis"][i, j], v)
    for (i, j), v in e.get("gated", {}).items():
        assert r["gated"][i, j] == v, (i, j)
    # what holds on every scene: 100 where gated out; match_dis is the match's distance or the threshold
    assert np.all(bits(r["dis"][r["gated"] == 0]) == bits(Y.NO_DISTANCE))
    for i, m in enumerate(r["match"]):
        assert bits(r["match_dis"][i]) == bits(r["dis"][i, m] if m >= 0 else sc["dis_th"])
        assert m < 0 or r["gated"][i, m]


@pytest.mark.parametrize("name", sorted(SC.SCENES))
def test_vectorised_form_equals_the_literal_loops(name):
    a, b = SC.reference(name), SC.reference(name, vectorised=True)
    for k in a:
        assert np.array_equal(bits(a[k]) if a[k].dtype == np.float32 else a[k], bits(b[k]) if b[k].dtype == np.float32 else b[k]), k
    sc = SC.get(name)
    for pid, w, xyz, T in sc["planes"]:
        assert np.array_equal(bits(Y.transform_cloud(xyz[:40], T)), bits(Y.transform_cloud_vectorised(xyz[:40], T)))


def test_the_scenes_cover_what_they_should():
    names = set(SC.SCENES)
    assert {"tie_ab", "tie_ba", "threshold_distance", "threshold_angle", "from_behind", "later_closer", "gated_out_closer", "empty_cloud", "far_cloud", "nan_point",
            "nan_row", "nan_cloud", "permuted_subset", "same_id_twice", "scaled_sim3", "three_sets", "sizes"} <= names
    for n in (1, 63, 64, 65, 255, 256, 257, Y.CHUNK - 1, Y.CHUNK + 1):
        assert n in SC.SIZES
    for k in range(3):
        sc = SC.get("room_%d" % k)
        assert 6 <= len(sc["planes"]) <= 10 and 3 <= len(sc["coef"]) <= 6 and all(p[3] is not None for p in sc["planes"])
    assert SC.get("three_sets")["set_start"].tolist() == [0, 2, 2, 5]
    S = SC.get("scaled_sim3")["M"][0].astype(np.float64)
    assert abs(np.cbrt(np.linalg.det(S[:3, :3])) - 1.7) < 1e-5


def test_transform_is_the_inverse_pose():
    rs = np.random.RandomState(0)
    T = SC.pose(rs)
    Xw = rs.uniform(-3, 3, (50, 3))
    Xc = (Xw @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
    back = Y.transform_cloud(Xc, T.astype(np.float32))
    assert np.abs(back - Xw).max() < 5e-6      # float32 inputs of magnitude <= 8: a few ulp of 2^-21
    nf = Y.transform_cloud(np.array([[np.nan, 1, 2], [np.inf, 0, 0]], np.float32), T.astype(np.float32))
    assert np.isnan(nf[0]).all() and not np.isfinite(nf[1]).any()


def test_model_compacts_past_half():
    m = Y.Model()
    for k in range(4):
        m.add(k, SC.UP, np.zeros((10, 3)))
    m.erase(0)
    m.erase(1)
    assert (m.used, m.dead, m.compactions) == (40, 20, 0)
    m.update_boundary(2, np.zeros((3, 3)))      # dead 30 of 43
    assert (m.used, m.dead, m.compactions) == (13, 0, 1)
    assert [(e[0], e[1], e[2]) for e in m.live()] == [(2, 0, 3), (3, 3, 10)]      # add order kept: the updated plane stays in front


def test_literals_match_the_reference_text():
    lit = literals("plane_association")      # (held to the reference text by tests/test_reference_literals.py)
    assert set(lit) == {"DIS_TH", "ANGLE_TH", "NO_DISTANCE"}
    assert np.float32(float(lit["DIS_TH"])) == Y.DIS_TH and np.float32(float(lit["ANGLE_TH"])) == Y.ANGLE_TH and np.float32(float(lit["NO_DISTANCE"])) == Y.NO_DISTANCE
    hdr = open(os.path.join(ROOT, "include", "eao_fusion.h")).read()
    assert re.search(r"#define EAO_PLANE_MAP_DIS_TH %sf\b" % re.escape(lit["DIS_TH"]), hdr)
    assert re.search(r"#define EAO_PLANE_MAP_ANGLE_TH %sf\b" % re.escape(lit["ANGLE_TH"]), hdr)
    internal = open(os.path.join(ROOT, "eao_fusion_amd", "csrc", "plane_map_internal.h")).read()
    assert re.search(r"kNoDistance = %s\.0f;" % re.escape(lit["NO_DISTANCE"]), internal)
    assert "kChunk = %d;" % Y.CHUNK in internal
    py = open(os.path.join(ROOT, "eao_fusion_amd", "plane_map.py")).read()
    assert "DIS_TH = %s " % lit["DIS_TH"] in py and "ANGLE_TH = %s " % lit["ANGLE_TH"] in py and "NO_DISTANCE = %s.0 " % lit["NO_DISTANCE"] in py
    adapter = open(os.path.join(ROOT, "include", "eaofusion", "MapPlanes.h")).read()
    assert "EAO_PLANE_MAP_DIS_TH" in adapter and "EAO_PLANE_MAP_ANGLE_TH" in adapter
