"""The yardstick of the object layer's data association (tests/object_association_reference.py: a literal transcription of Object_2D::NoParaDataAssociation and
Object_Map::ComputeProjectRectFrame, and a sort-free / vectorised form of each) on its own: every scene reaches the branch it is named for, the two forms
agree on every scene and on a few hundred random small cases, the float counters stay exact under the overflow bound, the literals are the reference text's, and
the golden files are what the yardstick computes."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import object_association_reference as Y
import object_association_scenes as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from reference_literals import literals  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "object_association")
NP_SCENES, RECT_SCENES = SC.np_scenes(), SC.rect_scenes()
CAM = ("fx", "fy", "cx", "cy", "cols", "rows")
_cache = {}


def literal(name):
    if name not in _cache:
        s = NP_SCENES[name]
        _cache[name] = Y.np_literal(s["det"], s["map"], s["S"])
    return _cache[name]


def same_result(a, b):
    return ((a["m"], a["n"], a["step"], a["verdict"]) == (b["m"], b["n"], b["step"], b["verdict"]) and np.array_equal(a["counts"], b["counts"])
            and a["w"].tobytes() == b["w"].tobytes() and a["r"].tobytes() == b["r"].tobytes())


@pytest.mark.parametrize("name", sorted(NP_SCENES))
def test_scene_reaches_its_branch_and_both_forms_agree(name):
    s, g = NP_SCENES[name], literal(name)
    b = s["branch"]
    assert same_result(g, Y.np_sort_free(s["det"], s["map"], s["S"]))
    m, k = len(s["det"]), len(s["map"])
    for key in ("verdict", "step", "n"):
        if key in b:
            assert g[key] == b[key], key
    if b.get("early"):
        assert m >= SC.MIN_POINTS and k < SC.MIN_POINTS and g["counts"].sum() == 0
    if "sampled" in b:
        assert (k > SC.SAMPLE_RATIO * m) == b["sampled"]
        assert g["step"] == (s["S"] // (SC.SAMPLE_RATIO * m) if b["sampled"] else 1)
    if b.get("ties"):
        assert all(g["counts"][3 * a + 2] > 0 for a in range(3))
    if "fails" in b:
        inside = [bool(g["r"][0] < g["w"][a] < g["r"][1]) for a in range(3)]
        assert inside == [a not in b["fails"] for a in range(3)]
    if g["verdict"] in (1, 2) and not b.get("early"):      # every pair lands in exactly one counter
        assert all(int(g["counts"][3 * a:3 * a + 3].sum()) == g["m"] * g["n"] for a in range(3))
        assert g["m"] * g["n"] < 2 ** 24


def test_scene_sizes_sit_on_the_kernels_shapes():
    src = open(os.path.join(ROOT, "eao_fusion_amd", "csrc", "object_assoc.hip")).read()
    shapes = tuple(int(re.search(r"constexpr int %s = (\d+);" % k, src).group(1)) for k in ("kBlock", "kOwned", "kTile"))
    assert shapes == (SC.BLOCK, SC.OWNED, SC.TILE)
    for m in (63, 64, 65, SC.BLOCK - 1, SC.BLOCK, SC.BLOCK + 1, SC.BLOCK * SC.OWNED - 1, SC.BLOCK * SC.OWNED, SC.BLOCK * SC.OWNED + 1):
        assert len(NP_SCENES["m%d" % m]["det"]) == m
    for k in (SC.TILE - 1, SC.TILE, SC.TILE + 1, 2 * SC.TILE + 1):
        assert len(NP_SCENES["ngood%d" % k]["map"]) == k


def test_overflow_bound_scenes_straddle_int32():
    under, over = literal("bound_under"), literal("bound_over")
    assert under["m"] * under["n"] * (under["m"] + under["n"] + 1) <= Y.INT32_MAX < over["m"] * over["n"] * (over["m"] + over["n"] + 1)
    assert over["m"] == under["m"] + 1 and under["verdict"] in (1, 2) and over["verdict"] == Y.UNDEFINED and over["counts"].sum() == 0


def test_counters_stay_below_2_pow_24_under_the_bound():
    """with n < 6 m after the sampling and m n (m + n + 1) <= INT32_MAX, m n < 2^24: a float counter incremented by one is exact"""
    worst = 0
    for n in list(range(20, 200)) + [2 ** k for k in range(8, 13)] + [3000, 5000, 6000]:
        m = max(SC.largest_m_under_the_bound(n), 1)
        if 6 * m <= n:
            continue      # the sampling keeps n below 6 m: such a pair does not exist
        worst = max(worst, m * n)
    assert 0 < worst < 2 ** 24
    rs = np.random.RandomState(3)
    for _ in range(300):      # n = ceil(nGood / step) < 6 m whenever the sampling runs
        m, k = int(rs.randint(20, 400)), int(rs.randint(20, 20000))
        S = k + int(rs.randint(0, k))
        v, n, step = Y.plan(m, k, S)
        assert n < 6 * m or k <= 3 * m


def test_random_small_cases_both_forms():
    rs = np.random.RandomState(11)
    for i in range(300):
        m, k = int(rs.randint(15, 45)), int(rs.randint(15, 220))
        S = k + int(rs.randint(0, 3 * k))
        q = float(rs.choice([0.0, 0.05, 0.25]))
        det, mp = rs.normal(0, 0.3, (m, 3)), rs.normal(0, 0.3, (k, 3))
        if q:
            det, mp = np.round(det / q) * q, np.round(mp / q) * q
        if i % 7 == 0:
            det[: m // 2] = mp[: m // 2] if k >= m // 2 else det[: m // 2]      # detection points that are map points
        assert same_result(Y.np_literal(det, mp, S), Y.np_sort_free(det, mp, S)), i


@pytest.mark.parametrize("name", sorted(RECT_SCENES))
def test_rect_scene_reaches_its_branch_and_both_forms_agree(name):
    s = RECT_SCENES[name]
    kw = {k: s[k] for k in CAM}
    st, rect, uv = Y.rect_literal(s["points"], s["Tcw"], **kw)
    st2, rect2, uv2 = Y.rect_vectorised(s["points"], s["Tcw"], **kw)
    assert st == st2 == s["status"] and uv.tobytes() == uv2.tobytes()
    assert (rect is None and rect2 is None) or np.array_equal(rect, rect2)
    if "clamps" in s:
        hit = set()
        if uv[:, 0].min() < 0:
            hit.add("x_min")
        if uv[:, 1].min() < 0:
            hit.add("y_min")
        if uv[:, 0].max() > s["cols"]:
            hit.add("x_max")
        if uv[:, 1].max() > s["rows"]:
            hit.add("y_max")
        assert hit == set(s["clamps"])
    if name == "z0_infinite":
        assert np.isinf(uv).any() and not np.isnan(uv).any()
    if name == "z0_nan":
        assert np.isnan(uv).any()
    if name == "point_behind_the_camera":
        assert (s["points"][:, 2] < 0).any()
    if name in ("box_right_of_int", "width_minus_infinity"):
        assert not np.isnan(uv).any()


def test_constants():
    lit = literals("object_association")      # (held to the reference text by tests/test_reference_literals.py)
    assert (int(lit["MIN_DET_POINTS"]), int(lit["MIN_MAP_POINTS"]), int(lit["SAMPLE_RATIO"]), int(lit["SAMPLE_RATIO_N"])) == (Y.MIN_DET_POINTS, Y.MIN_MAP_POINTS,
                                                                                                                              Y.SAMPLE_RATIO, Y.SAMPLE_RATIO)
    assert (float(lit["HALF"]), float(lit["CRITICAL"]), int(lit["VARIANCE_DIVISOR"])) == (Y.HALF, Y.CRITICAL, Y.VARIANCE_DIVISOR)
    assert (lit["HALF_R2"], lit["CRITICAL_R2"], lit["VARIANCE_DIVISOR_R2"]) == (lit["HALF"], lit["CRITICAL"], lit["VARIANCE_DIVISOR"])
    assert (SC.MIN_POINTS, SC.MIN_POINTS, SC.SAMPLE_RATIO) == (Y.MIN_DET_POINTS, Y.MIN_MAP_POINTS, Y.SAMPLE_RATIO)
    internal = open(os.path.join(ROOT, "eao_fusion_amd", "csrc", "object_assoc_internal.h")).read()
    for want in ("kMinDetPoints = %s;" % lit["MIN_DET_POINTS"], "kMinMapPoints = %s;" % lit["MIN_MAP_POINTS"], "kSampleRatio = %s;" % lit["SAMPLE_RATIO"],
                 "kCritical = %s;" % lit["CRITICAL"], "kVarianceDivisor = %s;" % lit["VARIANCE_DIVISOR"], "kHalf = %s;" % lit["HALF"]):
        assert internal.count(want) == 1, want
    header = open(os.path.join(ROOT, "include", "eao_fusion.h")).read()
    for name, key in (("MIN_DET_POINTS", "MIN_DET_POINTS"), ("MIN_MAP_POINTS", "MIN_MAP_POINTS"), ("SAMPLE_RATIO", "SAMPLE_RATIO"), ("CRITICAL", "CRITICAL"),
                      ("VARIANCE_DIVISOR", "VARIANCE_DIVISOR"), ("HALF", "HALF")):
        assert re.search(r"#define EAO_OBJECT_NP_%s %s\s" % (name, re.escape(lit[key])), header), name


def test_golden_files_are_the_yardsticks():
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_golden_object_association.py"), "--check"])
    for stem in ("np", "rect"):
        assert os.path.getsize(os.path.join(GOLD, stem + ".npz")) < 144 * 1024
    z = np.load(os.path.join(GOLD, "np.npz"))
    assert sorted({k.rsplit(".", 1)[0] for k in z.files}) == sorted(NP_SCENES)
    z = np.load(os.path.join(GOLD, "rect.npz"))
    assert sorted({k.rsplit(".", 1)[0] for k in z.files}) == sorted(RECT_SCENES)
