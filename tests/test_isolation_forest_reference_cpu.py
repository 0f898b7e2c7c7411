"""The isolation forest's yardstick (tests/isolation_forest_reference.py) against what the REFERENCE's own include/isolation_forest.h computed
(tests/golden/isolation_forest/*.npz, written by tools/gen_golden_isolation_forest.py): both restated builds to the recorded Serialize bytes, the scores, the
branch each scene is named for, the gap around the thresholds, the literals, and generate_canonical's clamp."""
import hashlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import isolation_forest_reference as Y
import isolation_forest_scenes as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from reference_literals import literals  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "isolation_forest")
SCENES = SC.scenes()
SORTED_FORM_MAX = 300      # the literal, sorting build restated in Python is held on every scene up to this size


def fixture(name):
    z = np.load(os.path.join(GOLD, name + ".npz"))
    return {k: z[k] for k in z.files}


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest().encode()


def ulps(a, b):
    """distance in units in the last place between two arrays of finite doubles of one sign"""
    return np.abs(a.view(np.int64) - b.view(np.int64))


def same_scores(got, want, slack):
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and (ulps(got[~nan], want[~nan]) <= slack).all()


def test_fixtures_are_the_scenes():
    assert sorted(SCENES) == sorted(f[:-4] for f in os.listdir(GOLD) if f.endswith(".npz"))
    for name, sc in SCENES.items():
        z = fixture(name)
        assert np.array_equal(z["points"].view(np.uint32), sc["points"].view(np.uint32)), name
        assert (int(z["tree_count"]), int(z["seed"]), int(z["sample_size"]), int(z["class_id"])) == (sc["tree_count"], sc["seed"], sc["sample_size"], sc["class_id"])
        assert ("stream" in z) == (not sc.get("by_hash")), name
        if "stream" in z:
            assert len(z["stream"]) == int(z["stream_len"]) and sha(z["stream"].tobytes()) == z["stream_sha256"].tobytes()
        assert os.path.getsize(os.path.join(GOLD, name + ".npz")) < 144 * 1024
        if sc["entry"] == "object":
            assert (sc["tree_count"], sc["seed"], sc["sample_size"]) == (Y.TREE_COUNT, Y.SEED, len(sc["points"]) // Y.SAMPLE_DIVISOR)


@pytest.mark.parametrize("name", sorted(SCENES))
def test_sort_free_build_and_scores(name):
    sc, z = SCENES[name], fixture(name)
    stream, scores, _ = Y.forest(sc["points"], sc["tree_count"], sc["seed"], sc["sample_size"])
    assert len(stream) == int(z["stream_len"]) and sha(stream) == z["stream_sha256"].tobytes()
    if "stream" in z:
        assert stream == z["stream"].tobytes()
    assert same_scores(scores, z["scores"], 1)      # (bit-equal with the libm the fixtures were recorded with; the slack is for another libm)


@pytest.mark.parametrize("name", sorted(n for n, s in SCENES.items() if len(s["points"]) <= SORTED_FORM_MAX))
def test_literal_build_with_the_sort(name):
    sc, z = SCENES[name], fixture(name)
    stream, _, _ = Y.forest(sc["points"], sc["tree_count"], sc["seed"], sc["sample_size"], sorted_form=True)
    assert stream == z["stream"].tobytes()


def leaves(name):
    """(dim, split, size, depth) of every leaf of the recorded stream, and the tree's depth limit"""
    sc = SCENES[name]
    stream, _, _ = Y.forest(sc["points"], sc["tree_count"], sc["seed"], sc["sample_size"]) if sc.get("by_hash") else (fixture(name)["stream"].tobytes(), 0, 0)
    sample_size, trees = Y.parse(stream)
    out = []
    for dim, split, size, right in trees:
        depth = np.zeros(len(dim), np.int64)
        for i in range(len(dim)):
            if size[i] == 0:
                depth[i + 1] = depth[right[i]] = depth[i] + 1
        out += [(int(dim[i]), float(split[i]), int(size[i]), int(depth[i])) for i in range(len(dim)) if size[i]]
    return out, Y.max_depth(sample_size)


def kinds(name):
    lv, md = leaves(name)
    return dict(depth_limit=sum(1 for d, s, z, dep in lv if dep >= md and z > 1),
                singleton=sum(1 for d, s, z, dep in lv if z == 1),
                kept_split=sum(1 for d, s, z, dep in lv if s != 0.0 and z > 1),          # middle == first: m_dimId and m_dimSplitValue stay set
                flat=sum(1 for d, s, z, dep in lv if dep < md and z > 1 and s == 0.0),   # min == max (after a dimension draw; the draw may have been 0)
                leaves=len(lv), trees_of_one_leaf=0)


@pytest.mark.parametrize("n", (30, 31, 64, 65, 128, 129, 300))
def test_clouds_reach_both_ordinary_leaves(n):
    k = kinds("gauss_%d" % n)
    assert k["depth_limit"] > 0 and k["singleton"] > 0 and k["kept_split"] == 0


def test_adjacent_floats_reach_the_leaf_that_keeps_its_split():
    assert kinds("adjacent")["kept_split"] > 0 and kinds("four_ulps")["kept_split"] > 0


def test_constant_coordinate_reaches_the_equal_extremes_leaf():
    lv, md = leaves("flat_y")
    assert any(dep < md and z > 1 and s == 0.0 and d == 1 for d, s, z, dep in lv)


def test_identical_points_give_single_leaf_trees():
    z = fixture("all_same")
    sample_size, trees = Y.parse(z["stream"].tobytes())
    assert all(len(t[0]) == 1 and t[2][0] == sample_size for t in trees)


def test_ties_straddle_splits():
    for name in ("lattice", "dup_pairs"):
        pts = SCENES[name]["points"]
        assert len(np.unique(pts, axis=0)) < len(pts) or len(np.unique(pts[:, 0])) < len(pts)
        assert kinds(name)["singleton"] > 0


def test_sample_of_one_scores_nan():
    z = fixture("sample_1")
    assert np.isnan(z["scores"]).all()
    _, scores, _ = Y.forest(SCENES["sample_1"]["points"], 5, 1, 1)
    assert np.isnan(scores).all()


def test_no_score_near_a_threshold():
    """so that no flag hinges on the last bit of pow"""
    for name in SCENES:
        s = fixture(name)["scores"]
        s = s[~np.isnan(s)]
        for th in (0.6, 0.65):
            assert len(s) == 0 or np.abs(s - np.float64(np.float32(th))).min() > 1e-9, name


def test_class_62_threshold_matters_on_its_scene():
    s = fixture("class62_60")["scores"]
    assert Y.outlier_flags(s, 62).sum() < Y.outlier_flags(s, 0).sum()


def test_canonical_float_clamp():
    """draws >= 0xFFFFFF80 convert to 2^32 and the quotient 1.0 is clamped to nextafter(1, 0); the draw below converts to the float below"""
    top = np.nextafter(np.float32(1), np.float32(0))
    for d in (0xFFFFFF80, 0xFFFFFFC0, 0xFFFFFFFF):
        assert Y.canonical_float(d) == top
    assert Y.canonical_float(0xFFFFFF7F) == top      # rounds down to 2^32 - 256: the same float by another road
    assert Y.canonical_float(0xFFFFFE80) == np.float32(1) - np.float32(2.0 ** -23)      # a tie, to even
    assert Y.canonical_float(0) == 0 and Y.canonical_float(1 << 31) == np.float32(0.5)


def test_mt19937_known_value():
    """the 10000th draw of a default-seeded std::mt19937 is 4123659995 ([rand.predef])"""
    g = Y.Mt19937(5489)
    for _ in range(9999):
        g()
    assert g() == 4123659995


def test_lds_edge_scenes_sit_on_the_header_budget():
    hdr = open(os.path.join(ROOT, "eao_fusion_amd", "csrc", "iforest_internal.h")).read()
    budget = int(re.search(r"kLdsBudget = (\d+);", hdr).group(1))

    def need(n, s):
        return ((max(n, 2 * s) * 2 + 15) & ~15) + 12 * s

    assert need(SC.LDS_EDGE_N, SC.LDS_EDGE_N) <= budget < need(SC.GLOBAL_PATH_N, SC.GLOBAL_PATH_N)
    assert need(2000, 1000) <= budget


def test_constants():
    lit = literals("isolation_forest")      # (held to the reference text by tests/test_reference_literals.py)
    assert (int(lit["TREE_COUNT"]), int(lit["SEED"]), int(lit["MIN_POINTS"]), int(lit["SAMPLE_DIVISOR"])) == (Y.TREE_COUNT, Y.SEED, Y.MIN_POINTS, Y.SAMPLE_DIVISOR)
    assert (int(lit["EXEMPT_CLASS_A"]), int(lit["EXEMPT_CLASS_B"]), int(lit["EXEMPT_CLASS_C"])) == Y.EXEMPT_CLASSES
    assert (float(lit["THRESHOLD"]), int(lit["THRESHOLD_CLASS"]), float(lit["THRESHOLD_OF_CLASS"])) == (Y.THRESHOLD, Y.THRESHOLD_CLASS, Y.THRESHOLD_OF_CLASS)
    assert (SC.TREE_COUNT, SC.SEED) == (Y.TREE_COUNT, Y.SEED)
    hdr = open(os.path.join(ROOT, "eao_fusion_amd", "csrc", "iforest_internal.h")).read()
    for want in ("kTreeCount = %s;" % lit["TREE_COUNT"], "kSeed = %s;" % lit["SEED"], "kSampleDivisor = %s;" % lit["SAMPLE_DIVISOR"], "kMinPoints = %s;" % lit["MIN_POINTS"],
                 "kExemptClasses[3] = {%s, %s, %s};" % (lit["EXEMPT_CLASS_A"], lit["EXEMPT_CLASS_B"], lit["EXEMPT_CLASS_C"]), "kThreshold = %sf;" % lit["THRESHOLD"],
                 "kThresholdClass = %s;" % lit["THRESHOLD_CLASS"], "kThresholdOfClass = %sf;" % lit["THRESHOLD_OF_CLASS"]):
        assert want in hdr, want
    ref = os.environ.get("EAO_REFERENCE_DIR")
    if ref and os.path.isdir(ref):      # with the reference tree at hand: the golden files against the header itself
        subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_golden_isolation_forest.py"), ref, "--check"])
