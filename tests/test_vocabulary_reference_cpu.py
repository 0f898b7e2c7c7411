"""The vocabulary yardstick (tests/vocabulary_reference.py) held on its own, without a device: a hand-computed two-level example, the invariants of a transform,
every scene of tests/vocabulary_scenes.py reaching the branch it claims, and the enum orders and FORB::L against the reference text."""
import math
import os
import re

import numpy as np
import pytest

import vocabulary_reference as Y
import vocabulary_scenes as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hand_tree(weighting, norm):
    # ids: 1 = A (children 3 = A1, 4 = A2), 2 = B (a leaf at depth 1).  Words in id order: B = 0, A1 = 1, A2 = 2.
    desc = np.zeros((4, 32), np.uint8)
    desc[1] = 0xFF           # B
    desc[3, 0] = 0x0F        # A2
    return dict(parent=np.array([0, 0, 1, 1], np.int32), descriptor=desc, weight=np.array([9.0, 2.0, 0.5, 0.25]), is_leaf=np.array([0, 1, 1, 1], np.uint8),
                weighting=weighting, norm=norm)


def _hand_features():
    f = np.zeros((4, 32), np.uint8)
    f[1] = 0xFF              # -> B
    f[2, 0] = 0x0F           # -> A, A2 (distance 0 against 4)
    f[3, 0] = 0x03           # -> A, then 2 bits from A1 and 2 bits from A2: the first in id order, A1
    return f


def test_hand_computed_two_level_example():
    t = Y.Tree(_hand_tree(Y.TF_IDF, Y.NORM_L1))
    assert (t.depth, t.n_words, t.max_children) == (2, 3, 2)
    ties = []
    assert [Y.descend(t, f, 0, ties)[0] for f in _hand_features()] == [1, 0, 2, 1] and ties == [2]
    r = Y.transform(t, _hand_features(), 0)
    assert r["word_id"].tolist() == [0, 1, 2]
    assert r["word_value"].tolist() == [2.0 / 3.25, (0.5 + 0.5) / 3.25, 0.25 / 3.25]
    assert r["fv"]["node_id"].tolist() == [2, 3, 4] and r["fv"]["node_start"].tolist() == [0, 1, 3, 4] and r["fv"]["index"].tolist() == [1, 0, 3, 2]
    assert r["feat_node"].tolist() == [3, 2, 4, 3] and r["feat_stopped"].tolist() == [0, 2, 0, 0]      # B is a leaf above level 2: its own id, flagged
    r1 = Y.transform(t, _hand_features(), 1)
    assert r1["fv"]["node_id"].tolist() == [1, 2] and r1["fv"]["index"].tolist() == [0, 2, 3, 1] and r1["feat_stopped"].tolist() == [0, 0, 0, 0]
    r2 = Y.transform(t, _hand_features(), 2)
    assert r2["fv"]["node_id"].tolist() == [0] and r2["fv"]["index"].tolist() == [0, 1, 2, 3]      # nid_level <= 0: the root
    # the other modes on the same descents
    assert Y.transform(t, _hand_features(), 0, Y.TF, Y.NORM_NONE)["word_value"].tolist() == [2.0 / 3.0, 1.0 / 3.0, 0.25 / 3.0]      # divided by v.size()
    assert Y.transform(t, _hand_features(), 0, Y.IDF, Y.NORM_NONE)["word_value"].tolist() == [2.0, 0.5, 0.25]                      # the weight once, untouched
    l2 = math.sqrt(2.0 * 2.0 + 0.5 * 0.5 + 0.25 * 0.25)
    assert Y.transform(t, _hand_features(), 0, Y.BINARY, Y.NORM_L2)["word_value"].tolist() == [2.0 / l2, 0.5 / l2, 0.25 / l2]
    # the score: one common word
    a, b = (np.array([1, 5], np.uint32), np.array([0.75, 0.25])), (np.array([5, 9], np.uint32), np.array([0.5, 0.5]))
    assert Y.score_l1(a, b) == -(abs(0.25 - 0.5) - 0.25 - 0.5) / 2.0 == 0.25
    assert math.copysign(1.0, Y.score_l1(a, (np.array([7], np.uint32), np.array([1.0])))) == -1.0      # no common word: -0.0


@pytest.mark.parametrize("name", sorted(SC.SCENES))
def test_invariants(name):
    sc = SC.scene(name)
    n = len(sc["features"])
    for levelsup in sc["levelsups"]:
        for weighting in SC.WEIGHTINGS:
            r = SC.reference(name, levelsup, weighting, Y.NORM_L1)
            kept = np.flatnonzero((r["feat_stopped"] & 1) == 0) if sc["tree"].n_nodes else np.zeros(0, np.int64)
            assert sorted(r["fv"]["index"].tolist()) == kept.tolist()      # every index once, unless stopped
            assert np.all(np.diff(r["fv"]["node_id"].astype(np.int64)) > 0) and np.all(np.diff(r["word_id"].astype(np.int64)) > 0)
            for j in range(len(r["fv"]["node_id"])):
                seg = r["fv"]["index"][r["fv"]["node_start"][j]:r["fv"]["node_start"][j + 1]]
                assert len(seg) > 0 and np.all(np.diff(seg.astype(np.int64)) > 0) and np.all(r["feat_node"][seg] == r["fv"]["node_id"][j])
            assert set(r["word_id"].tolist()) == set(r["feat_word"][kept].tolist())
            if len(r["word_id"]):
                assert abs(float(np.sum(r["word_value"])) - 1.0) <= n * 2.0 ** -52      # L1-normalised: the values sum to 1 within 1 ulp x n
                v = (r["word_id"], r["word_value"])
                assert abs(Y.score_l1(v, v) - 1.0) <= n * 2.0 ** -52                     # score(v, v) = 1 within rounding


def test_scenes_reach_their_branches():
    # k10_l3: ties among siblings occur by themselves
    sc = SC.scene("k10_l3")
    ties = []
    for f in sc["features"]:
        Y.descend(sc["tree"], f, 0, ties)
    assert len(ties) >= 1 and (sc["tree"].depth, sc["tree"].max_children, sc["tree"].n_nodes) == (3, 10, 1110)
    sibs = np.flatnonzero(sc["desc"]["parent"] == 1)
    assert not np.array_equal(sibs, np.arange(sibs[0], sibs[0] + len(sibs)))      # the children of a node are not contiguous in file order
    # irregular: 1 .. 20 children, leaves at depths 1 .. 5, a leaf shallower than nid_level
    t = SC.scene("irregular")["tree"]
    counts = {len(c) for c in t.children if c}
    leaf_levels = {t.level[i] for i in range(1, t.n_nodes + 1) if not t.children[i]}
    assert min(counts) == 1 and max(counts) >= 17 and leaf_levels == {1, 2, 3, 4, 5} and t.n_nodes <= 1300
    r = SC.reference("irregular", 0, Y.TF_IDF, Y.NORM_L1)
    assert (r["feat_stopped"] & 2).any() and not (r["feat_stopped"] & 2).all()
    assert not (SC.reference("irregular", 7, Y.TF_IDF, Y.NORM_L1)["feat_stopped"] & 2).any() and set(SC.reference("irregular", 7, Y.TF_IDF, Y.NORM_L1)["fv"]["node_id"]) == {0}
    assert {0, 4, t.depth, t.depth + 2} <= set(SC.scene("irregular")["levelsups"])
    # one_child
    t = SC.scene("one_child")["tree"]
    single = [i for i in range(1, t.n_nodes + 1) if len(t.children[i]) == 1]
    assert len(single) >= 2 and set(SC.reference("one_child", 0, 0, 1)["feat_word"]) >= {t.word_id[t.children[s][0]] for s in single if not t.children[t.children[s][0]]}
    # k17 / k20: more children than a 16-lane group, and winners beyond the 16th child
    for name, k in (("k17", 17), ("k20", 20)):
        sc = SC.scene(name)
        t = sc["tree"]
        assert t.max_children == k
        first = [t.children[0].index(Y.descend(t, f, 1)[2]) for f in sc["features"]]      # levelsup 1 of depth 2: nid is the child of the root
        assert max(first) >= 16 and min(first) < 16
    # duplicated siblings: the minimum is shared at every level, and the winner is the earlier twin
    sc = SC.scene("duplicated_siblings")
    t = sc["tree"]
    for f in sc["features"][:20]:
        ties = []
        wid, _, _, _ = Y.descend(t, f, 0, ties)
        assert ties == [1, 2, 3]
        leaf = [i for i in range(1, t.n_nodes + 1) if t.word_id[i] == wid][0]
        sib = t.children[t.parent[leaf]]
        assert sib.index(leaf) % 2 == 0 and np.array_equal(t.descriptor[leaf - 1], t.descriptor[sib[sib.index(leaf) + 1] - 1])
    # stopped words: zero, minus zero and negative weights are all met, and something is kept
    sc = SC.scene("stopped_words")
    r = SC.reference("stopped_words", 0, 0, 1)
    met = [sc["tree"].weight[[i for i in range(1, sc["tree"].n_nodes + 1) if sc["tree"].word_id[i] == w][0]] for w in set(r["feat_word"][(r["feat_stopped"] & 1) == 1])]
    assert any(w < 0 for w in met) and any(w == 0 and math.copysign(1, w) > 0 for w in met) and any(w == 0 and math.copysign(1, w) < 0 for w in met)
    assert 0 < len(r["fv"]["index"]) < len(sc["features"])
    # all stopped: empty vectors
    r = SC.reference("all_stopped", 0, 0, 1)
    assert len(r["word_id"]) == 0 and len(r["fv"]["node_id"]) == 0 and r["fv"]["node_start"].tolist() == [0] and (r["feat_stopped"] & 1).all()
    # a word hit >= 6 times whose sequential sum is not c * w
    sc = SC.scene("repeated_word")
    r = SC.reference("repeated_word", 0, Y.TF_IDF, Y.NORM_NONE)
    words, counts = np.unique(r["feat_word"][(r["feat_stopped"] & 1) == 0], return_counts=True)
    assert counts.max() >= 9 and (counts >= 6).sum() >= 3
    differs = 0
    for w, c in zip(words, counts):
        weight = sc["tree"].weight[[i for i in range(1, sc["tree"].n_nodes + 1) if sc["tree"].word_id[i] == w][0]]
        seq = weight
        for _ in range(c - 1):
            seq += weight
        assert r["word_value"][list(r["word_id"]).index(w)] == seq / float(len(r["word_id"]))      # c - 1 sequential additions, then the division by v.size()
        differs += int(c >= 6 and seq != c * weight)
    assert differs >= 1
    s = SC.REPEATED_WEIGHT
    assert ((((s + s) + s) + s) + s) + s != 6 * s
    # the empty vocabulary
    r = SC.reference("empty_vocabulary", 4, 0, 1)
    assert SC.scene("empty_vocabulary")["tree"].n_nodes == 0 and len(r["word_id"]) == 0 and r["fv"]["node_start"].tolist() == [0] and not r["feat_stopped"].any()
    assert set(SC.FEATURE_COUNTS) == {0, 1, 3, 4, 5, 63, 64, 65, 1000} and len(SC.scene("k10_l3")["features"]) == 1000


def test_score_sets_reach_their_cases():
    sets = SC.score_sets()
    assert [len(sets[k][1]) for k in ("n_db_0", "n_db_1", "n_db_65")] == [0, 1, 65]
    q = sets["identical"][0]
    assert abs(Y.score_l1(q, sets["identical"][1][0]) - 1.0) <= 300 * 2.0 ** -52
    for name in ("disjoint", "empty_vector"):
        s = Y.score_l1(sets[name][0], sets[name][1][0])
        assert s == 0.0 and math.copysign(1.0, s) == -1.0
    assert len(np.intersect1d(sets["one_common_word"][0][0], sets["one_common_word"][1][0][0])) == 1
    common = [len(np.intersect1d(q[0], v[0])) for v in sets["n_db_65"][1]]
    assert max(common) > 64 and min(common) == 0      # more common words than one wavefront has lanes


def test_orbvoc_shape():
    sc = SC.orbvoc(n=2)
    d = sc["desc"]
    assert len(d["parent"]) == 1111110 and int(d["is_leaf"].sum()) == 10 ** 6 and d["descriptor"].nbytes == 1111110 * 32
    assert np.array_equal(np.bincount(d["parent"], minlength=111111)[:111111], np.full(111111, 10)) and np.all(d["parent"] < np.arange(1, 1111111))


def test_enums_and_descriptor_length_equal_the_reference_text():
    # EAO_REFERENCE_DIR: the project's convention (tests/test_triangulation_reference_cpu.py) -- whoever has a checkout of the reference tree sets it
    ref = os.environ.get("EAO_REFERENCE_DIR")
    if not ref or not os.path.exists(os.path.join(ref, "Thirdparty", "DBoW2", "DBoW2", "BowVector.h")):
        pytest.skip("EAO_REFERENCE_DIR does not name a reference tree")
    dbow = os.path.join(ref, "Thirdparty", "DBoW2", "DBoW2")
    bow = open(os.path.join(dbow, "BowVector.h")).read()

    def enum(name):
        body = re.search(r"enum %s\s*\{(.*?)\}" % name, bow, re.S).group(1)
        return [w for w in re.findall(r"\w+", re.sub(r"//.*", "", body))]

    assert enum("WeightingType") == ["TF_IDF", "TF", "IDF", "BINARY"] and (Y.TF_IDF, Y.TF, Y.IDF, Y.BINARY) == (0, 1, 2, 3)
    assert enum("LNorm") == ["L1", "L2"] and (Y.NORM_L1, Y.NORM_L2) == (1, 2)
    scoring = enum("ScoringType")
    assert scoring == ["L1_NORM", "L2_NORM", "CHI_SQUARE", "KL", "BHATTACHARYYA", "DOT_PRODUCT"]
    so = open(os.path.join(dbow, "ScoringObject.h")).read()
    must = dict((n, (m, l)) for n, m, l in re.findall(r"class __SCORING_CLASS\((\w+), (true|false), (L1|L2)\);", so))
    classes = ["L1Scoring", "L2Scoring", "ChiSquareScoring", "KLScoring", "BhattacharyyaScoring", "DotProductScoring"]
    norms = [0 if must[c][0] == "false" else (1 if must[c][1] == "L1" else 2) for c in classes]
    hdr = open(os.path.join(ROOT, "include", "eaofusion", "ORBVocabulary.h")).read()
    assert "return scoring == 1 ? 2 : scoring == 5 ? 0 : 1;" in hdr and norms == [1 if s not in (1, 5) else (2 if s == 1 else 0) for s in range(6)]
    assert int(re.search(r"const int FORB::L\s*=\s*(\d+);", open(os.path.join(dbow, "FORB.cpp")).read()).group(1)) == Y.FORB_L == 32
