"""The KeyFrameDatabase yardstick (tests/keyframe_database_reference.py) and its scenes (tests/keyframe_database_scenes.py) held on their own, without a device:
a hand-computed example, every scene reaching the branch it claims, the float-against-double truncation search, and the literals 0.8f, 0.75f and the ten
neighbours against the reference text."""
import os
import re
import sys

import numpy as np
import pytest

import keyframe_database_reference as Y
import keyframe_database_scenes as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from reference_literals import literals  # noqa: E402


def test_hand_computed_example():
    # words 1 2 3 4; A holds {1, 2, 3}, B {3, 4}, C {2}; the query holds {2, 3, 4} with 0.5, 0.25, 0.25
    db = Y.Database(10)
    for k, ids, vals in ((5, [1, 2, 3], [0.5, 0.25, 0.25]), (6, [3, 4], [0.5, 0.5]), (7, [2], [1.0])):
        db.add(Y.KeyFrame(k, (ids, vals)))
    q = ([2, 3, 4], [0.5, 0.25, 0.25])
    assert db.intersect(q) == [(5, 2, 2, 0.5), (6, 2, 3, 0.5), (7, 1, 2, 0.5)]
    r = db.detect_relocalization_candidates(9, q, {5: [6], 6: [], 7: [5, 6]}.get)
    # word 2's list is [A, C], word 3's [A, B]: A and C enter at word 2 in add order, B at word 3
    assert r["sharing_id"] == [5, 7, 6] and r["sharing_words"] == [2, 1, 2] and (r["max_common_words"], r["min_common_words"], r["n_scores"]) == (2, 1, 2)
    assert r["scored_id"] == [5, 6] and r["scored_score"] == [np.float32(0.5)] * 2
    # A + its neighbour B = 1.0; B alone 0.5 is not above 0.75; C was listed by this query but never scored: not among the scored, so never a start
    assert r["acc_score"] == [np.float32(1.0), np.float32(0.5)] and r["best_id"] == [5, 6] and r["cand_id"] == [5] and r["used_unset"] == 0
    # the loop kind with A connected: A's count ends at 1 and it is not listed; with query id 9 again nothing would be listed at all
    l = db.detect_loop_candidates(10, q, [5], 0.1, {5: [6], 6: [5, 7], 7: [5, 6]}.get)
    assert l["sharing_id"] == [7, 6] and db.held[5].mnLoopWords == 1 and db.held[5].mnLoopQuery == 0
    assert l["scored_id"] == [6] and l["cand_id"] == [6] and l["used_unset"] == 0      # (7: one word, not above int(2 * 0.8f) = 1; 5: mnLoopQuery is not 10)


@pytest.mark.parametrize("name", sorted(SC.SCENES))
def test_every_scene_reaches_the_branch_it_claims(name):
    sc = SC.get(name)
    assert sc["claim"] and sc["check"](SC.reference(name)), sc["claim"]


def test_no_count_truncates_differently_in_float_and_double():
    assert SC.float_truncation_differs(8192) == []
    assert [int(np.float32(m) * np.float32(0.8)) for m in (1, 4, 5, 6, 10, 11, 125)] == [0, 3, 4, 4, 8, 8, 100]


def test_yardstick_state_follows_upstream():
    kf = Y.KeyFrame(3)
    assert (kf.mnLoopQuery, kf.mnLoopWords, kf.mLoopScore, kf.mnRelocQuery, kf.mnRelocWords, kf.mRelocScore) == (0, 0, None, 0, 0, None)
    R = SC.reference("repeated_query_id")
    assert R[1]["res"]["sharing_words"] == R[0]["res"]["sharing_words"]      # (the two kinds count alike)
    R = SC.reference("every_sharer_connected")
    assert not R[0]["res"]["sharing_id"]


def test_header_and_yardstick_spell_the_fixture():
    lit = literals("keyframe_database")
    assert set(lit) == {"MIN_COMMON_WORDS_FACTOR", "MIN_SCORE_TO_RETAIN_FACTOR", "N_NEIGHBOURS"}
    hdr = open(os.path.join(ROOT, "eao_fusion_amd", "csrc", "keyframe_db_internal.h")).read()
    assert "maxCommonWords * %s" % lit["MIN_COMMON_WORDS_FACTOR"] in hdr and "%s * bestAccScore" % lit["MIN_SCORE_TO_RETAIN_FACTOR"] in hdr
    assert Y.N_NEIGHBOURS == int(lit["N_NEIGHBOURS"])


def test_literals_equal_the_reference_text():
    """What the fixture's six rows do not say: each literal stands at no third site, bestAccScore starts where upstream starts it, and the KeyFrame
    constructor leaves the scores unset."""
    ref = os.environ.get("EAO_REFERENCE_DIR")
    if not ref or not os.path.exists(os.path.join(ref, "src", "KeyFrameDatabase.cc")):
        pytest.skip("EAO_REFERENCE_DIR does not name a reference tree")
    lit = {k: re.escape(v) for k, v in literals("keyframe_database").items()}
    src = open(os.path.join(ref, "src", "KeyFrameDatabase.cc")).read()
    assert len(re.findall(r"int minCommonWords = maxCommonWords\*%s;" % lit["MIN_COMMON_WORDS_FACTOR"], src)) == 2
    assert len(re.findall(r"float minScoreToRetain = %s\*bestAccScore;" % lit["MIN_SCORE_TO_RETAIN_FACTOR"], src)) == 2
    assert len(re.findall(r"GetBestCovisibilityKeyFrames\(%s\)" % lit["N_NEIGHBOURS"], src)) == 2
    assert "float bestAccScore = minScore;" in src and "float bestAccScore = 0;" in src
    kf = open(os.path.join(ref, "src", "KeyFrame.cc")).read()
    assert "mnLoopQuery(0), mnLoopWords(0), mnRelocQuery(0), mnRelocWords(0)" in kf and "mLoopScore(" not in kf and "mRelocScore(" not in kf
