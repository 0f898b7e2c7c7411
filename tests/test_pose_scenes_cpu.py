"""CPU suite: the PoseOptimization round scenes (tests/pose_scenes.py) hold what tests/test_gpu_pose_rounds.py needs them to hold -- on the oracle alone.  Every scene is run
thirteen times (as built + twelve one-ulp perturbations of its inputs); the figures below are CONDITIONS on the scene lists, not measurements: a scene list that is edited
until the rejected trials, the retrial batches cut short or the rounds on 0 / 1 / 2 edges are gone fails here.

Reached by the lists as they stand (tools/pose_round_bands.py; its --search walks 720 + 10800 far_off and 240 scattered candidates): 57 decided iterations with 2 - 5
trials on far_off + 26 on scattered, 11 with 6 - 9 trials, 10 rounds that end on an accepted retrial in front of the end of its candidate batch, 15 / 14 / 14 decided
iterations with more than one trial in rounds 2 / 3 / 4 of far_off alone.  None of the counts the families are asked for had to be lowered."""
import numpy as np
import pytest

import pose_scenes as S
from lm_tolerances import POSE_ROUNDS_CHAOTIC_BAND, POSE_ROUNDS_CHI2_REL, POSE_ROUNDS_LAMBDA_REL, UPDATE_REL

SCENES = S.all_scenes()


@pytest.fixture(scope="module")
def runs(oracle):
    out = {}
    with np.errstate(all="ignore"):
        for name, (family, fn, args) in SCENES.items():
            p = fn(*args)
            out[name] = (p, S.oracle_runs(oracle, p))
    return out


def test_every_scene_keeps_its_tables_and_rounds_under_one_ulp(runs):
    for name, (p, rs) in runs.items():
        assert S.tables_agree(rs), name
        assert all(len(r["trace"]["round_start"]) == S.expected_rounds(p) for r in rs), name      # (boundary: the `< 10` rule; everything else: four rounds)


def test_the_sizes_straddle_every_launch_geometry():
    ns = sorted({a[0] for a in S.FAR_OFF})
    assert set(S.FAR_OFF_N) <= set(ns)
    for edge in (64, 256, 512, 1024):                      # one wave / pose_class boundaries of csrc/pose.hip: both sides
        assert any(n <= edge for n in ns) and edge in ns and edge + 1 in ns
    assert 63 in ns and max(ns) > 2048                     # ... and the global-memory variant
    assert {a[2] for a in S.FAR_OFF} == {0.0, 0.1, 0.3} and {a[3] for a in S.FAR_OFF} == {0.0, 0.3, 1.0}
    assert {a[0] for a in S.SCATTERED} == set(S.SCATTERED_N) and max(S.SCATTERED_N) > 192      # (four waves from 193 edges on)
    assert sorted((a[0], a[1]) for a in S.BOUNDARY) == [(3, 0), (7, 2), (7, 3), (9, 0), (10, 0)]


def test_the_decided_prefixes_hold_rejected_trials_in_every_round(runs):
    few = many = refresh = 0
    per_round = np.zeros(4, int)
    for name, (p, rs) in runs.items():
        if SCENES[name][0] not in ("far_off", "scattered"):
            continue
        st = S.stats(len(p["points"]), rs, S.decided(rs))
        few += st["few"]; many += st["many"]; refresh += st["refresh"]
        per_round += np.array(st["per_round"])
    assert few >= 10, few              # iterations with 2 - 5 trials
    assert many >= 3, many             # ... with 6 - 9
    assert refresh >= 1, refresh       # rounds that end on an accepted retrial which is not the last of its candidate batch: the kernel's kRefresh pass
    assert (per_round[1:] >= 2).all(), per_round


def test_scattered_has_rounds_on_no_one_and_two_edges(runs):
    seen = set()
    for name, (p, rs) in runs.items():
        if SCENES[name][0] != "scattered":
            continue
        t = rs[0]["trace"]
        for act, (s, e) in zip(t["round_active"][1:], S.rounds_of(t)[1:]):
            seen.add(int(act))
            assert (e > s) == (act > 0), name          # g2o makes no iteration without a level-0 edge
    assert {0, 1, 2} <= seen, seen
    for a in S.ALL_EXCLUDED:                               # every edge excluded after round 1: no iteration afterwards, the input pose comes back
        p, rs = runs["scattered n=%d seed=%d" % a]
        for r in rs:
            assert list(r["trace"]["round_active"][1:]) == [0, 0, 0] and len(r["trace"]["trials"]) == r["trace"]["round_start"][1]
        assert np.array_equal(rs[0]["Tcw"], p["Tcw"]) and rs[0]["n_inliers"] == 0


def test_boundary_scenes_stop_where_the_rule_says(runs):
    for a in S.BOUNDARY:
        p, rs = runs["boundary n=%d planes=%d seed=%d" % a]
        assert len(rs[0]["trace"]["round_start"]) == (1 if a[0] + a[1] < 10 else 4)


def test_zero_depth_is_the_same_in_all_runs(runs):
    p, rs = runs["zero_depth"]
    t = rs[0]["trace"]
    assert not np.isfinite(t["chi2"]).any() and list(t["trials"]) == [1] * 10
    for r in rs[1:]:
        for k in ("trials", "chi2", "lam"):
            assert np.array_equal(r["trace"][k], t[k], equal_nan=True), k
        assert np.array_equal(r["outlier"], rs[0]["outlier"])


def test_admission_and_the_bounds_cover_the_oracles_own_runs(runs):
    """every far_off / scattered scene is inside the admission figures; every perturbed run of every scene passes the comparison the device is put through (the
    bounds are four times the largest spread, so this also pins the comparator); at most a quarter of the scenes is on the chaotic list, each with its band"""
    for name, (p, rs) in runs.items():
        dec = S.decided(rs)
        sc, sl = S.spread(rs, dec)
        if SCENES[name][0] in ("far_off", "scattered"):
            assert sc <= S.ADMIT_CHI2_SPREAD and sl <= S.ADMIT_LAMBDA_SPREAD, (name, sc, sl)
        for r in rs[1:]:
            bad, _, _ = S.compare_rounds(r["trace"], rs[0]["trace"], dec, POSE_ROUNDS_CHI2_REL, POSE_ROUNDS_LAMBDA_REL)
            assert not bad, (name, bad)
        band = S.pose_band(rs, p)
        assert (band > UPDATE_REL) == (name in POSE_ROUNDS_CHAOTIC_BAND), (name, band)
        if name in POSE_ROUNDS_CHAOTIC_BAND:
            assert "%.3e" % band == "%.3e" % POSE_ROUNDS_CHAOTIC_BAND[name]
    assert set(POSE_ROUNDS_CHAOTIC_BAND) <= set(SCENES) and 4 * len(POSE_ROUNDS_CHAOTIC_BAND) <= len(SCENES)


def test_the_comparator_sees_a_wrong_trace(runs):
    p, rs = runs["far_off n=512 seed=5003 out=0.1 mono=1"]
    ref, dec = rs[0]["trace"], S.decided(rs)
    ok = lambda t: not S.compare_rounds(t, ref, dec, POSE_ROUNDS_CHI2_REL, POSE_ROUNDS_LAMBDA_REL)[0]      # noqa: E731
    assert ok(ref)
    s2 = int(ref["round_start"][1])
    for key, f in (("trials", lambda v: v + 1), ("chi2", lambda v: v * (1 + 2 * POSE_ROUNDS_CHI2_REL)), ("lam", lambda v: v * (1 + 2 * POSE_ROUNDS_LAMBDA_REL))):
        t = {k: np.array(v) for k, v in ref.items()}
        t[key][s2 + 1] = f(t[key][s2 + 1])              # the second iteration of round 2
        assert not ok(t), key
    t = {k: np.array(v) for k, v in ref.items()}
    t["round_start"] = t["round_start"][:1]
    assert not ok(t)
    t = {k: np.array(v) for k, v in ref.items()}
    t["round_start"][2] = t["round_start"][3]             # round 3 without iterations
    assert not ok(t)
