"""Invariants of the guided-matching oracle (oracle/match_cpu.cpp; reference src/ORBmatcher.cc:45-129, 1328-1472).
No upstream fixtures exist, so the sequential restatement is checked against an independent numpy brute force of the
same rules (dense masks + greedy replay)."""
import numpy as np
import pytest

from eao_fusion_amd import synth


def _grid_cells(F):
    iw = np.float32(64) / np.float32(F["max_x"] - F["min_x"])
    ih = np.float32(48) / np.float32(F["max_y"] - F["min_y"])
    # C round(): half away from zero
    px = np.floor(np.abs((F["kp_x"] - F["min_x"]) * iw) + np.float32(0.5)) * np.sign((F["kp_x"] - F["min_x"]) * iw)
    py = np.floor(np.abs((F["kp_y"] - F["min_y"]) * ih) + np.float32(0.5)) * np.sign((F["kp_y"] - F["min_y"]) * ih)
    return px.astype(int), py.astype(int), iw, ih


def _brute_points(F, M, th, ratio):
    px, py, iw, ih = _grid_cells(F)
    N = len(px)
    ingrid = (px >= 0) & (px < 64) & (py >= 0) & (py < 48)
    order = sorted(np.nonzero(ingrid)[0], key=lambda i: (px[i], py[i], i))
    occ = F["occupied"].astype(bool).copy()
    out = np.full(len(M["level"]), -1)
    for m in range(len(out)):
        if M["skip"][m]:
            continue
        lvl = int(M["level"][m])
        r = np.float32(2.5 if M["view_cos"][m] > 0.998 else 4.0)
        if th != 1.0:
            r = np.float32(r * np.float32(th))
        rs = np.float32(r * F["scale_factors"][lvl])
        x, y = M["proj_x"][m], M["proj_y"][m]
        x0 = max(0, int(np.floor((x - F["min_x"] - rs) * iw))); x1 = min(63, int(np.ceil((x - F["min_x"] + rs) * iw)))
        y0 = max(0, int(np.floor((y - F["min_y"] - rs) * ih))); y1 = min(47, int(np.ceil((y - F["min_y"] + rs) * ih)))
        if x0 >= 64 or x1 < 0 or y0 >= 48 or y1 < 0:
            continue
        best, best2, bl, bl2, bi = 256, 256, -1, -1, -1
        for i in order:
            if not (x0 <= px[i] <= x1 and y0 <= py[i] <= y1):
                continue
            o = F["kp_octave"][i]
            if o < lvl - 1 or o > lvl:
                continue
            if not (abs(F["kp_x"][i] - x) < rs and abs(F["kp_y"][i] - y) < rs):
                continue
            if occ[i]:
                continue
            if F["u_right"][i] > 0 and abs(M["proj_xr"][m] - F["u_right"][i]) > rs:
                continue
            d = int(np.unpackbits(M["descriptors"][m] ^ F["descriptors"][i]).sum())
            if d < best:
                best2, best, bl2, bl, bi = best, d, bl, o, i
            elif d < best2:
                bl2, best2 = o, d
        if best <= 100:
            if bl == bl2 and best > np.float32(ratio) * best2:
                continue
            out[m] = bi
            occ[bi] = True
    return out


def test_points_search_vs_bruteforce(oracle):
    cur, last, mps = synth.synth_tracking(n=300, seed=7001)
    for th in (1.0, 3.0):
        nm, got = oracle.search_by_projection_points(cur, mps, th, 0.8)
        ref = _brute_points(cur, mps, th, 0.8)
        assert np.array_equal(got, ref)
        assert nm == (ref >= 0).sum() and nm > 100
        m = got[got >= 0]
        assert len(set(m)) == len(m)                    # a keypoint is claimed at most once
        assert not cur["occupied"][m].any()             # and never one that already held a map point
        assert not (got[mps["skip"] > 0] >= 0).any()


def test_frames_search_properties(oracle):
    cur, last, mps = synth.synth_tracking(n=400, seed=7002)
    nm, cm = oracle.search_by_projection_frames(cur, last, 7.0, False, True)
    nm0, cm0 = oracle.search_by_projection_frames(cur, last, 7.0, False, False)
    assert nm == (cm >= 0).sum() and nm0 == (cm0 >= 0).sum()
    assert 150 < nm <= nm0                                # the rotation histogram only removes matches
    k = np.nonzero(cm >= 0)[0]
    assert last["valid"][cm[k]].all() and not cur["occupied"][k].any()
    assert len(set(cm[k])) == len(k)
    # planted rotation is +12 deg: every surviving match sits in one of (at most) three histogram bins
    rot = (last["angle"][cm[k]] - cur["kp_angle"][k]) % 360
    bins = np.round(rot * np.float32(30 / 360.0)).astype(int) % 30
    assert len(set(bins)) <= 3
    # monocular flag widens the level window (no forward/backward test)
    nm_m, _ = oracle.search_by_projection_frames(cur, last, 7.0, True, True)
    assert nm_m > 0


# ---- contended scenes: the greedy order decides (tests/contention.py measures how much) -----------------------------------------------------
import contention  # noqa: E402

CONTENDED = {      # synth.synth_tracking_contended arguments of the scenes the CPU and GPU suites share
    "dups-chains-ties": dict(seed=7600),
    "long-chains": dict(seed=7601, n=200, dup_groups=20, chains=(200,), ratio_chains=(120,), ties=1),
    "hist-tenth": dict(seed=7602, hist={29: 40, 3: 4, 7: 3}, hist_only=True),
    "hist-equal": dict(seed=7603, hist={29: 40, 3: 4, 7: 4, 11: 4}, hist_only=True),
    "hist-contended": dict(seed=7604, n=100, dup_groups=20, chains=(60,), ratio_chains=(30,), hist={3: 30, 7: 30, 11: 30, 15: 30}),
}
MIN_DIFFER = 0.10      # of the greedy matches: queries whose outcome the claims of earlier queries change


@pytest.mark.parametrize("name", ["dups-chains-ties", "long-chains"])
@pytest.mark.parametrize("th", [1.0, 3.0])
def test_points_search_vs_bruteforce_contended(oracle, name, th):
    """SearchByProjection(Frame&, MapPoints) on scenes where earlier claims change later outcomes: the oracle against the numpy greedy replay,
    and the scene against its minimums (every category of the meter non-zero), so that a generator change cannot quietly take its teeth out."""
    cur, last, mps = synth.synth_tracking_contended(**CONTENDED[name])
    nm, got = oracle.search_by_projection_points(cur, mps, th, 0.8)
    ref, _, _ = contention.points(cur, mps, th, 0.8)
    assert np.array_equal(got, ref) and nm == (ref >= 0).sum()
    m = got[got >= 0]
    assert len(set(m)) == len(m) and not cur["occupied"][m].any()
    meter = contention.meter_points(cur, mps, th, 0.8)
    print("contention points %s th=%g: %s" % (name, th, meter))
    assert meter["differ"] >= MIN_DIFFER * meter["matched"], meter
    assert meter["differ_best"] > 0 and meter["differ_ratio"] > 0, meter
    assert meter["tie_equal"] > 0 and meter["tie_th"] > 0 and meter["tie_ratio"] > 0, meter


def test_points_bruteforce_agrees_with_the_replay_above(oracle):
    """The meter's vectorised replay and _brute_points are two restatements of one loop: the same table on a contended scene."""
    cur, last, mps = synth.synth_tracking_contended(seed=7605, n=150, dup_groups=15, chains=(40,), ratio_chains=(20,), ties=1)
    for th in (1.0, 3.0):
        assert np.array_equal(contention.points(cur, mps, th, 0.8)[0], _brute_points(cur, mps, th, 0.8))


FRAME_SCENES = [("plain-7002", dict(seed=7002, n=400), None), ("plain-moved", dict(seed=7006, n=600, moved=0.3), None),
                ("plain-back", dict(seed=7007, n=600, moved=-0.3), None)] + [(k, None, v) for k, v in CONTENDED.items()]


@pytest.mark.parametrize("name,plain,cont", FRAME_SCENES, ids=[s[0] for s in FRAME_SCENES])
def test_frames_search_vs_bruteforce(oracle, name, plain, cont):
    """SearchByProjection(Cur, Last, th, bMono) (src/ORBmatcher.cc:1328-1472): the oracle against a numpy brute force of the same rules --
    greedy claims, the forward / backward / both-ways level windows, the stereo gate, first of equal distances, the rotation histogram with
    ComputeThreeMaxima -- with and without the orientation check, stereo and monocular, on today's scenes and the contended ones."""
    cur, last, _ = synth.synth_tracking(**plain) if plain else synth.synth_tracking_contended(**cont)
    for th, mono, check in ((7.0, False, True), (15.0, False, False), (7.0, True, True)):
        onm, ocm = oracle.search_by_projection_frames(cur, last, th, mono, check)
        cm, nm, _, _, _ = contention.frames(cur, last, th, mono, check)
        assert onm == nm and np.array_equal(ocm, cm), (th, mono, check)
        assert nm > 20
    if cont is None:
        return
    meter = contention.meter_frames(cur, last, 7.0, False)
    print("contention frames %s: %s" % (name, meter))
    if cont.get("hist_only"):         # isolated probes: nothing to contend for, the histogram decides
        assert meter["hist_boundary"] > 0 and meter["kept"] < meter["matched"], meter
        assert meter["hist_tenth" if name == "hist-tenth" else "hist_equal"] > 0, meter
        return
    assert meter["differ"] >= MIN_DIFFER * meter["matched"] and meter["differ_best"] > 0, meter
    assert meter["tie_equal"] > 0 and meter["tie_th"] > 0, meter
    if name == "hist-contended":
        assert meter["hist_equal"] > 0 and meter["hist_boundary"] > 0, meter


def test_todays_scenes_decide_nothing():
    """Why the scenes above exist: on synth_tracking's scenes the greedy order changes no query (claims never meet a competitor)."""
    cur, last, mps = synth.synth_tracking(n=300, seed=7001)
    assert contention.meter_points(cur, mps, 1.0, 0.8)["differ"] == 0
    assert contention.meter_frames(cur, last, 7.0, False)["differ"] == 0
