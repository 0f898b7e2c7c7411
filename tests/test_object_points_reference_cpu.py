"""The yardstick of the point-list update (tests/object_points_reference.py) without a device: upstream's literal form and the device's form agree on every
scene, every scene shows what it claims, the recorded results (tests/golden/object_points/results.npz) are what the yardstick computes, and the literals of the
yardstick, the internal header and the adapter are those of the reference text (tests/golden/object_points_constants.json)."""
import os
import sys

import numpy as np
import pytest

import object_points_reference as Y
import object_points_scenes as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden_object_points as GG  # noqa: E402
import reference_literals as RL  # noqa: E402

SCENES = SC.scenes()
NAMES = sorted(SCENES)


@pytest.fixture(scope="module")
def results():
    return {name: (Y.literal(SCENES[name]), Y.device(SCENES[name])) for name in NAMES}


@pytest.mark.parametrize("name", NAMES)
def test_literal_and_device_form_agree(results, name):
    lit, dev = results[name]
    assert Y.differences(lit, dev) == []


@pytest.mark.parametrize("name", NAMES)
def test_scene_shows_what_it_claims(results, name):
    lit, _ = results[name]
    for key, want in SCENES[name]["claims"].items():
        if key == "variant":
            assert Y.variant(SCENES[name]) == want
        elif key in Y.RECORD_DTYPE.names:
            got = lit["rec"][key]
            if Y.RECORD_DTYPE[key].base.kind == "f":
                assert Y.same_float(np.asarray(got, np.float32), np.asarray(want, np.float32)), (key, got)
            else:
                assert np.array_equal(got, want), (key, got)
        else:
            assert np.array_equal(lit[key], np.asarray(want).reshape(np.asarray(lit[key]).shape)), (key, lit[key])


def test_the_scenes_cover_the_sizes_and_the_branches():
    sizes = {(len(s["map_points"]), len(s["cand_points"])) for s in SCENES.values()}
    for edge in (64, SC.BLOCK, SC.TILE):
        assert {edge - 1, edge, edge + 1} <= {m for m, _ in sizes} | {m + c - 1 for m, c in sizes}
    assert {SC.CAND_BLOCK - 1, SC.CAND_BLOCK, SC.CAND_BLOCK + 1} <= {c for _, c in sizes}
    res = [Y.literal(s) for s in SCENES.values()]
    assert {int(r["rec"]["status"]) for r in res} == {Y.DONE, Y.REJECTED, Y.UNDEFINED}
    assert {SC.CHUNK - 1, SC.CHUNK, SC.CHUNK + 1} <= {int(r["rec"]["n_appended"]) for r in res}
    done = [(s, r) for s, r in zip(SCENES.values(), res) if r["rec"]["status"] == Y.DONE]
    for erase in (Y.ERASE_PROJECTION, Y.ERASE_BOX, Y.ERASE_SHRUNK):
        assert any(s.get("erase", 0) == erase and r["rec"]["n_erased"] > 0 and r["rec"]["n_survivors"] > 0 for s, r in done)
    for gate in (Y.GATE_RADIUS, Y.GATE_CUBOID):
        assert any(s.get("gate", 0) == gate and 0 < r["rec"]["n_gated"] < len(s["cand_points"]) for s, r in done)
    # an appended candidate that a later one targets, and an erased appended candidate
    assert any((r["target"] >= len(s["map_points"])).any() for s, r in done)
    assert any(s.get("erase", 0) == Y.ERASE_PROJECTION and (r["erased"][len(s["map_points"]):] == 1).any() for s, r in done)


def test_equal_positions_share_their_gate():
    """what lets the device compare all pairs at once: the gate is a function of the position, and -0.0f beside +0.0f does not change it"""
    rng = np.random.default_rng(5)
    base = Y.full(dict(SCENES["three_equal_candidates_cuboid"]))
    for gate in (Y.GATE_RADIUS, Y.GATE_CUBOID):
        d = dict(base, gate=gate, center=np.float32([0.0, -0.0, 0.1]), rmax=np.float32(0.1))
        for _ in range(200):
            p = (rng.standard_normal(3) * 0.2).astype(np.float32)
            p[rng.integers(0, 3)] = 0.0
            q = p.copy()
            q[p == 0] = -0.0
            assert Y.gate_of(d, p) == Y.gate_of(d, q)


def test_recorded_results(results):
    z = np.load(GG.PATH)
    out = GG.build({name: results[name][1] for name in NAMES}, SCENES)
    assert GG.same_as_recorded(z, out) == []


def test_literals():
    lit = RL.literals("object_points")      # (held to the reference text by tests/test_reference_literals.py)
    assert float(lit["TH_MANY_FRAMES"]) == Y.TH_MANY_FRAMES and int(lit["MANY_FRAMES"]) == Y.MANY_FRAMES and int(lit["KEEP_COUNT"]) == Y.KEEP_COUNT
    assert int(lit["EDGE_PIXELS"]) == Y.EDGE_PIXELS and float(lit["CUBOID_SLACK"]) == Y.CUBOID_SLACK
    assert float(lit["MIN_IOU"]) == Y.MIN_IOU and float(lit["MIN_IOU_FORMER"]) == Y.MIN_IOU_FORMER
    h = open(os.path.join(ROOT, "eao_fusion_amd", "csrc", "object_points_internal.h")).read()
    for line in ("constexpr double kThManyFrames = %s;" % lit["TH_MANY_FRAMES"], "constexpr int32_t kManyFrames = %s;" % lit["MANY_FRAMES"],
                 "constexpr int32_t kKeepCount = %s;" % lit["KEEP_COUNT"], "constexpr int32_t kEdgePixels = %s;" % lit["EDGE_PIXELS"],
                 "constexpr double kCuboidSlack = %s;" % lit["CUBOID_SLACK"], "constexpr double kMinIou = %s;" % lit["MIN_IOU"],
                 "constexpr double kMinIouFormer = %s;" % lit["MIN_IOU_FORMER"]):
        assert line in h, line
    hip = open(os.path.join(ROOT, "eao_fusion_amd", "csrc", "object_points.hip")).read()
    for line in ("constexpr int kTile = %d;" % SC.TILE, "constexpr int kCandBlock = %d;" % SC.CAND_BLOCK, "constexpr int kChunk = %d;" % SC.CHUNK,
                 "constexpr int kBlock = %d;" % SC.BLOCK):
        assert line in hip, line
