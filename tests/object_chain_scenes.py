"""Seeded scenes of the chained update of a map object (tests/object_chain_reference.py is their yardstick).  A scene is a chain desc (an object_points desc with
map_bad, cand_bad, cand_alias, centroids, Ryaw, prev_cuboid_center, class_id, bi_forest) with `claims`: what the scene is there for, which
tests/test_object_chain_reference_cpu.py holds the yardstick to.  A claim is a field of the chain record, of the points record (`points.<field>`), of the cuboid
record (`cuboid.<field>`), or an output array."""
import numpy as np

import isolation_forest_reference as IF
import object_chain_reference as Y
import object_cuboid_reference as OC
import object_points_reference as OP
import object_points_scenes as PS

f32, f64 = np.float32, np.float64
CHUNK = 1024          # kChunk of csrc/object_cuboid.hip and kTile / kChunk of csrc/object_points.hip
LDS_BUDGET = 59392    # kLdsBudget of csrc/iforest_internal.h (tests/test_object_chain_reference_cpu.py reads it from there)


def lds_bytes(n):
    """LdsPlan::bytes of lds_plan(n, n / 2)"""
    s = n // IF.SAMPLE_DIVISOR
    return ((max(n, 2 * s) * 2 + 15) & ~15) + 12 * s


def lds_edge():
    """the largest n whose forest of n / 2 samples still has its working set in LDS"""
    n = 30
    while lds_bytes(n + 1) <= LDS_BUDGET:
        n += 1
    return n


def dress(rng, d, m=6, class_id=0, bi_forest=1, yaw=0.4, prev=(0.4, -0.2, 1.9), **claims):
    """the cuboid's and the forest's inputs on a points desc"""
    d = dict(d)
    d.update(centroids=PS.cloud(rng, m, spread=(0.05, 0.05, 0.05)), Ryaw=OC.ryaw(0.0, 0.0, yaw), prev_cuboid_center=np.array(prev, f64), class_id=class_id, bi_forest=bi_forest,
             map_bad=np.zeros(len(d["map_points"]), np.uint8), cand_bad=np.zeros(len(d["cand_points"]), np.uint8), claims=claims)
    return d


def alias_by_position(d):
    """a candidate at the position of a list entry IS that entry's MapPoint (the tracker sees a list entry again)"""
    mp, cp = np.asarray(d["map_points"], f32), np.asarray(d["cand_points"], f32)
    where = {tuple(p.tolist()): k for k, p in reversed(list(enumerate(mp)))}
    return np.array([where.get(tuple(p.tolist()), -1) for p in cp], np.int32)


def survivors_of(d):
    return Y.OP.device(dict(d, map_count=Y.raised_counts(d)))["survivors"]


def leave(rng, d, n_final):
    """bad flags on survivors picked at random until n_final stay"""
    surv = survivors_of(d)
    assert len(surv) >= n_final, (len(surv), n_final)
    for s, i in surv[rng.choice(len(surv), len(surv) - n_final, replace=False)]:
        (d["cand_bad"] if s else d["map_bad"])[i] = 1
    d["claims"]["n_final"] = n_final
    return d


def frame(rng, M, C, n_final=None, alias=True, **kw):
    """a DataAssociateUpdate as the tracker sees it (object_points_scenes.frame_update), dressed"""
    points_kw = {k: kw.pop(k) for k in list(kw) if k in ("rejected", "change_gate", "gate", "erase", "box_off_edge", "rmax", "n_frames_after_push")}
    d = dress(rng, PS.frame_update(rng, M, C, repeats=C // 3, **points_kw), **kw)
    if alias:
        d["cand_alias"] = alias_by_position(d)
    return d if n_final is None else leave(rng, d, n_final)


def plain(rng, n, n_bad=0, **kw):
    """a list of n + n_bad entries that only loses its bad points: no gate, no erase, no candidates"""
    d = dress(rng, PS.scene(PS.cloud(rng, n + n_bad), np.zeros((0, 3))), **kw)
    d["map_bad"][rng.choice(n + n_bad, n_bad, replace=False)] = 1
    d["claims"]["n_final"] = n
    return d


def scenes():
    out = {}
    rng = np.random.default_rng(20241021)
    # ---- the forest's size rule (:1256) and an odd and an even sample: n_final / 2 is 14, 15, 15
    for n, st in ((29, Y.FOREST_SKIPPED), (30, Y.FOREST_DONE), (31, Y.FOREST_DONE)):
        out["n_final_%d" % n] = frame(rng, 60, 12, n_final=n, forest_status=st)
    out["every_point_erased"] = frame(rng, 40, 6, n_final=0, forest_status=Y.FOREST_SKIPPED, **{"cuboid.status": OC.EMPTY})
    out["rejected"] = frame(rng, 80, 10, rejected=True, **{"points.status": OP.REJECTED})
    out["rejected"]["map_bad"][3] = 1
    und = frame(rng, 50, 5, **{"points.status": OP.UNDEFINED})
    und["map_points"][7] = [0.0, 5.0, 0.0]      # 0 * inf in the projection: a NaN
    out["undefined"] = und
    # ---- where the bad points sit
    for name, at in (("bad_point_first", 0), ("bad_point_last", -1)):
        d = frame(rng, 70, 9, erase=OP.ERASE_NONE)
        s, i = survivors_of(d)[at]
        (d["cand_bad"] if s else d["map_bad"])[i] = 1
        d["claims"]["n_final"] = len(survivors_of(d)) - 1
        out[name] = d
    d = frame(rng, 70, 9, erase=OP.ERASE_NONE)
    appended = [int(i) for s, i in survivors_of(d) if s == 1]
    d["cand_bad"][appended[1]] = 1
    d["claims"].update(n_final=len(survivors_of(d)) - 1, final_lacks=[1, appended[1]])
    out["bad_point_appended"] = d
    # ---- the alias rule: entry 0 projects outside the box with a count of 8 and is seen again; the gate lets the candidate in, the count step 4 reads is 9
    P = dict(PS.CAMERA, erase=OP.ERASE_PROJECTION, box_off_edge=1, box_rect=[10, 10, 10, 10], gate=OP.GATE_RADIUS, center=[0.0, 0.0, 0.0], rmax=1000.0)
    mp = PS.pixels([[50, 50], [15, 15], [52, 52]])
    base = dress(rng, PS.scene(mp, [mp[0], [70, 70, 1]], map_count=[8, 0, 8], cand_count=[8, 9], sum_pos=mp.sum(axis=0), **P), m=4)
    out["alias_raises_8_to_9"] = dict(base, cand_alias=np.array([0, -1], np.int32), claims=dict(erased=[0, 0, 1, 0], n_final=3))
    out["alias_null_erases"] = dict(base, claims=dict(erased=[1, 0, 1, 0], n_final=2))
    two = dress(rng, PS.scene(mp, [mp[0], mp[0], [4000, 0, 1]], map_count=[7, 0, 8], cand_count=[7, 8, 0], sum_pos=mp.sum(axis=0), **dict(P, rmax=100.0)), m=4)
    out["two_candidates_alias_one_entry"] = dict(two, cand_alias=np.array([0, 0, 2], np.int32), claims=dict(erased=[0, 0, 1], gate=[1, 1, 0], n_final=2))
    # ---- the forest's class rules
    out["class_75_is_exempt"] = frame(rng, 90, 8, class_id=75, forest_status=Y.FOREST_SKIPPED)
    out["class_62_threshold"] = frame(rng, 90, 8, class_id=62, forest_status=Y.FOREST_DONE)
    out["bi_forest_off"] = frame(rng, 90, 8, bi_forest=0, forest_status=Y.FOREST_SKIPPED)
    # ---- the cuboid's five-frame gate (:1071)
    out["four_centroids"] = frame(rng, 64, 6, m=4, **{"cuboid.bounds_written": 1})
    out["five_centroids"] = frame(rng, 64, 6, m=5, **{"cuboid.bounds_written": 0})
    # ---- final lists one below, at and above the chunk and the tile
    for n in (CHUNK - 1, CHUNK, CHUNK + 1):
        out["n_final_%d" % n] = plain(rng, n, n_bad=5, forest_status=Y.FOREST_DONE)
    out["frame_to_1024"] = frame(rng, 1100, 90, n_final=CHUNK, box_off_edge=0, forest_status=Y.FOREST_DONE)
    # ---- the two sides of the forest's LDS budget at S = n / 2
    edge = lds_edge()
    for n in (edge, edge + 1):
        out["n_final_%d" % n] = plain(rng, n, n_bad=3, forest_status=Y.FOREST_DONE)
    return out


def mixed_batch(n=32):
    """descs over the scenes, in an order that puts long and short lists, finished and unfinished updates side by side"""
    S = scenes()
    names = sorted(S)
    rng = np.random.default_rng(5)
    return [S[names[int(k)]] for k in rng.integers(0, len(names), n)]


def split_launch():
    """one desc on the two-launch side of kSplitPairs: 2048 x 2048"""
    rng = np.random.default_rng(99)
    return frame(rng, 2048, 2048, forest_status=Y.FOREST_DONE)
