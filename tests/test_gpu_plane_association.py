"""The plane association on the device (eao_plane_map_*; csrc/plane_map.hip, csrc/plane_map_internal.h) against the yardstick tests/plane_association_reference.py
on the scenes of tests/plane_association_scenes.py.  Every comparison is exact: indices and flags with array_equal, floats as their 32-bit patterns.  There is no
tolerance anywhere in this file -- the resident clouds included: the transform is held to the yardstick bit for bit, and the query tests replay the yardstick on the
device's own read-back points and world positions as well, so that each of the two is held on its own."""
import ctypes as C
import os
import threading

import numpy as np
import pytest
import torch  # noqa: F401  (before the library loads, so that both resolve the same HIP runtime)

import plane_association_reference as Y
import plane_association_scenes as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "plane_association")
KEYS = ("world_coef", "gated", "dis", "match", "match_dis")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def load(sc, pm=None):
    from eao_fusion_amd.plane_map import PlaneMap
    pm = pm or PlaneMap()
    for pid, w, xyz, T in sc["planes"]:
        pm.add(pid, w, xyz, T)
    return pm


def query(pm, sc, **kw):
    args = dict(cand_id=sc["cand_id"], set_start=sc["set_start"], dis_th=sc["dis_th"], angle_th=sc["angle_th"], full=True)
    args.update(kw)
    return pm.associate(sc["M"], sc["coef"], **args)


def replayed(pm, sc, ids):
    """the yardstick on what the device holds: read-back clouds and world positions of the candidates"""
    back = {pid: pm.boundary(pid) for pid in set(ids)}
    return Y.associate(sc["M"], sc["set_start"], sc["coef"], [(back[i][1], back[i][0]) for i in ids], sc["dis_th"], sc["angle_th"], vectorised=True)


def assert_same(got, want, what):
    for k in KEYS:
        assert got[k].shape == want[k].shape, "%s %s shape" % (what, k)
        assert np.array_equal(bits(got[k]), bits(want[k])), "%s %s" % (what, k)


def cand_ids(sc):
    return sc["cand_id"] if sc["cand_id"] is not None else [p[0] for p in sc["planes"]]


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SC.SCENES))
def test_resident_clouds_are_the_yardsticks_bit_for_bit(name):
    sc = SC.get(name)
    pm = load(sc)
    assert pm.info()["n_live"] == len(sc["planes"]) and pm.info()["n_points_in_use"] == sum(len(p[2]) for p in sc["planes"])
    for pid, w, xyz, T in sc["planes"]:
        got, gw = pm.boundary(pid)
        assert got.shape == (len(xyz), 3)
        assert np.array_equal(bits(got), bits(Y.transform_cloud_vectorised(xyz, T))), "%s plane %d" % (name, pid)
        assert np.array_equal(bits(gw), bits(w))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SC.SCENES))
def test_every_scene_complete_matrix_flags_and_matches(name):
    sc = SC.get(name)
    pm = load(sc)
    got = query(pm, sc)
    assert_same(got, replayed(pm, sc, cand_ids(sc)), name + " (read-back)")
    assert_same(got, SC.reference(name), name)      # the literal loops on the yardstick's own transform
    lean = query(pm, sc, full=False)
    assert sorted(lean) == ["match", "match_dis"]
    assert np.array_equal(lean["match"], got["match"]) and np.array_equal(bits(lean["match_dis"]), bits(got["match_dis"]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["three_sets", "room_1"])
def test_a_batch_equals_single_calls(name):
    sc = SC.get(name)
    pm = load(sc)
    if name == "room_1":      # the room seen by four keyframes, the second without planes
        rs = np.random.RandomState(3)
        M = np.array([sc["M"][0]] + [SC.pose(rs).astype(np.float32) for _ in range(3)])
        coef = np.concatenate([sc["coef"], sc["coef"][::-1], sc["coef"][:2]])
        n = len(sc["coef"])
        start = [0, n, n, 2 * n, 2 * n + 2]
    else:
        M, coef, start = sc["M"], sc["coef"], sc["set_start"].tolist()
    whole = pm.associate(M, coef, set_start=start, cand_id=sc["cand_id"], full=True)
    for s in range(len(M)):
        one = pm.associate(M[s], coef[start[s]:start[s + 1]], cand_id=sc["cand_id"], full=True)
        for k in KEYS:
            assert np.array_equal(bits(one[k]), bits(whole[k][start[s]:start[s + 1]])), "%s set %d %s" % (name, s, k)


@pytest.mark.gpu
def test_null_candidate_list_is_add_order():
    sc = SC.get("room_2")
    pm = load(sc)
    assert_same(query(pm, sc, cand_id=None), query(pm, sc, cand_id=[p[0] for p in sc["planes"]]), "NULL against the list")
    ids = [p[0] for p in sc["planes"]][::-1]
    assert_same(query(pm, sc, cand_id=ids), replayed(pm, sc, ids), "reversed list")
    none = pm.associate(sc["M"], sc["coef"], cand_id=[], full=True)
    assert none["match"].tolist() == [-1] * len(sc["coef"]) and none["dis"].shape == (len(sc["coef"]), 0)
    assert np.array_equal(bits(none["match_dis"]), bits(np.full(len(sc["coef"]), Y.DIS_TH, np.float32)))


def _big_cloud(rs, n, z):
    c = SC.at_height(np.full(n, z, np.float32), int(rs.randint(1 << 30)))
    c[-1, 2] = np.float32(z) / 2      # the minimum at the last point
    return c


@pytest.mark.gpu
def test_update_erase_readd_growth_and_compaction_against_a_fresh_handle():
    from eao_fusion_amd.plane_map import PlaneMap
    rs = np.random.RandomState(9)
    pm, m = PlaneMap(), Y.Model()

    def both(op, *a):
        getattr(pm, op)(*a)
        getattr(m, op)(*a)

    def check(what):
        info = pm.info()
        assert (info["n_live"], info["n_points_in_use"]) == (len(m.live()), m.used), what
        fresh = PlaneMap()
        for e in m.live():
            fresh.add(e[0], e[3], e[4])
        coef = np.array([[0, 0, 1, 0], [0, 0, -1, 0.01], [0, 0, 1, -0.05]], np.float32)
        ids = [e[0] for e in m.live()]
        for cand in (None, ids[::-1]):
            a = pm.associate(SC.I4, coef, cand_id=cand, full=True)
            assert_same(a, fresh.associate(SC.I4, coef, cand_id=cand, full=True), what + " against a fresh handle")
            assert_same(a, Y.associate(SC.I4, None, coef, m.candidates(cand), vectorised=True), what + " against the yardstick")
        return info

    for k in range(5):
        both("add", k, SC.UP, _big_cloud(rs, 1500 + k, 0.02 * (k + 1)))
    cap0 = check("five planes")["arena_capacity"]
    for k in range(5, 9):      # past the initial arena
        both("add", k, SC.UP if k % 2 else -SC.UP, _big_cloud(rs, 1500 + k, 0.02 * (k + 1)))
    assert check("nine planes")["arena_capacity"] > cap0
    both("update_boundary", 0, _big_cloud(rs, 700, 0.3))      # the nearest plane moves away
    both("set_world_pos", 1, np.array([1, 0, 0, 0], np.float32))      # ... and the next one turns out of the gate
    check("updated")
    c0 = m.compactions
    for k in (2, 3, 4, 5, 6):
        both("erase", k)
    assert m.compactions > c0 and pm.info()["n_points_in_use"] == m.used
    check("erased and compacted")
    both("add", 3, SC.UP, _big_cloud(rs, 65, 0.001))      # an erased id comes back
    both("update_boundary", 8, np.zeros((0, 3), np.float32))
    check("re-added")
    pm.erase(12345)      # unknown: a no-op
    check("after a no-op")
    both("clear")
    assert pm.info()["n_live"] == 0 and pm.associate(SC.I4, [SC.UP], full=True)["match"].tolist() == [-1]


@pytest.mark.gpu
def test_two_calls_return_the_same_bytes():
    for name in ("room_0", "sizes", "three_sets"):
        sc = SC.get(name)
        pm = load(sc)
        a, b = query(pm, sc), query(pm, sc)
        assert all(a[k].tobytes() == b[k].tobytes() for k in KEYS)
        c = query(load(sc), sc)      # and so does another handle
        assert all(a[k].tobytes() == c[k].tobytes() for k in KEYS)


@pytest.mark.gpu
@pytest.mark.parametrize("shared", [True, False])
def test_four_host_threads(shared):
    sc = SC.get("room_0")
    pms = [load(sc)] * 4 if shared else [load(sc) for _ in range(4)]
    want = SC.reference("room_0")
    errors = []

    def work(pm, t):
        try:
            for it in range(6):
                if it % 2:      # a plane of the thread's own comes and goes between the queries (it is not among the candidates)
                    pm.add(1000 + t, SC.UP, SC.at_height([0.5] * (50 + t)))
                    pm.erase(1000 + t)
                assert_same(query(pm, sc, cand_id=cand_ids(sc)), want, "thread %d" % t)
        except Exception as e:      # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(pms[t], t)) for t in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


@pytest.mark.gpu
def test_invalid_arguments_leave_outputs_and_state_untouched():
    from eao_fusion_amd import _lib
    sc = SC.get("later_closer")
    pm = load(sc)
    L = _lib.load()
    before = pm.info()
    M, coef = SC.I4.reshape(16).copy(), np.array([SC.UP, SC.UP], np.float32)
    start = np.array([0, 2], np.int32)
    SENT = 0x5A

    def call(n_sets=1, M=M, start=start, coef=coef, n_cand=3, cand=np.array([1, 2, 3], np.uint64), h=pm.h):
        out = [np.full(2, SENT, np.int32), np.full(2, SENT, np.float32), np.full(8, SENT, np.float32), np.full(6, SENT, np.float32), np.full(6, SENT, np.uint8)]
        st = L.eao_plane_map_associate(h, n_sets, _lib.ptr(M), _lib.ptr(start), _lib.ptr(coef), n_cand, _lib.ptr(cand), 0.2, 0.8, *[_lib.ptr(o) for o in out])
        return st, all((o == SENT).all() for o in out)

    assert call() == (_lib.EAO_OK, False)
    bad = [dict(cand=np.array([1, 2, 99], np.uint64)), dict(n_sets=-1), dict(start=np.array([1, 2], np.int32)), dict(start=np.array([0, -1], np.int32)),
           dict(n_cand=-1), dict(n_cand=2, cand=None), dict(M=None), dict(coef=None), dict(h=None), dict(start=np.array([0, 5000], np.int32)),
           dict(n_cand=(1 << 16) + 1)]
    for kw in bad:
        assert call(**kw) == (_lib.EAO_ERR_INVALID, True), kw
    # match / match_dis are required when there are rows
    assert L.eao_plane_map_associate(pm.h, 1, _lib.ptr(M), _lib.ptr(start), _lib.ptr(coef), 3, None, 0.2, 0.8, None, None, None, None, None) == _lib.EAO_ERR_INVALID
    w, xyz = SC.UP.copy(), np.zeros((2, 3), np.float32)
    n = C.c_int32(77)
    buf = np.full((4, 3), SENT, np.float32)
    assert L.eao_plane_map_add(pm.h, 1, _lib.ptr(w), 2, _lib.ptr(xyz), None) == _lib.EAO_ERR_INVALID      # a live id
    assert L.eao_plane_map_add(pm.h, 50, _lib.ptr(w), -1, _lib.ptr(xyz), None) == _lib.EAO_ERR_INVALID
    assert L.eao_plane_map_add(pm.h, 50, _lib.ptr(w), 2, None, None) == _lib.EAO_ERR_INVALID
    assert L.eao_plane_map_add(pm.h, 50, None, 2, _lib.ptr(xyz), None) == _lib.EAO_ERR_INVALID
    assert L.eao_plane_map_add(pm.h, 50, _lib.ptr(w), (1 << 20) + 1, _lib.ptr(xyz), None) == _lib.EAO_ERR_INVALID
    assert L.eao_plane_map_update_boundary(pm.h, 50, 2, _lib.ptr(xyz), None) == _lib.EAO_ERR_INVALID      # not held
    assert L.eao_plane_map_set_world_pos(pm.h, 50, _lib.ptr(w)) == _lib.EAO_ERR_INVALID
    assert L.eao_plane_map_boundary(pm.h, 50, 4, _lib.ptr(buf), C.byref(n), None) == _lib.EAO_ERR_INVALID
    assert L.eao_plane_map_boundary(pm.h, 1, 0, _lib.ptr(buf), C.byref(n), None) == _lib.EAO_ERR_INVALID      # cap below the count
    assert n.value == 77 and (buf == SENT).all()
    assert pm.info() == before
    assert_same(query(pm, sc), SC.reference("later_closer"), "after the refusals")


@pytest.fixture(scope="module")
def scale():
    sc = SC.scale_scene()
    want = Y.associate(sc["M"], sc["set_start"], sc["coef"], [(p[1], p[2]) for p in sc["planes"]], vectorised=True)
    for a in want.values():
        a.setflags(write=False)
    return sc, want


@pytest.mark.gpu
def test_scale_300_planes_of_2000_points_12_rows(scale):
    sc, want = scale
    assert len(sc["planes"]) == 300 and len(sc["coef"]) == 12 and all(len(p[2]) == 2000 for p in sc["planes"])
    assert (want["match"] >= 0).all() and 12 < int(want["gated"].sum()) < 3600      # (random planes cross: a cloud of another plane may be the nearer one)
    pm = load(sc)
    assert pm.info()["n_points_in_use"] == 600000
    assert_same(query(pm, sc), want, "scale")


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(f[:-4] for f in os.listdir(GOLDEN) if f.endswith(".npz")))
def test_golden_files(name):
    from eao_fusion_amd.plane_map import PlaneMap
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    pm = PlaneMap()
    st = g["cloud_start"]
    for k, pid in enumerate(g["plane_id"]):
        pm.add(int(pid), g["plane_world"][k], g["cloud_xyz"][st[k]:st[k + 1]], g["Tcw"][k] if g["has_Tcw"][k] else None)
        assert np.array_equal(bits(pm.boundary(int(pid))[0]), bits(g["expect_world_xyz"][st[k]:st[k + 1]])), "%s plane %d" % (name, pid)
    got = pm.associate(g["M"], g["coef"], cand_id=g["cand_id"] if g["has_cand"] else None, set_start=g["set_start"], dis_th=g["dis_th"], angle_th=g["angle_th"],
                       full=True)
    assert_same(got, {k: g["expect_" + k] for k in KEYS}, name)


@pytest.mark.gpu
def test_the_chain_scene_add_associate_pose_optimization():
    """the associated planes as the plane edges of eao_pose_optimization: equal to the same pose problem built from the yardstick's association"""
    from eao_fusion_amd import synth
    from eao_fusion_amd.optimizer import Optimizer
    from eao_fusion_amd.plane_map import PlaneMap
    prob = synth.synth_pose(n=150, seed=4100, n_planes=4)
    rs = np.random.RandomState(2)
    worlds = [np.asarray(w, np.float64) for w in prob["plane_world"]] + [np.array([0.6, 0.0, 0.8, 7.0]), np.array([0.0, 1.0, 0.0, 9.0])]      # two nobody sees
    pm, m, ids = PlaneMap(), Y.Model(), []
    for k in rs.permutation(len(worlds)):
        w = worlds[k]
        n = w[:3] / np.linalg.norm(w[:3])
        a = np.cross(n, [0.3, 0.5, 0.8]); a /= np.linalg.norm(a)
        b = np.cross(n, a)
        uv = rs.uniform(-2, 2, (300, 2))
        X = (-w[3] / np.linalg.norm(w[:3]) * n + uv[:, :1] * a + uv[:, 1:] * b).astype(np.float32)
        pm.add(100 + int(k), w.astype(np.float32), X)
        m.add(100 + int(k), w.astype(np.float32), X)
        ids.append(100 + int(k))
    order = sorted(ids)      # std::set order of the map
    obs = np.asarray(prob["plane_obs"], np.float64)
    coef = (obs / np.linalg.norm(obs[:, :3], axis=1, keepdims=True)).astype(np.float32)      # mvPlaneCoefficients carry unit normals; synth's edges do not
    got = pm.associate(prob["Tcw"], coef, cand_id=order)
    want = Y.associate(prob["Tcw"], None, coef, m.candidates(order), vectorised=True)
    assert np.array_equal(got["match"], want["match"]) and (got["match"] >= 0).sum() >= 3

    def problem(match):
        keep = [i for i, j in enumerate(match) if j >= 0]
        p = dict(prob)
        p["plane_world"] = np.array([m.candidates([order[match[i]]])[0][0] for i in keep], np.float32)
        p["plane_obs"] = np.asarray(prob["plane_obs"], np.float32)[keep]
        p["plane_seen"] = np.asarray(prob["plane_seen"], np.uint8)[keep]
        return p

    a, b = Optimizer.PoseOptimization(problem(got["match"])), Optimizer.PoseOptimization(problem(want["match"]))
    assert np.array_equal(bits(a["Tcw"]), bits(b["Tcw"])) and np.array_equal(a["outlier"], b["outlier"]) and np.array_equal(a["plane_outlier"], b["plane_outlier"])
    assert a["n_inliers"] == b["n_inliers"] and a["n_inliers"] > 100
