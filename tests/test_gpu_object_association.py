"""The object layer's data association on the device (eao_object_np_counts_batch, eao_object_np_association_batch, eao_object_project_rects_batch;
csrc/object_assoc.hip) against the yardstick (tests/object_association_reference.py, the literal transcription of Object_2D::NoParaDataAssociation and
Object_Map::ComputeProjectRectFrame) and its recorded results (tests/golden/object_association/*.npz).  There is no tolerance anywhere: m, n, step, the counts,
the verdicts, the rects and their status are integers, and w, r, u and v are compared as bit patterns."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

import object_association_reference as Y
import object_association_scenes as SC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "object_association")
NP_SCENES, RECT_SCENES = SC.np_scenes(), SC.rect_scenes()
CAM = ("fx", "fy", "cx", "cy", "cols", "rows")
_want = {}


@pytest.fixture(scope="module")
def OA():
    from eao_fusion_amd import object_association
    return object_association


def want_np(name):
    if name not in _want:
        s = NP_SCENES[name]
        _want[name] = Y.np_literal(s["det"], s["map"], s["S"])
    return _want[name]


def want_rect(name):
    if ("rect", name) not in _want:
        s = RECT_SCENES[name]
        _want["rect", name] = Y.rect_literal(s["points"], s["Tcw"], **{k: s[k] for k in CAM})
    return _want["rect", name]


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_pair(want, mns, counts, verdict, w, r):
    assert tuple(int(v) for v in mns) == (want["m"], want["n"], want["step"])
    assert np.array_equal(counts, want["counts"])
    assert int(verdict) == want["verdict"]
    assert np.array_equal(u32(w), u32(want["w"])) and np.array_equal(u32(r), u32(want["r"]))


def check_rect(want, rect, status, uv):
    st, rc, wuv = want
    assert int(status) == st
    assert np.array_equal(rect, rc if st == Y.RECT_OK else np.full(4, -1, np.int32))      # untouched unless written
    assert np.array_equal(u32(uv), u32(wuv))


def test_abi_has_the_entries():
    from eao_fusion_amd import _lib
    L = _lib.load()
    for name in ("eao_object_np_counts_batch", "eao_object_np_association_batch", "eao_object_project_rects_batch", "eao_object_assoc_set_profiling",
                 "eao_object_assoc_last_kernel_ms"):
        assert hasattr(L, name) and name in _lib.SYMBOLS
    assert L.eao_abi_version() == 6
    assert OA_UNDEFINED() == Y.UNDEFINED


def OA_UNDEFINED():
    from eao_fusion_amd import object_association
    return object_association.UNDEFINED


@pytest.mark.parametrize("name", sorted(NP_SCENES))
def test_rank_sum_scene(OA, name):
    s = NP_SCENES[name]
    mns, counts = OA.np_counts([s["det"]], [s["map"]], [(0, 0)], [s["S"]])
    verdict, w, r = OA.np_association([s["det"]], [s["map"]], [(0, 0)], [s["S"]])
    check_pair(want_np(name), mns[0], counts[0], verdict[0], w[0], r[0])
    assert OA.no_para_data_association(s["det"], s["map"], s["S"]) == want_np(name)["verdict"]


@pytest.mark.parametrize("name", sorted(RECT_SCENES))
def test_rect_scene(OA, name):
    s = RECT_SCENES[name]
    rect, status, uv = OA.project_rects([s["points"]], s["Tcw"], *[s[k] for k in CAM], want_uv=True)
    check_rect(want_rect(name), rect[0], status[0], uv[0])
    rect2, status2 = OA.project_rects([s["points"]], s["Tcw"], *[s[k] for k in CAM])      # without uv: the same box
    assert np.array_equal(rect, rect2) and np.array_equal(status, status2)


def test_golden_files(OA):
    z = np.load(os.path.join(GOLD, "np.npz"))
    names = sorted(NP_SCENES)
    dets, maps = [NP_SCENES[n]["det"] for n in names], [NP_SCENES[n]["map"] for n in names]
    pairs = [(i, i) for i in range(len(names))]
    total = [NP_SCENES[n]["S"] for n in names]
    mns, counts = OA.np_counts(dets, maps, pairs, total)
    verdict, w, r = OA.np_association(dets, maps, pairs, total)
    for i, n in enumerate(names):
        assert np.array_equal(mns[i], z[n + ".mns"]) and np.array_equal(counts[i], z[n + ".counts"]) and int(verdict[i]) == int(z[n + ".verdict"]), n
        assert np.array_equal(u32(w[i]), u32(z[n + ".w"])) and np.array_equal(u32(r[i]), u32(z[n + ".r"])), n
    z = np.load(os.path.join(GOLD, "rect.npz"))
    for n, s in RECT_SCENES.items():
        rect, status, uv = OA.project_rects([s["points"]], s["Tcw"], *[s[k] for k in CAM], want_uv=True)
        assert int(status[0]) == int(z[n + ".status"]) and np.array_equal(u32(uv[0]), u32(z[n + ".uv"])), n
        if status[0] == Y.RECT_OK:
            assert np.array_equal(rect[0], z[n + ".rect"]), n


def test_batches_equal_single_calls(OA):
    """all scenes in one call -- the early returns, the undefined pair and the device pairs mixed --, pairs repeated, and the empty pair list"""
    names = sorted(NP_SCENES)
    dets, maps, total = [NP_SCENES[n]["det"] for n in names], [NP_SCENES[n]["map"] for n in names], [NP_SCENES[n]["S"] for n in names]
    k = names.index("same_distribution")
    pairs = [(i, i) for i in range(len(names))] + [(k, k), (k, k), (names.index("shifted_x"), k)]
    mns, counts = OA.np_counts(dets, maps, pairs, total)
    verdict, w, r = OA.np_association(dets, maps, pairs, total)
    for i, n in enumerate(names):
        check_pair(want_np(n), mns[i], counts[i], verdict[i], w[i], r[i])
    for p in (len(names), len(names) + 1):      # the repeated pair
        check_pair(want_np("same_distribution"), mns[p], counts[p], verdict[p], w[p], r[p])
    check_pair(want_np("shifted_x"), mns[-1], counts[-1], verdict[-1], w[-1], r[-1])      # (its map object is same_distribution's)
    mns, counts = OA.np_counts(dets, maps, [], total)
    assert mns.shape == (0, 3) and counts.shape == (0, 9)
    assert OA.np_association([], [], [])[0].shape == (0,)
    # the rects: every scene under its own pose singly (above); here several objects under ONE pose, objects without points among them
    s = RECT_SCENES["all_four_clamps"]
    cam = [s[k] for k in CAM]
    objs = [RECT_SCENES[n]["points"] for n in ("in_view", "no_points", "z0_nan", "points_129", "no_points", "one_point", "width_minus_infinity")]
    rect, status, uv = OA.project_rects(objs, s["Tcw"], *cam, want_uv=True)
    for j, pts in enumerate(objs):
        check_rect(Y.rect_literal(pts, s["Tcw"], **dict(zip(CAM, cam))), rect[j], status[j], uv[j])
    rect, status = OA.project_rects([], s["Tcw"], *cam)
    assert rect.shape == (0, 4) and status.shape == (0,)


def test_mixed_batch_of_64_by_64(OA):
    """64 detections against 64 map objects with bad points, ties and every early return, against the sort-free form"""
    rs = np.random.RandomState(2024)
    dets, maps, total = [], [], []
    for i in range(64):
        m = int(rs.choice([12, 19, 20, 21, 40, 64, 150, 300]))
        q = float(rs.choice([0.0, 0.05]))
        d = rs.normal(0.1 * (i % 3), 0.3, (m, 3))
        dets.append((np.round(d / q) * q if q else d).astype(np.float32))
        k = int(rs.choice([0, 19, 20, 60, 61, 200, 700, 1030]))
        p = rs.normal(0.0, 0.3, (k, 3))
        maps.append((np.round(p / 0.05) * 0.05 if i % 2 else p).astype(np.float32))
        total.append(k + int(rs.randint(0, 2 * k + 1)))
    pairs = [(d, j) for d in range(64) for j in range(64)]
    mns, counts = OA.np_counts(dets, maps, pairs, total)
    verdict, w, r = OA.np_association(dets, maps, pairs, total)
    cols = [[np.sort(mp[:, a]) for a in range(3)] for mp in maps]
    seen = set()
    for p, (d, j) in enumerate(pairs):
        v, n, step = Y.plan(len(dets[d]), len(maps[j]), total[j])
        assert tuple(int(x) for x in mns[p]) == (len(dets[d]), n, step)
        if v is not None:
            assert int(verdict[p]) == v and not counts[p].any() and not w[p].any() and not r[p].any()
            seen.add(v)
            continue
        c = np.zeros(9, np.int64)
        for a in range(3):
            lb, ub = np.searchsorted(cols[j][a], dets[d][:, a], "left"), np.searchsorted(cols[j][a], dets[d][:, a], "right")
            kl, ku = -(-lb // step), -(-ub // step)
            c[3 * a], c[3 * a + 1], c[3 * a + 2] = kl.sum(), (n - ku).sum(), (ku - kl).sum()
        assert np.array_equal(counts[p], c.astype(np.uint32)), (d, j)
        wv, ww, wr = Y.decide(len(dets[d]), n, c)
        assert int(verdict[p]) == wv and np.array_equal(u32(w[p]), u32(ww)) and np.array_equal(u32(r[p]), u32(wr)), (d, j)
        seen.add(wv)
    assert seen == {0, 1, 2}


def test_deterministic_across_calls_and_threads(OA):
    names = ["det_points_are_map_points_sampled", "ngood%d" % (2 * SC.TILE + 1), "m%d" % (SC.BLOCK * SC.OWNED + 1), "lattice"]
    dets, maps, total = [NP_SCENES[n]["det"] for n in names], [NP_SCENES[n]["map"] for n in names], [NP_SCENES[n]["S"] for n in names]
    pairs = [(i, j) for i in range(len(names)) for j in range(len(names))]
    rs = RECT_SCENES["all_four_clamps"]

    def run():
        mns, counts = OA.np_counts(dets, maps, pairs, total)
        verdict, w, r = OA.np_association(dets, maps, pairs, total)
        rect, status, uv = OA.project_rects([rs["points"], RECT_SCENES["points_129"]["points"]], rs["Tcw"], *[rs[k] for k in CAM], want_uv=True)
        return b"".join(np.ascontiguousarray(a).tobytes() for a in (mns, counts, verdict, w, r, rect, status, uv[0], uv[1]))

    first = run()
    results, errors = [None] * 4, []

    def worker(k):
        try:
            results[k] = [run() for _ in range(3)]
        except Exception as ex:      # noqa: BLE001
            errors.append(ex)

    threads = [threading.Thread(target=worker, args=(k,)) for k in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert run() == first and all(b == first for res in results for b in res)


def _raw_np(L, det_start, det_xyz, map_start, map_xyz, map_total, pair_det, pair_map, n_det=None, n_map=None, n_pair=None):
    """both rank-sum entries over planted outputs -> (status of each, whether every output still holds what was planted)"""
    from eao_fusion_amd import _lib
    arrs = [np.ascontiguousarray(det_start, np.int32), np.ascontiguousarray(det_xyz, np.float32), np.ascontiguousarray(map_start, np.int32),
            np.ascontiguousarray(map_xyz, np.float32), np.ascontiguousarray(map_total, np.int32), np.ascontiguousarray(pair_det, np.int32),
            np.ascontiguousarray(pair_map, np.int32)]
    ds, dx, ms, mx, mt, pd, pm = arrs
    n_det = len(ds) - 1 if n_det is None else n_det
    n_map = len(ms) - 1 if n_map is None else n_map
    n_pair = len(pd) if n_pair is None else n_pair
    P = max(len(pd), 1)
    mns, counts = np.full((P, 3), -7, np.int32), np.full((P, 9), 0xABCDABCD, np.uint32)
    verdict, w, r = np.full(P, -7, np.int32), np.full((P, 3), 123.5, np.float32), np.full((P, 2), 123.5, np.float32)
    a = (n_det, _lib.ptr(ds), _lib.ptr(dx), n_map, _lib.ptr(ms), _lib.ptr(mx), _lib.ptr(mt), n_pair, _lib.ptr(pd), _lib.ptr(pm))
    st1 = L.eao_object_np_counts_batch(*a, _lib.ptr(mns), _lib.ptr(counts))
    st2 = L.eao_object_np_association_batch(*a, _lib.ptr(verdict), _lib.ptr(w), _lib.ptr(r))
    untouched = bool((mns == -7).all() and (counts == 0xABCDABCD).all() and (verdict == -7).all() and (w == 123.5).all() and (r == 123.5).all())
    return st1, st2, untouched


def test_refusals_leave_the_outputs_untouched(OA):
    from eao_fusion_amd import _lib
    L = _lib.load()
    d, m = SC._gauss(25, 1), SC._gauss(60, 2)
    bad = (_lib.EAO_ERR_INVALID, _lib.EAO_ERR_INVALID, True)
    assert _raw_np(L, [0, 25], d, [0, 60], m, [60], [0], [0])[:2] == (0, 0)      # the call the refusals below spoil
    nan_d, nan_m = d.copy(), m.copy()
    nan_d[24, 2] = np.nan
    nan_m[0, 0] = np.nan
    assert _raw_np(L, [0, 25], nan_d, [0, 60], m, [60], [0], [0]) == bad                 # a NaN in a detection a pair reads
    assert _raw_np(L, [0, 25], d, [0, 60], nan_m, [60], [0], [0]) == bad                 # ... in a map object
    assert _raw_np(L, [25, 0], d, [0, 60], m, [60], [0], [0]) == bad                     # starts that do not ascend
    assert _raw_np(L, [0, 25], d, [0, 61, 60], np.r_[m, m], [61, 60], [0], [0]) == bad
    assert _raw_np(L, [-1, 25], d, [0, 60], m, [60], [0], [0]) == bad
    assert _raw_np(L, [0, 25], d, [0, 60], m, [59], [0], [0]) == bad                     # map_total below the good points
    assert _raw_np(L, [0, 25], d, [0, 60], m, [60], [1], [0]) == bad                     # a pair index out of range
    assert _raw_np(L, [0, 25], d, [0, 60], m, [60], [0], [-1]) == bad
    assert _raw_np(L, [0, 25], d, [0, 60], m, [60], [0], [1]) == bad
    assert _raw_np(L, [0, 25], d, [0, 60], m, [60], [0], [0], n_det=-1) == bad           # negative counts
    assert _raw_np(L, [0, 25], d, [0, 60], m, [60], [0], [0], n_map=-1) == bad
    assert _raw_np(L, [0, 25], d, [0, 60], m, [60], [0], [0], n_pair=-1) == bad
    # infinities are accepted; a NaN in a list no pair reads, or in a pair the early returns decide, is not read
    inf_d = d.copy()
    inf_d[3, 1] = np.inf
    assert _raw_np(L, [0, 25], inf_d, [0, 60], m, [60], [0], [0])[:2] == (0, 0)
    assert _raw_np(L, [0, 25, 50], np.r_[d, nan_d], [0, 60], m, [60], [0], [0])[:2] == (0, 0)
    assert int(OA.np_association([nan_d[6:]], [m], [(0, 0)])[0][0]) == 0                 # m = 19
    assert int(OA.np_association([d], [nan_m[:19]], [(0, 0)])[0][0]) == 2                # nGood = 19

    def raw_rects(start, n_map, cols, rows):
        ms = np.ascontiguousarray(start, np.int32)
        rect, status, uv = np.full((4, 4), -7, np.int32), np.full(4, 9, np.uint8), np.full((200, 2), 123.5, np.float32)
        T, xyz = np.eye(4, dtype=np.float32), np.ascontiguousarray(np.r_[m, m])
        st = L.eao_object_project_rects_batch(n_map, _lib.ptr(ms), _lib.ptr(xyz), _lib.ptr(T), 500.0, 500.0, 320.0, 240.0, cols, rows, _lib.ptr(rect),
                                              _lib.ptr(status), _lib.ptr(uv))
        return st, bool((rect == -7).all() and (status == 9).all() and (uv == 123.5).all())

    assert raw_rects([0, 60], 1, 640, 480)[0] == 0
    for args in (([60, 0], 1, 640, 480), ([0, 60, 30], 2, 640, 480), ([-1, 60], 1, 640, 480), ([0, 60], -1, 640, 480), ([0, 60], 1, -1, 480), ([0, 60], 1, 640, -1)):
        assert raw_rects(*args) == (_lib.EAO_ERR_INVALID, True), args


def test_profiling_reports_both_kernels(OA):
    OA.set_profiling(True)
    try:
        s, rs = NP_SCENES["same_distribution"], RECT_SCENES["in_view"]
        OA.np_association([s["det"]], [s["map"]], [(0, 0)])
        OA.project_rects([rs["points"]], rs["Tcw"], *[rs[k] for k in CAM])
        ms = OA.last_kernel_ms()
        assert len(ms) == 2 and all(0.0 < v < 1000.0 for v in ms)
    finally:
        OA.set_profiling(False)


def test_adapter_over_stand_in_objects_into_the_forest(OA, tmp_path):
    """include/eaofusion/ObjectAssociation.h over the stand-ins of tests/cpp/object_association, linked against the library itself: step 10.1's boxes, one
    detection against the map objects of its class, and the associated objects on into eao_object_iforest_outliers_batch, each against its yardstick"""
    import isolation_forest_reference as YF
    import test_object_association_class_cpu as T
    from eao_fusion_amd import isolation_forest as IF
    exe = str(tmp_path / "object_association_gpu")
    lib_dir = os.path.join(ROOT, "eao_fusion_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wno-sign-compare", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "object_association", "object_association_driver.cpp"), "-L", lib_dir, "-leaofusion_hip",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-pthread", "-o", exe])
    base = NP_SCENES["same_distribution"]
    d = base["det"]
    flags = np.zeros(len(d), int)
    flags[[0, 17]] = [1, 2]
    good_d = d[flags == 0]
    mflags = np.zeros(len(base["map"]), int)
    mflags[::50] = 1
    objs = [(7, NP_SCENES["shifted_x"]["map"] + np.float32(0.3), None, 0), (8, base["map"], None, 0), (7, base["map"], mflags, 0), (7, base["map"][:90], None, 0),
            (7, base["map"], None, 1), (7, base["map"][:15], None, 0)]
    body = " ".join(T.mapobj(c, p, f, erase=e, last_add=95) for c, p, f, e in objs)
    got = T.run_driver(exe, "cands %s %d %s\n" % (T.det(7, d, flags), len(objs), body))
    want = []
    for i in range(len(objs) - 1, -1, -1):
        c, p, f, e = objs[i]
        if c != 7 or e:
            continue
        g = p if f is None else p[f == 0]
        if Y.np_literal(good_d, g, len(p))["verdict"] == 1:
            want.append(i)
    assert want and len(want) < 4
    assert got == ["ret %d" % len(want), "ids 777 " + " ".join(str(i) for i in want)]
    for i in (0, 2, 3, 5):      # the single form, pair by pair
        c, p, f, e = objs[i]
        g = p if f is None else p[f == 0]
        assert T.run_driver(exe, "single %s %s\n" % (T.det(7, d, flags), T.mapobj(c, p, f))) == ["ret %d" % Y.np_literal(good_d, g, len(p))["verdict"]]
    # step 10.1 over the same objects under a pose
    rs = RECT_SCENES["in_view"]
    cam = {k: rs[k] for k in CAM}
    got = T.run_driver(exe, "rects %s %d %d %d %s\n" % (T.frame(100, (rs["fx"], rs["fy"], rs["cx"], rs["cy"]), rs["Tcw"]), rs["cols"], rs["rows"], len(objs), body))
    lines, written = [], 0
    for c, p, f, e in objs:
        st, rect, _ = Y.rect_literal(p, rs["Tcw"], **cam)
        if e or st != Y.RECT_OK:
            lines.append(T.PLANTED)
        else:
            lines.append("rect %d %d %d %d" % tuple(int(v) for v in rect))
            written += 1
    assert got == ["ret %d" % written] + lines and written >= 4
    # the associated objects go on to the forest (the call sites of IsolationForestDeleteOutliers follow the association upstream)
    chosen = [objs[i][1] for i in want]
    out = IF.outliers_batch(chosen, [7] * len(chosen), want_scores=True)
    for p, o in zip(chosen, out):
        _, scores, _ = YF.forest(p, YF.TREE_COUNT, YF.SEED, len(p) // 2)
        assert np.array_equal(o["flags"], YF.outlier_flags(scores, 7))
