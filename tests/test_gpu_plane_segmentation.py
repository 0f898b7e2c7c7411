"""Frame::ComputePlanesFromPEAC on the device (eao_plane_seg_*; csrc/plane_seg.hip, csrc/plane_seg_internal.h) against the yardstick
tests/plane_segmentation_reference.py on the scenes of tests/plane_segmentation_scenes.py.  Every comparison is exact: integers with array_equal, doubles and
floats as their 64- and 32-bit patterns.  There is no tolerance anywhere in this file.  The expected values are the golden files, which
tests/test_plane_segmentation_reference_cpu.py holds to the yardstick; the replay tests run the yardstick itself on the device's own block records."""
import os
import threading

import numpy as np
import pytest
import torch  # noqa: F401  (before the library loads, so that both resolve the same HIP runtime)

import plane_segmentation_reference as R
import plane_segmentation_scenes as SC
import plane_segmentation_walk as WALK

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "plane_segmentation")
SCENES = SC.scenes()
NAMES = list(SCENES)
TABLE = ("normal", "center", "mse", "curvature", "N", "rid", "coef", "kept", "n_pixels", "cloud_count")
_cache = {}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else (a.view(np.uint32) if a.dtype == np.float32 else a)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def golden(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return {k: z[k] for k in z.files}


def segmenter(name):
    from eao_fusion_amd.plane_seg import PlaneSegmenter, cfg_from
    return PlaneSegmenter(cfg_from(SCENES[name]["cfg"]))


def read_back(ps):
    """everything a handle holds after a run, in the layout of R.result_arrays"""
    P = ps.planes()
    clouds = [ps.cloud(k) for k in range(len(P))]
    mid = ps.middle()
    return dict(
        records=ps.blocks(), membership=ps.membership(), blk_map=mid["blk_map"], plidmap=mid["plidmap"], claims=mid["claims"],
        normal=np.array([p["normal"] for p in P], np.float64).reshape(-1, 3), center=np.array([p["center"] for p in P], np.float64).reshape(-1, 3),
        mse=np.array([p["mse"] for p in P], np.float64), curvature=np.array([p["curvature"] for p in P], np.float64),
        N=np.array([p["N"] for p in P], np.int32), rid=np.array([p["rid"] for p in P], np.int32), coef=np.array([p["coef"] for p in P], np.float32).reshape(-1, 4),
        kept=np.array([p["kept"] for p in P], np.uint8), n_pixels=np.array([p["n_pixels"] for p in P], np.int32),
        cloud_count=np.array([p["cloud_count"] for p in P], np.int32), clouds=np.concatenate(clouds + [np.zeros((0, 3), np.float32)]).astype(np.float32),
        cloud_offset=np.array([p["cloud_offset"] for p in P], np.int32))


def device(name):
    """one run per scene for the whole module; nothing changes what it returns"""
    if name not in _cache:
        _cache[name] = read_back(segmenter(name).run(SCENES[name]["depth"]))
    return _cache[name]


def agrees(got, want, keys):
    """the keys on which got and the golden file differ; a golden file that holds a digest of an array is compared by digest"""
    bad = []
    for k in keys:
        if k in want:
            ok = same(got[k], want[k])
        else:
            ok = np.array_equal(R.digest(got[k]), want["sha256_" + k])
        if not ok:
            bad.append(k)
    return bad


@pytest.mark.parametrize("name", NAMES)
def test_block_records(name):
    got, want = device(name)["records"], golden(name)
    c = SCENES[name]["cfg"]
    assert got.shape == ((c.height // c.window) * (c.width // c.window), 18)
    assert agrees(dict(records=got), want, ["records"]) == []
    flags = got[:, 0:1].copy().view(np.int32)[:, 0]
    claims = SCENES[name]["claims"]
    if "missing_blocks" in claims:
        assert np.flatnonzero(flags & 1).tolist() == claims["missing_blocks"]
    if "discontinuity_blocks" in claims:
        assert np.flatnonzero(flags & 2).tolist() == claims["discontinuity_blocks"]


@pytest.mark.parametrize("name", ["room_vga", "room_small", "table"])
def test_device_fit_is_the_host_build_of_the_same_function(name):
    rec = device(name)["records"]
    head = rec[:, 0:1].copy().view(np.int32)
    keep = np.flatnonzero(head[:, 0] == 0)
    assert len(keep) > 0
    lines = "".join("%d %s\n" % (head[b, 1], " ".join("%016x" % v for v in rec[b, 1:10].view(np.uint64))) for b in keep)
    out = WALK.run(WALK.build(False), "fit", lines).split("\n")
    for b, line in zip(keep, out):
        assert [int(w, 16) for w in line.split()] == rec[b, 10:18].view(np.uint64).tolist(), "block %d" % b


@pytest.mark.parametrize("name", NAMES)
def test_outputs(name):
    got, want = device(name), golden(name)
    assert agrees(got, want, TABLE + ("blk_map", "plidmap", "claims", "membership", "clouds")) == []
    off = np.concatenate([[0], np.cumsum(got["cloud_count"])[:-1]]).astype(np.int32) if len(got["cloud_count"]) else np.zeros(0, np.int32)
    assert np.array_equal(got["cloud_offset"], off)
    claims = SCENES[name]["claims"]
    if "n_planes" in claims:
        assert len(got["kept"]) == claims["n_planes"]
    if "n_kept" in claims:
        assert int(got["kept"].sum()) == claims["n_kept"]
    if "n_voxels" in claims:
        assert got["cloud_count"].tolist() == [claims["n_voxels"]]
    for k in range(len(got["kept"])):
        assert int((got["membership"] == k).sum()) == int(got["n_pixels"][k])


@pytest.mark.parametrize("name", SC.SMALL)
def test_replay_of_the_devices_own_records(name):
    s, got = SCENES[name], device(name)
    r = R.result_arrays(R.run(s["cfg"], s["depth"], records=R.records_from_array(got["records"])))
    bad = [k for k in TABLE + ("blk_map", "plidmap", "claims", "membership", "clouds") if not same(got[k], r[k])]
    assert bad == []


def test_two_runs_and_two_handles_return_the_same_bytes():
    for name in ("room_small", "room_vga"):
        a = segmenter(name)
        first = read_back(a.run(SCENES[name]["depth"]))
        second = read_back(a.run(SCENES[name]["depth"]))
        other = read_back(segmenter(name).run(SCENES[name]["depth"]))
        for k in first:
            assert first[k].tobytes() == second[k].tobytes() == other[k].tobytes() == device(name)[k].tobytes(), (name, k)


def test_a_strided_image_is_the_packed_image():
    name = "ragged_65x45"
    d = SCENES[name]["depth"]
    wide = np.full((d.shape[0], d.shape[1] + 7), np.nan, np.float32)
    wide[:, :d.shape[1]] = d
    got = read_back(segmenter(name).run(wide[:, :d.shape[1]]))
    assert all(got[k].tobytes() == device(name)[k].tobytes() for k in got)


def _in_threads(jobs):
    out, err = [None] * len(jobs), []

    def work(i):
        try:
            out[i] = jobs[i]()
        except Exception as e:      # noqa: BLE001
            err.append(e)
    th = [threading.Thread(target=work, args=(i,)) for i in range(len(jobs))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert err == []
    return out


def test_four_threads_on_one_handle_and_on_four():
    name = "table"
    want = device(name)
    one = segmenter(name)
    lock = threading.Lock()

    def shared():
        with lock:      # a handle holds ONE frame's results: run and read-back are one step of the caller's
            return read_back(one.run(SCENES[name]["depth"]))
    for got in _in_threads([shared] * 4):
        assert all(got[k].tobytes() == want[k].tobytes() for k in want)
    # without the caller's lock the runs still serialise on the handle's mutex: whichever came last, the results are this frame's
    _in_threads([lambda: one.run(SCENES[name]["depth"])] * 4)
    got = read_back(one)
    assert all(got[k].tobytes() == want[k].tobytes() for k in want)
    hs = [segmenter(name) for _ in range(4)]
    for got in _in_threads([(lambda h=h: read_back(h.run(SCENES[name]["depth"]))) for h in hs]):
        assert all(got[k].tobytes() == want[k].tobytes() for k in want)


def test_nothing_stale_after_a_different_frame():
    # the same geometry (80 x 60, min_support 300): a frame of three first-round planes and many claims, then a frame with no plane, then one plane
    ps = segmenter("room_small")
    for name in ("room_small", "no_plane", "one_plane", "halo", "room_small"):
        assert SCENES[name]["cfg"].__dict__ == SCENES["room_small"]["cfg"].__dict__
        got = read_back(ps.run(SCENES[name]["depth"]))
        assert all(got[k].tobytes() == device(name)[k].tobytes() for k in got), name


def test_invalid_arguments():
    import ctypes as C
    from eao_fusion_amd import _lib
    from eao_fusion_amd.plane_seg import PlaneSegmenter, cfg_from, default_cfg
    L = _lib.load()
    c = SCENES["room_small"]["cfg"]
    for field, value in (("width", 0), ("height", -1), ("window", 1), ("window", 33), ("width", 5), ("fx", 0.0), ("fy", float("nan")), ("min_support", 0),
                         ("max_step", -1), ("depth_min", 0.0), ("depth_max", 0.1), ("depth_max", float("inf")), ("leaf", 0.0), ("depth_alpha", float("nan")),
                         ("z_far", 100.0)):
        bad = cfg_from(c)
        setattr(bad, field, value)
        h = C.c_void_p(0)
        assert L.eao_plane_seg_create(C.byref(bad), C.byref(h)) == _lib.EAO_ERR_INVALID and not h.value, field
    assert L.eao_plane_seg_create(None, None) == _lib.EAO_ERR_INVALID
    big = default_cfg(4096, 2048, 500, 500, 2048, 1024)
    h = C.c_void_p(0)
    assert L.eao_plane_seg_create(C.byref(big), C.byref(h)) == _lib.EAO_ERR_INVALID
    ps = PlaneSegmenter(cfg_from(c))
    n = C.c_int32(-7)
    # before any frame: every read-back refuses and writes nothing
    assert L.eao_plane_seg_planes(ps.h, 0, None, C.byref(n)) == _lib.EAO_ERR_INVALID and n.value == -7
    assert L.eao_plane_seg_info(ps.h, C.byref(n), None, None, None) == _lib.EAO_ERR_INVALID and n.value == -7
    d = SCENES["room_small"]["depth"]
    assert L.eao_plane_seg_run(ps.h, None, 80) == _lib.EAO_ERR_INVALID
    assert L.eao_plane_seg_run(None, d.ctypes.data, 80) == _lib.EAO_ERR_INVALID
    assert L.eao_plane_seg_run(ps.h, d.ctypes.data, 79) == _lib.EAO_ERR_INVALID
    assert L.eao_plane_seg_planes(ps.h, 0, None, C.byref(n)) == _lib.EAO_ERR_INVALID and n.value == -7      # (still no frame)
    want = device("room_small")
    ps.run(d)
    # a refused call afterwards leaves the frame's results as they are
    assert L.eao_plane_seg_run(ps.h, d.ctypes.data, 79) == _lib.EAO_ERR_INVALID
    xyz = np.full((4, 3), 7.0, np.float32)
    assert L.eao_plane_seg_cloud(ps.h, 0, 4, xyz.ctypes.data, C.byref(n)) == _lib.EAO_ERR_INVALID and n.value == -7 and (xyz == 7.0).all()
    assert L.eao_plane_seg_cloud(ps.h, 1, 0, None, C.byref(n)) == _lib.EAO_ERR_INVALID and n.value == -7
    assert L.eao_plane_seg_cloud(ps.h, -1, 0, None, C.byref(n)) == _lib.EAO_ERR_INVALID
    arr = (_lib.PlaneSegPlane * 1)()
    assert L.eao_plane_seg_planes(ps.h, 0, arr, C.byref(n)) == _lib.EAO_ERR_INVALID and n.value == -7
    assert L.eao_plane_seg_blocks(ps.h, 47, xyz.ctypes.data, C.byref(n)) == _lib.EAO_ERR_INVALID and (xyz == 7.0).all()
    assert L.eao_plane_seg_membership(ps.h, None) == _lib.EAO_ERR_INVALID
    got = read_back(ps)
    assert all(got[k].tobytes() == want[k].tobytes() for k in want)


def _pose(seed=7):
    rs = np.random.RandomState(seed)
    a = rs.uniform(-0.2, 0.2, 3)
    Rx = np.array([[1, 0, 0], [0, np.cos(a[0]), -np.sin(a[0])], [0, np.sin(a[0]), np.cos(a[0])]])
    Ry = np.array([[np.cos(a[1]), 0, np.sin(a[1])], [0, 1, 0], [-np.sin(a[1]), 0, np.cos(a[1])]])
    Rz = np.array([[np.cos(a[2]), -np.sin(a[2]), 0], [np.sin(a[2]), np.cos(a[2]), 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3] = Rx @ Ry @ Rz
    T[:3, 3] = rs.uniform(-0.5, 0.5, 3)
    return T.astype(np.float32)


@pytest.mark.parametrize("name,with_pose", [("room_vga", True), ("table", False)])
def test_add_from_seg_is_add_of_the_read_back_cloud(name, with_pose):
    from eao_fusion_amd import _lib
    from eao_fusion_amd.plane_map import PlaneMap
    ps = segmenter(name).run(SCENES[name]["depth"])
    planes = ps.planes()
    Tcw = _pose() if with_pose else None
    M = Tcw if with_pose else np.eye(4, dtype=np.float32)
    a, b = PlaneMap(), PlaneMap()
    kept = [k for k, p in enumerate(planes) if p["kept"]]
    assert len(kept) >= 1
    for k in kept:
        world = (M.T @ planes[k]["coef"]).astype(np.float32)      # Frame::ComputePlaneWorldCoeff, src/Frame.cc:373-379
        a.add_from_seg(10 + k, world, ps, k, Tcw)
        b.add(10 + k, world, ps.cloud(k), Tcw)
    assert a.info()["n_live"] == len(kept) and a.info()["n_points_in_use"] == b.info()["n_points_in_use"] == sum(planes[k]["cloud_count"] for k in kept)
    for k in kept:
        (xa, wa), (xb, wb) = a.boundary(10 + k), b.boundary(10 + k)
        assert xa.tobytes() == xb.tobytes() and wa.tobytes() == wb.tobytes() and len(xa) == planes[k]["cloud_count"]
    coef = np.array([planes[k]["coef"] for k in kept], np.float32)
    ra, rb = a.associate(M, coef, full=True), b.associate(M, coef, full=True)
    assert all(ra[k].tobytes() == rb[k].tobytes() for k in rb) and (ra["match"] >= 0).all()
    # a plane that was not kept has no cloud upstream; an index out of range; a handle that holds no frame: refused, the map as it was
    before = a.info()
    for k in [k for k, p in enumerate(planes) if not p["kept"]] + [-1, len(planes)]:
        with pytest.raises(_lib.EaoError) as e:
            a.add_from_seg(99, np.zeros(4, np.float32), ps, k, Tcw)
        assert e.value.status == _lib.EAO_ERR_INVALID
    with pytest.raises(_lib.EaoError):
        a.add_from_seg(99, np.zeros(4, np.float32), segmenter(name), 0, Tcw)
    with pytest.raises(_lib.EaoError):
        a.add_from_seg(10 + kept[0], np.zeros(4, np.float32), ps, kept[0], Tcw)      # (a live id)
    with pytest.raises(_lib.EaoError):
        a.update_boundary_from_seg(99, ps, kept[0], Tcw)                             # (an id that is not held)
    assert a.info() == before
    # UpdateBoundary from the handle: the same bytes as from the host pointer, compaction included
    for _ in range(3):
        a.update_boundary_from_seg(10 + kept[0], ps, kept[-1], Tcw)
        b.update_boundary(10 + kept[0], ps.cloud(kept[-1]), Tcw)
        assert a.info() == b.info()
    for k in kept:
        assert a.boundary(10 + k)[0].tobytes() == b.boundary(10 + k)[0].tobytes()


def test_the_chain_segmentation_map_association_pose_optimization():
    """the frame's kept planes become map planes from the handle, are associated, and enter eao_pose_optimization as its plane edges: equal to the same chain
    built from read-back clouds"""
    from eao_fusion_amd import synth
    from eao_fusion_amd.optimizer import Optimizer
    from eao_fusion_amd.plane_map import PlaneMap
    ps = segmenter("room_vga").run(SCENES["room_vga"]["depth"])
    planes = [p for p in ps.planes()]
    kept = [k for k, p in enumerate(planes) if p["kept"]]
    prob = synth.synth_pose(n=150, seed=4100, n_planes=len(kept))
    Tcw = np.ascontiguousarray(prob["Tcw"], np.float32).reshape(4, 4)
    coef = np.array([planes[k]["coef"] for k in kept], np.float32)
    worlds = [(Tcw.T @ c).astype(np.float32) for c in coef]
    a, b = PlaneMap(), PlaneMap()
    for i, k in enumerate(kept):
        a.add_from_seg(200 + i, worlds[i], ps, k, Tcw)
        b.add(200 + i, worlds[i], ps.cloud(k), Tcw)
    ma, mb = a.associate(Tcw, coef)["match"], b.associate(Tcw, coef)["match"]
    assert np.array_equal(ma, mb) and ma.tolist() == list(range(len(kept)))

    def problem(match):
        p = dict(prob)
        p["plane_world"] = np.array([worlds[j] for j in match], np.float32)
        p["plane_obs"] = coef
        p["plane_seen"] = np.ones(len(match), np.uint8)
        return p
    ra, rb = Optimizer.PoseOptimization(problem(ma)), Optimizer.PoseOptimization(problem(mb))
    assert ra["Tcw"].tobytes() == rb["Tcw"].tobytes() and np.array_equal(ra["outlier"], rb["outlier"]) and np.array_equal(ra["plane_outlier"], rb["plane_outlier"])
    assert ra["n_inliers"] > 100 and len(ra["plane_outlier"]) == len(kept)


def test_profiling_changes_no_byte_and_reports_four_stages():
    import ctypes as C
    from eao_fusion_amd import _lib
    name = "table"
    ps = segmenter(name)
    us = np.full(4, -1.0)
    ps.run(SCENES[name]["depth"])
    assert _lib.load().eao_plane_seg_last_timing(ps.h, us.ctypes.data) == _lib.EAO_ERR_INVALID and (us == -1.0).all()      # profiling was off
    ps.set_profiling(True)
    got = read_back(ps.run(SCENES[name]["depth"]))
    assert all(got[k].tobytes() == device(name)[k].tobytes() for k in got)
    t = ps.last_timing()
    assert t.shape == (4,) and (t > 0).all() and np.isfinite(t).all()
    ps.set_profiling(False)
    assert _lib.load().eao_plane_seg_last_timing(ps.h, us.ctypes.data) == _lib.EAO_ERR_INVALID
    assert _lib.load().eao_plane_seg_set_profiling(None, 1) == _lib.EAO_ERR_INVALID
