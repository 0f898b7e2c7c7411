"""The update of a map object's point list on the device (eao_object_points_update_batch, eao_object_points_update; csrc/object_points.hip) against the yardstick
(tests/object_points_reference.py), its recorded results (tests/golden/object_points/results.npz) and the host header's literal walk
(tools/object_points_walk.cpp).  There is no tolerance anywhere: gates, targets, counts, list positions and statuses are integers and every float is compared as
a bit pattern (a NaN by isnan: its sign and payload are nobody's contract)."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import object_cuboid_reference as YC
import object_points_reference as Y
import object_points_scenes as SC
import test_object_points_abi_cpu as ABI

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden_object_points as GG  # noqa: E402

SCENES = SC.scenes()
NAMES = sorted(SCENES)
OK, INVALID = 0, -1


@pytest.fixture(scope="module")
def OP():
    from eao_fusion_amd import object_points
    return object_points


@pytest.fixture(scope="module")
def gold():
    return np.load(GG.PATH)


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("object_points") / "object_points_walk")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", os.path.join(ROOT, "tools", "object_points_walk.cpp"), "-o", exe])
    return exe


def walked(walk, descs):
    out = subprocess.run([walk], input="".join(Y.walk_script(d) for d in descs), capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.strip().split("\n")
    assert len(lines) == len(descs)
    return [line.split() for line in lines]


def raw_bytes(outs):
    return [{k: (None if a is None else a.tobytes()) for k, a in o.items()} for o in outs]


@pytest.fixture(scope="module")
def batch_of_scenes(OP):
    """every scene in one call"""
    return OP.update_batch([SCENES[n] for n in NAMES])


@pytest.mark.parametrize("name", NAMES)
def test_scene(OP, gold, batch_of_scenes, name):
    """every output, through the single entry and inside the batch of all scenes, against the recorded results"""
    want, _variant = GG.unpack(gold, name)
    got = OP.update(SCENES[name])
    assert Y.differences(got, want) == []
    assert Y.differences(batch_of_scenes[NAMES.index(name)], want) == []


def test_device_equals_the_host_header(walk, batch_of_scenes):
    """every scene through the literal walk of csrc/object_points_internal.h (one run of the program)"""
    for n, line, got in zip(NAMES, walked(walk, [SCENES[n] for n in NAMES]), batch_of_scenes):
        assert line == Y.walk_line(got).split(), n


def test_mixed_batch_of_64_equals_single_calls(OP, walk):
    """every combination of the stages in one call against one call per desc, byte for byte, and against the host walk"""
    descs = SC.mixed_batch(64)
    assert {(d["change_gate"], d["gate"], d["erase"]) for d in descs} == {(c, g, e) for c in (0, 1) for g in (0, 1, 2) for e in (0, 1, 2, 3)}
    st, outs = OP.update_raw(descs, fill=0xAB)
    assert st == OK
    statuses = set()
    for d, o, b, line in zip(descs, outs, raw_bytes(outs), walked(walk, descs)):
        st1, o1 = OP.update_raw([d], single=True, fill=0xAB)
        assert st1 == OK and raw_bytes(o1)[0] == b
        assert line == Y.walk_line(OP.trim(d, o)).split()
        statuses.add(int(o["rec"][0]["status"]))
    assert statuses == {Y.DONE, Y.REJECTED}
    assert OP.update_raw([], fill=0xAB)[0] == OK


def test_two_calls_return_the_same_bytes(OP):
    descs = [SCENES[n] for n in ("frame_M2055_C515", "merge_cuboid_500_300", "counts_8_and_9", "zero_signs_are_equal")]
    first = raw_bytes(OP.update_raw(descs)[1])
    for _ in range(3):
        assert raw_bytes(OP.update_raw(descs)[1]) == first


def test_four_host_threads(OP):
    descs = [SCENES[n] for n in ("frame_M1025_C3", "frame_M964_C65", "appended_1025", "nothing_at_all")]
    first = raw_bytes(OP.update_raw(descs)[1])
    out, errs = [None] * 4, []

    def work(i):
        try:
            out[i] = [raw_bytes(OP.update_raw(descs)[1]) for _ in range(3)]
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs and all(o is not None and all(b == first for b in o) for o in out)


def test_the_split_threshold(OP, walk):
    """n_cand * (n_map + n_cand) at 2^22 runs as one launch, above it as two: the same outputs, held to the host walk"""
    rng = np.random.default_rng(99)
    at = SC.frame_update(rng, 3072, 1024, repeats=400)
    above = SC.frame_update(rng, 3073, 1024, repeats=400)
    lines = walked(walk, [at, above])
    OP.set_profiling(True)
    try:
        for d, line, split in ((at, lines[0], False), (above, lines[1], True)):
            got = OP.update(d)
            match_ms, finish_ms = OP.last_kernel_ms()
            assert (match_ms >= 0) == split and finish_ms >= 0
            assert line == Y.walk_line(got).split()
            assert got["rec"]["status"] == Y.DONE and got["rec"]["n_appended"] > 0 and (got["target"] >= 0).sum() >= 300
    finally:
        OP.set_profiling(False)


def test_a_desc_of_2_16_list_points_and_2_12_candidates(OP, walk):
    """the compare spread over 16 workgroups, the ordered parts behind it in a second launch; beside it in the same call a small desc"""
    big, small = SC.large(), SCENES["frame_M65_C3"]
    got = OP.update_batch([big, small])
    lines = walked(walk, [big, small])
    assert lines[0] == Y.walk_line(got[0]).split() and lines[1] == Y.walk_line(got[1]).split()
    r = got[0]["rec"]
    assert r["status"] == Y.DONE and r["n_appended"] > 1000 and r["n_erased"] > 1000 and (got[0]["target"] >= (1 << 16)).any()


REFUSALS = ABI.refusals()


@pytest.mark.parametrize("k", range(len(REFUSALS)))
def test_refusal_leaves_the_outputs_untouched(OP, k):
    descs, kw = REFUSALS[k]
    st, outs = OP.update_raw(descs, fill=0xAB, **kw)
    assert st == INVALID and ABI.untouched(outs)
    good = SCENES["append_then_box"]      # and the thread's next call is served
    assert Y.differences(OP.update(good), Y.device(good)) == []


def test_survivors_feed_the_cuboid_entry(OP):
    """the surviving positions as the call wrote them are the `points` of eao_object_cuboids_batch: its record is the yardstick's cuboid of the yardstick's list"""
    from eao_fusion_amd import object_cuboid
    rng = np.random.default_rng(3)
    d = SCENES["frame_M2055_C515"]
    st, outs = OP.update_raw([d])
    assert st == OK
    n = int(outs[0]["rec"][0]["n_survivors"])
    want = Y.device(d)
    assert n == len(want["points"]) > 100
    centroids = SC.cloud(rng, 6, spread=(0.05, 0.05, 0.05))
    obj = dict(points=outs[0]["points"][:3 * n], centroids=centroids, Ryaw=YC.ryaw(0, 0, 0.4), prev_cuboid_center=np.array([0.5, -0.3, 2.0]))
    got = object_cuboid.object_cuboids(obj)
    assert YC.same_records(got, YC.device(dict(obj, points=want["points"])))


# ---- the adapter (include/eaofusion/ObjectMap.h) over stand-in Object_Map / MapPoint / Object_2D / Frame, linked with the library itself
@pytest.fixture(scope="module")
def adapter(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("object_points_adapter") / "object_points_driver")
    lib = os.path.join(ROOT, "eao_fusion_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-DEAOFUSION_FORCE_CV_COMPAT", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "object_points", "object_points_driver.cpp"), "-o", exe, "-pthread", "-L", lib, "-leaofusion_hip",
                           "-Wl,-rpath," + lib])
    return exe


def test_adapter_on_the_device(OP, adapter):
    """DataAssociateUpdate over stand-in objects, on through the cuboid and the forest, equals `points entry, host writes, cuboid entry, forest entry, host erase`
    done by hand"""
    import test_object_points_class_cpu as CL
    from eao_fusion_amd import isolation_forest as IFO
    from eao_fusion_amd import object_cuboid
    rng = np.random.default_rng(808)
    M, C, frames, rmax, cls = 150, 60, 7, CL.RMAX, CL.CLS
    mp, cp = SC.cloud(rng, M, CL.CENTER, (0.3, 0.3, 0.3)), SC.cloud(rng, C, CL.CENTER, (0.3, 0.3, 0.3))
    cp[5:25] = mp[40:60]      # seen again: equal positions, other MapPoints
    cp[50] = cp[30]           # and a candidate twice
    cp[55:] += 3.0            # beyond the radius
    mc, cc = rng.integers(-1, 12, M), rng.integers(-1, 10, C)
    lst = [CL.point(1 + i, mp[i], int(mc[i]), i % 2, 100 + i) for i in range(M)]
    cand = [CL.point(1000 + j, cp[j], int(cc[j]), (j + 1) % 2, 5000 + j) for j in range(C)]
    box = (400, 130, 110, 110)
    out = subprocess.run([adapter], input=CL.dau_text(1, 1, 1, box, 7, lst, cand, frames=frames), capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = out.stdout.strip().split("\n")
    # by hand
    s = np.zeros(3, np.float32)
    for p in mp:
        s = (s + p).astype(np.float32)
    d = dict(map_points=mp, cand_points=cp, map_count=np.maximum(mc, 0), cand_count=np.maximum(cc, 0), Tcw=CL.TCW, fx=500, fy=501, cx=320, cy=240, cols=640, rows=480,
             gate=Y.GATE_RADIUS, erase=Y.ERASE_PROJECTION, box_off_edge=1, box_rect=box, center=CL.CENTER, rmax=rmax, n_frames_after_push=frames + 1, sum_pos=s)
    res = OP.update(d)
    assert Y.differences(res, Y.device(d)) == []
    r = res["rec"]
    assert 0 < r["n_gated"] < C and r["n_appended"] > 5 and r["n_erased"] > 5 and r["n_survivors"] >= 30 and (res["target"] >= M).any()
    ids = [lst[i]["id"] if src == 0 else cand[i]["id"] for src, i in res["survivors"]]
    cub = object_cuboid.object_cuboids(dict(points=res["points"], centroids=np.zeros((frames + 1, 3), np.float32), Ryaw=YC.ryaw_libm(0, 0, 0), prev_cuboid_center=np.zeros(3)))
    flags = IFO.outliers_batch([res["points"]], [cls])[0]["flags"]
    total = cub["sum_pos"].copy()
    for p in res["points"][flags == 1]:
        total = (total - p).astype(np.float32)
    assert lines[0] == "step2" and lines[1] == "ret 1"
    assert lines[2] == ("list " + " ".join(str(i) for i, f in zip(ids, flags) if not f)).rstrip()
    assert lines[3] == "new " + " ".join(str(cand[i]["id"]) for src, i in res["list"][M:])
    assert lines[4] == "sum " + CL.hx(total)
    # the host writes: the gated-in candidates, and the features through target[j] in candidate order
    pts = {p["id"]: dict(p) for p in lst + cand}
    final = [lst[i]["id"] if src == 0 else cand[i]["id"] for src, i in res["list"]]
    for j, c in enumerate(cand):
        if res["gate"][j]:
            pts[c["id"]].update(object_id=CL.OID, object_class=cls, count=int(res["count"][j]))
            if res["target"][j] >= 0:
                pts[final[res["target"][j]]].update(have=c["have"], feature=c["feature"])
    assert lines[5:] == CL.state_lines(1, [], [], total, list(pts.values()), CL.OID)[4:]
