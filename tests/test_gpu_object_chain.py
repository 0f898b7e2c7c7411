"""The chained update of a map object on the device (eao_object_update_chain_batch, eao_object_update_chain; csrc/object_chain.hip) against the yardstick
(tests/object_chain_reference.py), the host walk (tools/object_chain_walk.cpp) and the three existing entries chained by hand in the same process.  There is no tolerance anywhere: gates, targets,
counts, list positions, flags and statuses are integers and every float is compared as a bit pattern (a NaN by isnan: its sign and payload are nobody's
contract)."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import object_chain_reference as Y
import object_chain_scenes as SC
import test_object_chain_abi_cpu as ABI

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden_object_chain as GG  # noqa: E402

SCENES = SC.scenes()
NAMES = sorted(SCENES)
OK, INVALID = 0, -1


@pytest.fixture(scope="module")
def CH():
    from eao_fusion_amd import object_chain
    return object_chain


@pytest.fixture(scope="module")
def yardstick():
    """the yardstick's result of every scene, computed once"""
    return {n: Y.chain(SCENES[n], "device") for n in NAMES}


@pytest.fixture(scope="module")
def batch_of_scenes(CH):
    """every scene in one call"""
    return CH.update_batch([SCENES[n] for n in NAMES])


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    """tools/object_chain_walk.cpp: the three HIP-free headers chained on the host"""
    exe = str(tmp_path_factory.mktemp("object_chain") / "object_chain_walk")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", os.path.join(ROOT, "tools", "object_chain_walk.cpp"), "-o", exe])
    return exe


def walked(walk, descs):
    """one run of the program over the descs: its lines, token by token"""
    out = subprocess.run([walk], input="".join(Y.walk_script(d) for d in descs), capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.strip().split("\n")
    assert len(lines) == len(descs)
    return [line.split() for line in lines]


def raw_bytes(outs):
    return [{k: (None if a is None else a.tobytes()) for k, a in o.items()} for o in outs]


def by_hand(desc):
    """the three existing entries, chained by the caller: eao_object_points_update (twice where an alias needs the gate first) -> the erase of the bad points ->
    eao_object_cuboids -> eao_object_iforest_outliers_batch.  The same keys as object_chain.trim gives."""
    from eao_fusion_amd import isolation_forest, object_cuboid, object_points
    res = object_points.update(desc)
    if res["rec"]["status"] != object_points.DONE:
        return res
    alias = desc.get("cand_alias")
    if alias is not None:      # the caller that needs the incremented count in stage 3 passes it in map_count
        count = np.array(object_points.lists_of(desc)[1], np.int32)
        for j in np.flatnonzero(res["gate"]):
            if alias[j] >= 0:
                count[alias[j]] += 1
        res = object_points.update(dict(desc, map_count=count))
    mb, cb = Y.bad_flags(desc)
    keep = np.array([not (cb[i] if s else mb[i]) for s, i in res["survivors"]], bool)
    final, pts = res["survivors"][keep], res["points"][keep]
    del res["points"]
    res["final"] = final
    res["cuboid"] = object_cuboid.object_cuboids(dict(points=pts, centroids=desc["centroids"], Ryaw=desc["Ryaw"], prev_cuboid_center=desc["prev_cuboid_center"]))
    f = isolation_forest.outliers_batch([pts], [desc["class_id"]], bool(desc["bi_forest"]), want_scores=True)[0]
    rec = np.zeros((), Y.RECORD_DTYPE)
    rec["n_final"], rec["removed"] = len(final), f["removed"]
    ran = Y.IF.object_runs(desc["bi_forest"], desc["class_id"], len(final))
    rec["forest_status"] = Y.FOREST_DONE if ran else Y.FOREST_SKIPPED      # (no scene's Build fails: a failure has no flags and scores of -1)
    assert not ran or (f["scores"] >= 0).all()
    res.update(forest_flags=f["flags"], scores=f["scores"], chain=rec)
    return res


def same_bytes(a, b):
    """two results of the same keys, every array byte for byte"""
    return set(a) == set(b) and all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)


@pytest.mark.parametrize("name", NAMES)
def test_scene(CH, yardstick, batch_of_scenes, name):
    """every output, through the single entry and inside the batch of all scenes, against the yardstick and its recorded results"""
    got = CH.update(SCENES[name])
    assert Y.differences(got, yardstick[name]) == []
    assert Y.differences(GG.recorded_part(got), GG.unpack(np.load(GG.PATH), name)) == []
    assert Y.differences(batch_of_scenes[NAMES.index(name)], yardstick[name]) == []


def test_device_equals_the_host_walk(CH, walk, batch_of_scenes):
    """every output of every scene against the host walk (one run of the program), as integers and bit patterns, through the batch and through the single entry"""
    for n, line, got in zip(NAMES, walked(walk, [SCENES[n] for n in NAMES]), batch_of_scenes):
        assert line == Y.walk_tokens(SCENES[n], got), n
        assert line == Y.walk_tokens(SCENES[n], CH.update(SCENES[n])), n


@pytest.mark.parametrize("name", NAMES)
def test_scene_equals_the_three_entries_chained_by_hand(CH, batch_of_scenes, name):
    want = by_hand(SCENES[name])
    got = batch_of_scenes[NAMES.index(name)]
    assert Y.differences(got, want) == []
    assert same_bytes(got, want)


def test_mixed_batch_of_32_equals_single_calls(CH, walk):
    """one call of 32 descs against one call per desc, byte for byte, and against the host walk"""
    descs = SC.mixed_batch(32)
    st, outs = CH.update_raw(descs, fill=0xAB)
    assert st == OK
    statuses = set()
    for d, o, b, line in zip(descs, outs, raw_bytes(outs), walked(walk, descs)):
        st1, o1 = CH.update_raw([d], single=True, fill=0xAB)
        assert st1 == OK and raw_bytes(o1)[0] == b
        assert line == Y.walk_tokens(d, CH.trim(d, o))
        statuses.add(int(o["rec"][0]["status"]))
    assert len(statuses) >= 2
    assert CH.update_raw([], fill=0xAB)[0] == OK


def test_two_calls_return_the_same_bytes(CH):
    descs = [SCENES[n] for n in ("frame_to_1024", "n_final_%d" % (SC.lds_edge() + 1), "alias_raises_8_to_9", "rejected", "n_final_31")]
    first = raw_bytes(CH.update_raw(descs)[1])
    for _ in range(3):
        assert raw_bytes(CH.update_raw(descs)[1]) == first


def test_four_host_threads(CH):
    descs = [SCENES[n] for n in ("n_final_1025", "class_62_threshold", "undefined", "n_final_30")]
    first = raw_bytes(CH.update_raw(descs)[1])
    out, errs = [None] * 4, []

    def work(i):
        try:
            out[i] = [raw_bytes(CH.update_raw(descs)[1]) for _ in range(3)]
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs and all(o is not None and all(b == first for b in o) for o in out)


def test_two_launch_side_of_the_split(CH, walk):
    """2048 x 2048: the match runs as its own launch"""
    d = SC.split_launch()
    CH.set_profiling(True)
    try:
        got = CH.update(d)
        ms = CH.last_kernel_ms()
    finally:
        CH.set_profiling(False)
    assert ms[0] >= 0 and all(v >= 0 for v in ms[1:])
    assert Y.differences(got, Y.chain(d, "device")) == []
    assert same_bytes(got, by_hand(d))
    assert walked(walk, [d])[0] == Y.walk_tokens(d, got)


def test_every_refusal_leaves_the_outputs_untouched(CH):
    for descs, kw in ABI.refusals():
        st, outs = CH.update_raw(descs, fill=0xAB, **kw)
        assert st == INVALID and ABI.untouched(outs), kw
    st, outs = CH.update_raw([SCENES["rejected"]], fill=0xAB)      # a status other than DONE: the points record and nothing else
    assert st == OK and int(outs[0]["rec"][0]["status"]) == Y.OP.REJECTED
    assert ABI.untouched([{k: v for k, v in outs[0].items() if k != "rec"}])


def test_profiling_slots(CH):
    CH.set_profiling(True)
    try:
        CH.update(SCENES["n_final_31"])
        fused = CH.last_kernel_ms()
        CH.update(SCENES["class_75_is_exempt"])
        skipped = CH.last_kernel_ms()
    finally:
        CH.set_profiling(False)
    assert fused[0] == -1 and all(v >= 0 for v in fused[1:])
    assert all(v >= 0 for v in skipped[1:4])


# ---- the adapter (include/eaofusion/ObjectMap.h) over stand-in Object_Map / MapPoint / Object_2D / Frame, linked with the library itself
@pytest.fixture(scope="module")
def adapter(tmp_path_factory):
    import subprocess
    exe = str(tmp_path_factory.mktemp("object_chain_adapter") / "object_chain_driver")
    lib = os.path.join(ROOT, "eao_fusion_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-DEAOFUSION_FORCE_CV_COMPAT", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "object_chain", "object_chain_driver.cpp"), "-o", exe, "-pthread", "-L", lib, "-leaofusion_hip",
                           "-Wl,-rpath," + lib])
    return exe


@pytest.mark.parametrize("flag", [1, 2])
def test_adapter_on_the_device(adapter, flag):
    """DataAssociateUpdateChained over stand-in objects against the existing DataAssociateUpdate on a copy of the same objects, member for member: the lists, the
    sums, the cuboid's members and every MapPoint field"""
    import subprocess
    import test_object_chain_class_cpu as CC
    import test_object_points_class_cpu as CL
    rng = np.random.default_rng(909)
    M, C = 150, 60
    mp, cp = SC.PS.cloud(rng, M, CL.CENTER, (0.3, 0.3, 0.3)), SC.PS.cloud(rng, C, CL.CENTER, (0.3, 0.3, 0.3))
    cp[5:25] = mp[40:60]      # seen again: equal positions, other MapPoints
    cp[55:] += 3.0            # beyond the radius
    mc, cc = rng.integers(-1, 12, M), rng.integers(-1, 10, C)
    mc[70:80] = 8             # the very MapPoints of candidates 30 .. 39: a count of 8 that step 3 raises to 9
    lst = [CL.point((1000 if i % 17 == 3 else 1) + i, mp[i], int(mc[i]), i % 2, 100 + i) for i in range(M)]      # (an id of 1000 or more is a bad point)
    cand = [CL.point((2000 if j % 13 == 6 else 500) + j, cp[j], int(cc[j]), (j + 1) % 2, 5000 + j) for j in range(C)]
    for j in range(30, 40):
        cand[j] = lst[40 + j]
    text = {verb: CC.script(verb, lst, cand, flag=flag, box=(400, 130, 110, 110), rect_x=395, cls=CL.CLS, det_cls=CL.CLS, frames=7) for verb in ("dau", "chained")}
    out = {}
    for verb in text:
        run = subprocess.run([adapter], input=text[verb], capture_output=True, text=True)
        assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
        out[verb] = run.stdout.strip().split("\n")
    assert out["dau"] == out["chained"]
    lines = out["chained"]
    if flag != 1:      # (behind the change gate the outcome is the scene's; both forms agree on it above)
        return
    assert lines[0] == "step2" and lines[1] == "ret 1"
    ids = [int(v) for v in lines[2].split()[1:]]
    assert len(ids) >= 30 and not any(i >= 1000 for i in ids) and len(lines[3].split()) > 5
