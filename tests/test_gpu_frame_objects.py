"""A frame's 2D objects on the device (eao_frame_objects_batch, eao_frame_objects; csrc/frame_objects.hip) against the yardstick
(tests/frame_objects_reference.py) and its recorded results (tests/golden/frame_objects/results.npz).  There is no tolerance anywhere: counts, lists, boxes and
flags are integers, and every float of every record is compared as a 32-bit pattern (a NaN by isnan: its payload is nobody's contract)."""
import ctypes as C
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import frame_objects_reference as Y
import frame_objects_scenes as SC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden_frame_objects as GG  # noqa: E402

SCENES = SC.scenes()
NAMES = sorted(SCENES)
_want = {}
OK, INVALID, CAPACITY = 0, -1, -3


@pytest.fixture(scope="module")
def FO():
    from eao_fusion_amd import frame_objects
    return frame_objects


def want(name):
    if name not in _want:
        _want[name] = Y.compact(SCENES[name][0])
    return _want[name]


def test_abi_has_the_entries(FO):
    from eao_fusion_amd import _lib
    L = _lib.load()
    for name in ("eao_frame_objects_batch", "eao_frame_objects", "eao_frame_objects_set_profiling", "eao_frame_objects_last_kernel_ms"):
        assert hasattr(L, name) and name in _lib.SYMBOLS
    assert FO.RECORD_DTYPE == Y.RECORD_DTYPE and (FO.MAX_KEYPOINTS, FO.MAX_BOXES) == (Y.MAX_KEYPOINTS, Y.MAX_BOXES)


@pytest.mark.parametrize("name", NAMES)
def test_scene(FO, name):
    """every field of every record and both lists, through the single entry"""
    got = FO.frame_objects(SCENES[name][0])
    assert Y.same(got, want(name))
    assert SCENES[name][1](got)


def test_golden_files(FO):
    z = np.load(os.path.join(ROOT, "tests", "golden", "frame_objects", "results.npz"))
    got = FO.frame_objects_batch([SCENES[n][0] for n in NAMES])
    for n, g in zip(NAMES, got):
        assert Y.same(g, GG.unpack(z, n)), n


def raw_bytes(raw):
    return tuple(np.ascontiguousarray(a).tobytes() for a in raw[1:])


def test_batch_equals_single_calls(FO):
    """every scene in one call -- an empty frame and a frame without boxes among them -- against one call per scene, byte for byte"""
    frames = [SCENES[n][0] for n in NAMES]
    st, rec, sa, la, sk, lk = FO.frame_objects_raw(frames)
    assert st == OK
    b = 0
    for fr in frames:
        s1, r1, a1, l1, k1, m1 = FO.frame_objects_raw([fr], single=True)
        m = len(r1)
        assert s1 == OK and rec[b:b + m].tobytes() == r1.tobytes()
        assert np.array_equal(sa[b:b + m + 1] - sa[b], a1) and np.array_equal(sk[b:b + m + 1] - sk[b], k1)
        assert la[sa[b]:sa[b + m]].tobytes() == l1[:a1[m]].tobytes() and lk[sk[b]:sk[b + m]].tobytes() == m1[:k1[m]].tobytes()
        b += m
    assert b == len(rec)


def test_mixed_batch_and_empty_batches(FO):
    mixed = [SCENES[n][0] for n in ("frame_without_keypoints", "timing_shape", "frame_without_boxes", "box_without_points", "frame_without_boxes")]
    got = FO.frame_objects_batch(mixed)
    for g, n in zip(got, ("frame_without_keypoints", "timing_shape", "frame_without_boxes", "box_without_points", "frame_without_boxes")):
        assert Y.same(g, want(n)), n
    st, rec, sa, la, sk, lk = FO.frame_objects_raw([], fill=0xAB)
    assert st == OK and sa.tolist() == [0] and sk.tolist() == [0]
    st, rec, sa, la, sk, lk = FO.frame_objects_raw([SCENES["frame_without_boxes"][0]] * 2, fill=0xAB)
    assert st == OK and sa.tolist() == [0] and sk.tolist() == [0]


def test_two_calls_return_the_same_bytes(FO):
    frames = [SCENES[n][0] for n in ("timing_shape", "all_4096_in_one_box", "map_point_at_two_keypoints")]
    first = raw_bytes(FO.frame_objects_raw(frames))
    for _ in range(3):
        assert raw_bytes(FO.frame_objects_raw(frames)) == first


def test_four_host_threads(FO):
    frames = [SCENES[n][0] for n in ("timing_shape", "n_kp_257", "edge_rules")]
    first = raw_bytes(FO.frame_objects_raw(frames))
    out, errs = [None] * 4, []

    def work(i):
        try:
            out[i] = [raw_bytes(FO.frame_objects_raw(frames)) for _ in range(3)]
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs and all(o is not None and all(b == first for b in o) for o in out)


def test_capacity(FO):
    """a list buffer that is too short: the starts hold the counts, nothing else is written"""
    fr = SCENES["timing_shape"][0]
    w = want("timing_shape")
    total_a, total_k = sum(len(l) for l in w["assigned"]), sum(len(l) for l in w["kept"])
    assert total_k < total_a
    for ca, ck in ((total_a - 1, total_k), (total_a, total_k - 1), (0, 0)):
        st, rec, sa, la, sk, lk = FO.frame_objects_raw([fr], assigned_cap=ca, kept_cap=ck, fill=0xAB)
        assert st == CAPACITY
        assert np.array_equal(np.diff(sa), [len(l) for l in w["assigned"]]) and np.array_equal(np.diff(sk), [len(l) for l in w["kept"]]) and sa[0] == 0 and sk[0] == 0
        assert set(rec.tobytes()) == {0xAB} and set(la.tobytes()) <= {0xAB} and set(lk.tobytes()) <= {0xAB}
    st, rec, sa, la, sk, lk = FO.frame_objects_raw([fr], assigned_cap=total_a, kept_cap=total_k, fill=0xAB)      # exactly enough
    assert st == OK and Y.same(dict(records=rec, assigned=[la[sa[k]:sa[k + 1]] for k in range(16)], kept=[lk[sk[k]:sk[k + 1]] for k in range(16)]), w)


def refusals():
    base = SCENES["three_four_seven_eight_points"][0]

    def edit(**kw):
        fr = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in base.items()}
        for k, (i, v) in kw.items():
            if i is None:
                fr[k] = v
            else:
                fr[k][i] = v
        return fr

    big = SC.frame(np.zeros((4097, 2)), np.zeros((4097, 3)), [(0, 0, 10, 10)])
    many = SC.frame(np.zeros((1, 2)), np.zeros((1, 3)), [(0, 0, 10, 10)] * 257)
    Tnan = base["Tcw"].copy()
    Tnan[1, 2] = np.nan
    return {"kp_nan": edit(kp_x=(3, np.nan)), "kp_inf": edit(kp_y=(0, np.inf)), "xyz_inf": edit(mp_xyz=((2, 1), -np.inf)), "pose_nan": edit(Tcw=(None, Tnan)),
            "fx_inf": edit(fx=(None, np.inf)), "kp_2_30": edit(kp_x=(1, 2.0 ** 30)), "kp_minus_2_30": edit(kp_y=(1, -2.0 ** 30)),
            "negative_width": edit(boxes=((1, 2), -1)), "negative_height": edit(boxes=((0, 3), -5)), "box_beyond_2_15": edit(boxes=((2, 0), 2 ** 15 + 1)),
            "width_beyond_2_15": edit(boxes=((2, 2), 2 ** 15 + 1)), "n_kp_4097": big, "n_box_257": many, "mp_id_minus_2": edit(mp_id=(5, -2)),
            "cols_beyond_2_15": edit(cols=(None, 2 ** 15 + 1))}


REFUSALS = refusals()


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusal_leaves_the_outputs_untouched(FO, name):
    good = SCENES["box_edges"][0]
    for frames in ([REFUSALS[name]], [good, REFUSALS[name]]):      # alone, and behind a frame that is fine
        raw = FO.frame_objects_raw(frames, fill=0xAB)
        assert raw[0] == INVALID
        assert all(set(np.ascontiguousarray(a).tobytes()) <= {0xAB} for a in raw[1:])


def test_a_non_finite_position_without_a_map_point_is_not_read(FO):
    fr = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in SCENES["n_kp_65"][0].items()}
    i = int(np.nonzero(fr["mp_id"] < 0)[0][0])
    fr["mp_xyz"][i] = np.nan
    assert Y.same(FO.frame_objects(fr), want("n_kp_65"))


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("frame_objects") / "frame_objects_walk")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", os.path.join(ROOT, "tools", "frame_objects_walk.cpp"), "-o", exe])
    return exe


def test_device_equals_the_host_header(FO, walk):
    """every scene through the literal walk of csrc/frame_objects_internal.h (one run of the program); the signs of zero quartiles are the sort's there"""
    out = subprocess.run([walk], input="".join(Y.walk_script(SCENES[n][0]) for n in NAMES), capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    lines, at = out.stdout.strip().split("\n"), 0
    for n, g in zip(NAMES, FO.frame_objects_batch([SCENES[n][0] for n in NAMES])):
        mine = Y.walk_lines(g, zero_signs=False)
        host = lines[at:at + len(mine)]
        at += len(mine)
        rec = [i for i, l in enumerate(host) if l.startswith("rec ")]
        assert len(rec) == len(g["records"]), n
        # the host prints the sort's zero signs: compare the q1 / q3 / max_th columns by value, everything else as text
        for i, (h, m) in enumerate(zip(host, mine)):
            if i in rec:
                hc, mc = h.split(), m.split()
                for c in (21, 22, 23):
                    if hc[c] in ("00000000", "80000000"):
                        hc[c] = "00000000"
                assert hc == mc, (n, i)
            else:
                assert h == m, (n, i)
    assert at == len(lines)


def test_profiling(FO):
    from eao_fusion_amd import _lib
    FO.set_profiling(True)
    try:
        FO.frame_objects(SCENES["timing_shape"][0])
        ms = FO.last_kernel_ms()
        assert len(ms) == 3 and all(m == -1 or 0 <= m < 1000 for m in ms) and any(m >= 0 for m in ms)
    finally:
        FO.set_profiling(False)
    seen = []
    t = threading.Thread(target=lambda: seen.append(_lib.load().eao_frame_objects_last_kernel_ms((C.c_float * 3)())))
    t.start()
    t.join()
    assert seen == [INVALID]      # nothing was measured on that thread


# ---- the adapter (include/eaofusion/FrameObjects.h) over stand-in Frame / MapPoint / Object_2D, on into the rank-sum test for one surviving object
@pytest.fixture(scope="module")
def adapter(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("frame_objects_adapter") / "frame_objects_driver")
    lib = os.path.join(ROOT, "eao_fusion_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-DEAOFUSION_FORCE_CV_COMPAT", "-DFRAME_OBJECTS_DEVICE", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "frame_objects", "frame_objects_driver.cpp"), "-o", exe, "-L", lib, "-leaofusion_hip",
                           "-Wl,-rpath," + lib])
    return exe


def test_adapter_on_the_device(FO, adapter):
    """BuildFrameObjects over the timing-shaped frame, the survivors' members against the yardstick, and one survivor against itself through
    eao_object_np_association_batch: a sample tested against its own distribution associates when it has at least 20 points"""
    fr = SCENES["timing_shape"][0]
    w = want("timing_shape")
    out = subprocess.run([adapter, "single"], input=Y.walk_script(fr), capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.strip().split("\n")
    alive = [k for k in range(16) if not w["records"]["bad"][k]]
    assert lines[0] == "frame 0 ret %d" % len(alive) and "survivors " + " ".join(str(k) for k in alive) in lines
    lists = {int(l.split()[1]): [int(v) for v in l.split()[2:]] for l in lines if l.startswith("list ")}
    assert all(lists[k] == [int(i) for i in w["kept"][k]] for k in alive)      # (no map point sits at two keypoints in this scene)
    got = {int(l.split()[1]): l.split()[2:] for l in lines if l.startswith("obj ")}
    for k in alive:
        r = w["records"][k]
        fl = np.concatenate([r["sum_pos"], r["pos"], r["std"], r["center_2d"]]).astype(np.float32)
        assert got[k] == [str(int(r["n"])), str(int(r["on_edge"]))] + [str(int(v)) for v in r["feature_rect"]] + ["%08x" % v for v in fl.view(np.uint32)], k
    big = [k for k in alive if w["records"]["n"][k] >= 20]
    assert big and lines[-1] == "np %d 1" % big[0]
