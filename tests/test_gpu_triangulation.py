"""GPU: the triangulation half of LocalMapping::CreateNewMapPoints (eao_triangulate_matches_batch, eao_keyframe_set_depth, eao_kf_create_new_map_points; reference
src/LocalMapping.cc:288-454) against the numpy yardstick of tests/triangulation_reference.py over the scenes of tests/triangulation_scenes.py.
Every bound comes from tests/triangulation_tolerances.py."""
import os
import sys
import threading

import numpy as np
import pytest

import triangulation_reference as Y
import triangulation_scenes as S
from triangulation_tolerances import MARGIN_REL, x3d_rel

from eao_fusion_amd import search, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = list(S.all_scenes())


@pytest.fixture(scope="module")
def g():
    import torch  # noqa: F401  (first, so that the library resolves the same HIP runtime)
    import eao_fusion_amd as E
    assert E.load().eao_device_check() == 0, E.load().eao_last_error()
    return search.product()


def _device(g, sc):
    return g.triangulate_matches_batch(sc["K1"], sc["cam1"], sc["K2s"], sc["cams2"], sc["match12"], sc["ratio_factor"])


@pytest.fixture(scope="module")
def device(g):
    """every scene through the device once; the tests below share the results and leave them unchanged"""
    return {name: _device(g, sc) for name, sc in S.all_scenes().items()}


@pytest.fixture(scope="module")
def yard():
    return {name: Y.triangulate_batch(sc["K1"], sc["cam1"], sc["K2s"], sc["cams2"], sc["match12"], sc["ratio_factor"]) for name, sc in S.all_scenes().items()}


@pytest.mark.parametrize("name", SCENES)
def test_replay_of_the_devices_own_points(device, name):
    """gates_after_point on the device's x3d gives the device's verdict, bit for bit, for EVERY pair: an accepted pair passes every gate, a pair rejected with a
    point is rejected by that gate; a verdict without a point, and an empty slot, carry zeros."""
    sc = S.all_scenes()[name]
    verdict, x3d = device[name]
    assert verdict.shape == sc["match12"].shape and x3d.shape == sc["match12"].shape + (3,)
    for k, row in enumerate(sc["match12"]):
        empty = row < 0
        assert (verdict[k][empty] == Y.EMPTY).all() and not x3d[k][empty].any()
        idx1 = np.nonzero(~empty)[0]
        if len(idx1) == 0:
            continue
        dv, dx = verdict[k][idx1], x3d[k][idx1]
        assert ((dv >= 1) & (dv <= 12)).all()
        gate, _m = Y.gates_after_point(sc["K1"], sc["cam1"], sc["K2s"][k], sc["cams2"][k], row, sc["ratio_factor"], dx)
        has = np.isin(dv, Y.HAS_POINT)
        want = np.where(np.isin(dv, Y.ACCEPTING), 0, dv)
        assert np.array_equal(gate[has], want[has]), (name, k, idx1[has][gate[has] != want[has]])
        assert not dx[~has].any()


@pytest.mark.parametrize("name", SCENES)
def test_parity_with_the_yardstick(device, yard, name):
    """The verdict (the branch is the accepting code) of every pair the yardstick does not place inside MARGIN_REL of a comparison, and x3d of the accepted ones
    within the scene's X3D_REL of their distance to Ow1.  NaN inputs: the same verdict and NaN in the same places."""
    sc = S.all_scenes()[name]
    verdict, x3d = device[name]
    _yv, _yx, per = yard[name]
    Ow1 = np.asarray(sc["cam1"]["Ow"], np.float64)
    compared = 0
    for k, p in enumerate(per):
        if len(p["idx1"]) == 0:
            continue
        dv, dx = verdict[k][p["idx1"]], x3d[k][p["idx1"]]
        yx = p["x3d"][p["idx1"]]
        clear = ~(p["near"] < MARGIN_REL)
        assert np.array_equal(dv[clear], p["pair_verdict"][clear]), (name, k, [(int(i), Y.VERDICT_NAMES[a], Y.VERDICT_NAMES[b]) for i, a, b in
                                                                              zip(p["idx1"][clear], dv[clear], p["pair_verdict"][clear]) if a != b][:8])
        assert np.array_equal(np.isnan(dx), np.isnan(yx))
        acc = clear & np.isin(dv, Y.ACCEPTING) & ~np.isnan(yx).any(axis=1)
        d = np.linalg.norm(yx.astype(np.float64) - Ow1, axis=1)
        err = np.linalg.norm(dx.astype(np.float64) - yx.astype(np.float64), axis=1)
        print("%s neighbour %d: largest |dX| / |X - Ow1| %.3e of %.3e" % (name, k, float((err[acc] / d[acc]).max()) if acc.any() else 0.0, x3d_rel(name)))
        assert (err[acc] <= x3d_rel(name) * d[acc]).all(), (name, k, float((err[acc] / d[acc]).max()))
        compared += int(clear.sum())
    total = sum(len(p["idx1"]) for p in per)
    assert compared >= 0.99 * total or not sc["friendly"]


def test_twenty_neighbours_equal_twenty_calls_of_one(g, device):
    sc = S.all_scenes()["twenty"]
    verdict, x3d = device["twenty"]
    for k in range(len(sc["K2s"])):
        v1, x1 = g.triangulate_matches_batch(sc["K1"], sc["cam1"], [sc["K2s"][k]], [sc["cams2"][k]], sc["match12"][k:k + 1], sc["ratio_factor"])
        assert v1[0].tobytes() == verdict[k].tobytes() and x1[0].tobytes() == x3d[k].tobytes(), k


@pytest.mark.parametrize("name", ["twenty", "stereo_mix", "nan_row"])
def test_second_call_returns_the_same_bytes(g, device, name):
    v, x = _device(g, S.all_scenes()[name])
    assert v.tobytes() == device[name][0].tobytes() and x.tobytes() == device[name][1].tobytes()


def _in_thread(fn):
    """fn() on a new thread: the library's per-thread stream and buffers start fresh there"""
    box = {}

    def run():
        try:
            box["r"] = fn()
        except BaseException as e:      # noqa: BLE001
            box["e"] = e
    t = threading.Thread(target=run)
    t.start()
    t.join()
    if "e" in box:
        raise box["e"]
    return box["r"]


def test_sizes_in_sequence_on_one_thread_equal_fresh_calls(g):
    """257 -> 0 -> 1 -> 65 -> 257 pairs on ONE thread (its grow-only buffers keep what the larger call left) against each size on a thread of its own."""
    seq = [S.sized(n) for n in (257, 0, 1, 65, 257)]
    got = _in_thread(lambda: [_device(g, sc) for sc in seq])
    for sc, (v, x) in zip(seq, got):
        fv, fx = _in_thread(lambda sc=sc: _device(g, sc))
        assert v.tobytes() == fv.tobytes() and x.tobytes() == fx.tobytes(), sc["name"]
        assert (v > 0).sum() == (sc["match12"] >= 0).sum()


def test_two_threads_return_the_serial_results(g, device):
    names = ("twenty", "stereo_mix")
    out = {n: [] for n in names}

    def work(n):
        for _ in range(4):
            out[n].append(_device(g, S.all_scenes()[n]))
    ts = [threading.Thread(target=work, args=(n,)) for n in names]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for n in names:
        assert len(out[n]) == 4
        for v, x in out[n]:
            assert v.tobytes() == device[n][0].tobytes() and x.tobytes() == device[n][1].tobytes(), n


# ---------------------------------------------------------------------------------------------------------------- resident keyframes
def _cam_of(T, K, bf, dz=0.0):
    T = np.asarray(T, np.float32)
    R, t = T[:3, :3].copy(), T[:3, 3].copy()
    t[2] += np.float32(dz)
    Ow = (-(R.astype(np.float64).T @ t.astype(np.float64))).astype(np.float32)
    fx, fy, cx, cy = (np.float32(v) for v in K)
    return dict(Rcw=R, tcw=t, Ow=Ow, fx=fx, fy=fy, cx=cx, cy=cy, invfx=np.float32(1.0) / fx, invfy=np.float32(1.0) / fy, mb=np.float32(bf) / fx, mbf=np.float32(bf))


def _with_depth(frame, bf):
    """mvDepth of a search-scene keyframe from its right coordinates (depth = mbf / disparity), mvKeys a little off mvKeysUn"""
    f = dict(frame)
    ur = np.asarray(f["u_right"], np.float32)
    with np.errstate(all="ignore"):
        f["depth"] = np.where(ur >= 0, np.float32(bf) / (f["kp_x"] - ur), np.float32(-1)).astype(np.float32)
    f["raw_x"] = (f["kp_x"] + np.float32(0.125)).astype(np.float32)
    f["raw_y"] = (f["kp_y"] - np.float32(0.0625)).astype(np.float32)
    return f


@pytest.mark.parametrize("kw,n_nb,only_stereo", [(dict(), 7, 0), (dict(n=1200, seed=8001, flip=0.09, mono_frac=0.6), 18, 0), (dict(n=300, seed=8002, clutter=0.5, n_nodes=12), 3, 1),
                                                 (dict(contended=True, n=600, seed=8501, n_nodes=9, dup_points=0.4, dup_keypoints=0.4), 5, 0)])
def test_create_new_map_points_on_handles(g, kw, n_nb, only_stereo):
    """eao_kf_create_new_map_points = eao_kf_search_for_triangulation, then eao_triangulate_matches_batch on its table, byte for byte -- over the two-keyframe
    search scenes and neighbour variants of tests/test_gpu_search.py with poses and depths added (18 neighbours: two launches of 16 and 2)."""
    import test_gpu_search as TS
    kw = dict(kw)
    scene = (synth.synth_search_scene_contended if kw.pop("contended", False) else synth.synth_search_scene)(**kw)
    h = search.product_handles()
    bf = scene["bf"]
    k1 = _with_depth(scene["K1"], bf)
    k1["occupied"] = ((scene["mp1"] >= 0) & (np.arange(len(scene["mp1"])) % 2 == 0)).astype(np.uint8)
    nb = TS._neighbours(scene, n_nb)
    k2s = [_with_depth(x[0], bf) for x in nb]
    cam1 = _cam_of(scene["T1w"], scene["K"], bf)
    cams2 = [_cam_of(scene["T2w"], scene["K"], bf * (1.0 + 0.05 * (k % 3)), dz=0.01 * k) for k in range(n_nb)]
    rf = Y.ratio_factor(scene["K1"]["scale_factors"][1])
    h1 = search.KeyFrameHandle(h.lib, h.check, k1, scene["fv1"])
    h2s = [search.KeyFrameHandle(h.lib, h.check, k2, x[1]) for k2, x in zip(k2s, nb)]
    F, ex, ey = [x[2] for x in nb], [x[3] for x in nb], [x[4] for x in nb]
    # a handle without depth: refused before anything is written
    sent = (np.full(n_nb, -7, np.int32), np.full((n_nb, h1.n), -7, np.int32), np.full((n_nb, h1.n), -7, np.int32), np.full((n_nb, h1.n, 3), np.float32(-7), np.float32))
    search.keyframe_set_depth(h1, k1["depth"], k1["raw_x"], k1["raw_y"])
    for hh, k2 in zip(h2s[:-1], k2s[:-1]):
        hh.set_depth(k2["depth"], k2["raw_x"], k2["raw_y"])
    with pytest.raises(Exception) as ei:
        h.create_new_map_points_h(h1, cam1, h2s, cams2, F, ex, ey, only_stereo, rf, True, out=sent)
    assert getattr(ei.value, "status", None) == -1 and all((a == -7).all() for a in sent)
    h2s[-1].set_depth(k2s[-1]["depth"], k2s[-1]["raw_x"], k2s[-1]["raw_y"])
    nm0, m0 = h.search_for_triangulation_h(h1, h2s, F, ex, ey, only_stereo, True)
    nm, m, verdict, x3d = search.kf_create_new_map_points(h1, cam1, h2s, cams2, F, ex, ey, only_stereo, rf, True)
    assert nm.tobytes() == nm0.tobytes() and m.tobytes() == m0.tobytes()
    v2, x2 = g.triangulate_matches_batch(k1, cam1, k2s, cams2, m0, rf)
    assert verdict.tobytes() == v2.tobytes() and x3d.tobytes() == x2.tobytes()
    assert np.isin(verdict, Y.ACCEPTING).sum() > 20 and (verdict > 0).sum() == nm0.sum()
    # ... and again (the search's generation stamps and the triangulation's buffers have moved on)
    nm_b, m_b, v_b, x_b = search.kf_create_new_map_points(h1, cam1, h2s, cams2, F, ex, ey, only_stereo, rf, True)
    assert m_b.tobytes() == m0.tobytes() and v_b.tobytes() == v2.tobytes() and x_b.tobytes() == x2.tobytes()
    # the search entry point alone still returns what it returned
    nm1, m1 = h.search_for_triangulation_h(h1, h2s, F, ex, ey, only_stereo, True)
    assert nm1.tobytes() == nm0.tobytes() and m1.tobytes() == m0.tobytes()


def test_invalid_arguments_fail_before_anything_is_written(g):
    sc = S.all_scenes()["stereo_mix"]
    n_nb, n1 = sc["match12"].shape
    args = (sc["K1"], sc["cam1"], sc["K2s"], sc["cams2"], sc["match12"], sc["ratio_factor"])

    def refused(**kw):
        with pytest.raises(Exception) as ei:
            g.triangulate_matches_batch(*args, **kw)
        assert getattr(ei.value, "status", None) == -1, ei.value
    v, x = np.full((n_nb, n1), -7, np.int32), np.full((n_nb, n1, 3), np.float32(-7), np.float32)
    refused(out=(None, x))
    refused(out=(v, None))
    refused(out=(v, x), n_nb=-1)
    bad = sc["match12"].copy()
    bad[1, 5] = len(sc["K2s"][1]["kp_x"])      # one past the neighbour's last keypoint
    with pytest.raises(Exception) as ei:
        g.triangulate_matches_batch(sc["K1"], sc["cam1"], sc["K2s"], sc["cams2"], bad, sc["ratio_factor"], out=(v, x))
    assert getattr(ei.value, "status", None) == -1
    k1 = dict(sc["K1"], kp_octave=np.where(np.arange(n1) == 3, 8, sc["K1"]["kp_octave"]).astype(np.int32))
    with pytest.raises(Exception) as ei:
        g.triangulate_matches_batch(k1, sc["cam1"], sc["K2s"], sc["cams2"], sc["match12"], sc["ratio_factor"], out=(v, x))
    assert getattr(ei.value, "status", None) == -1
    assert (v == -7).all() and (x == -7).all()
    # no neighbours: nothing to do, nothing written
    v0, x0 = g.triangulate_matches_batch(sc["K1"], sc["cam1"], [], [], np.zeros((0, n1), np.int32), sc["ratio_factor"])
    assert v0.shape == (0, n1) and x0.shape == (0, n1, 3)


def test_golden_files_on_the_device(g):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_golden_triangulation as G
    d = os.path.join(ROOT, "tests", "golden", "triangulation")
    sc = G.unpack(np.load(os.path.join(d, "inputs.npz")))
    want_v, want_x = np.load(os.path.join(d, "verdicts.npz"))["verdict"], np.load(os.path.join(d, "points.npz"))["x3d"]
    v, x = g.triangulate_matches_batch(sc["K1"], sc["cam1"], sc["K2s"], sc["cams2"], sc["match12"], sc["ratio_factor"])
    assert np.array_equal(v, want_v)      # (the CPU test holds the scene clear of every comparison by more than MARGIN_REL)
    acc = np.isin(v, Y.ACCEPTING)
    d1 = np.linalg.norm(want_x.astype(np.float64) - np.asarray(sc["cam1"]["Ow"], np.float64), axis=2)
    assert acc.sum() > 150 and (np.linalg.norm(x.astype(np.float64) - want_x, axis=2)[acc] <= x3d_rel("stereo_mix") * d1[acc]).all()      # (the recorded scene is stereo_mix)


def test_cpp_triangulation_adapters(g, tmp_path):
    """include/eaofusion/LocalMapping.h over stand-in KeyFrames (tests/cpp/triangulate_adapter_test.cpp: both forms, the dropped duplicates, the refused handle);
    the accepted pairs it writes are those of the C-ABI through the Python mirror, less the pairs whose idx1 an earlier neighbour already served."""
    import struct
    import subprocess
    import test_gpu_search as TS
    exe = str(tmp_path / "triangulate_adapter_test")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-DEAOFUSION_FORCE_CV_COMPAT", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "triangulate_adapter_test.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "eao_fusion_amd"), "-leaofusion_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "eao_fusion_amd"), "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    scene = synth.synth_search_scene(n=500, seed=8200)
    bf, n_nb = scene["bf"], 4
    k1 = _with_depth(scene["K1"], bf)
    k1["occupied"] = ((scene["mp1"] >= 0) & (np.arange(len(scene["mp1"])) % 2 == 0)).astype(np.uint8)
    nb = TS._neighbours(scene, n_nb)
    k2s = [_with_depth(x[0], bf) for x in nb]
    cam1 = _cam_of(scene["T1w"], scene["K"], bf)
    cams2 = [_cam_of(scene["T2w"], scene["K"], bf, dz=0.01 * k) for k in range(n_nb)]
    # the epipoles as the adapter forms them (src/ORBmatcher.cc:663-670), so that the mirror's search sees the same arguments
    exs, eys = [], []
    for c in cams2:
        C2 = [np.float32(np.float64(c["Rcw"][r, 0]) * np.float64(cam1["Ow"][0]) + np.float64(c["Rcw"][r, 1]) * np.float64(cam1["Ow"][1])
                         + np.float64(c["Rcw"][r, 2]) * np.float64(cam1["Ow"][2]) + np.float64(c["tcw"][r])) for r in range(3)]
        invz = np.float32(1.0) / C2[2]
        exs.append(c["fx"] * C2[0] * invz + c["cx"])
        eys.append(c["fy"] * C2[1] * invz + c["cy"])
    path = str(tmp_path / "scene.bin")
    with open(path, "wb") as f:
        K1 = scene["K1"]
        f.write(K1["scale_factors"].tobytes()); f.write(K1["level_sigma2"].tobytes()); f.write(K1["inv_level_sigma2"].tobytes())
        f.write(struct.pack("<fi", float(K1["log_scale_factor"]), n_nb))
        for K, fv, cam, F in [(k1, scene["fv1"], cam1, None)] + [(k2, x[1], c, x[2]) for k2, x, c in zip(k2s, nb, cams2)]:
            n = len(K["kp_x"])
            f.write(struct.pack("<i", n))
            for key in ("kp_x", "kp_y", "kp_angle", "u_right"):
                f.write(np.ascontiguousarray(K[key], np.float32).tobytes())
            f.write(np.ascontiguousarray(K["kp_octave"], np.int32).tobytes())
            f.write(np.ascontiguousarray(K.get("occupied") if K.get("occupied") is not None else np.zeros(n), np.uint8).tobytes())
            f.write(np.ascontiguousarray(K["descriptors"], np.uint8).tobytes())
            for key in ("depth", "raw_x", "raw_y"):
                f.write(np.ascontiguousarray(K[key], np.float32).tobytes())
            f.write(struct.pack("<i", len(fv["node_id"])))
            f.write(fv["node_id"].astype(np.uint32).tobytes()); f.write(fv["node_start"].astype(np.int32).tobytes()); f.write(fv["index"].astype(np.uint32).tobytes())
            f.write(np.concatenate([cam["Rcw"].ravel(), cam["tcw"], cam["Ow"], [cam[k] for k in search.TRI_CAMERA_SCALARS]]).astype(np.float32).tobytes())
            if F is not None:
                f.write(np.ascontiguousarray(F, np.float32).tobytes())
    res = str(tmp_path / "result.bin")
    out = subprocess.run([exe, path, res], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "duplicates dropped" in out.stderr
    # the same through the mirror
    nm, m = g.search_for_triangulation_batch(k1, scene["fv1"], k2s, [x[1] for x in nb], [x[2] for x in nb], exs, eys, 0, False)
    verdict, x3d = g.triangulate_matches_batch(k1, cam1, k2s, cams2, m, Y.ratio_factor(scene["K1"]["scale_factors"][1]))
    buf = open(res, "rb").read()
    off = 4
    dropped = struct.unpack_from("<i", buf, 0)[0]
    served, want_dropped = set(), 0
    for k in range(n_nb):
        cnt = struct.unpack_from("<i", buf, off)[0]
        off += 4
        want = []
        for i in np.nonzero(np.isin(verdict[k], Y.ACCEPTING))[0]:
            if int(i) in served:
                want_dropped += 1
                continue
            served.add(int(i))
            want.append((int(i), int(m[k, i]), int(verdict[k, i]), x3d[k, i].tobytes()))
        got = []
        for _ in range(cnt):
            i1, i2, v = struct.unpack_from("<iii", buf, off)
            got.append((i1, i2, v, buf[off + 12:off + 24]))
            off += 24
        assert got == want, k
    assert off == len(buf) and dropped == want_dropped and dropped > 0 and len(served) > 20
