"""The yolox feature on the device (eao_fusion_amd/csrc/yolox.hip through eao_fusion_amd/yolox.py) against the yardstick (tests/yolox_reference.py, the
double-precision exponential, the device's tie rule): integers as integers, floats as 32-bit patterns, no tolerance anywhere."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import yolox_reference as Y
import yolox_scenes as SC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden_yolox as G  # noqa: E402

SCENES = SC.scenes()
SMALL = sorted(n for n, s in SCENES.items() if s["S"] == 64 and "max_proposals" not in s)


@pytest.fixture(scope="module")
def YX():
    import torch  # noqa: F401  (first, so that both runtimes resolve the same libamdhip64)
    from eao_fusion_amd import yolox
    return yolox


@pytest.fixture(scope="module")
def h64(YX):
    return YX.Yolox(input_size=64, max_batch=4)


@pytest.fixture(scope="module")
def h640(YX):
    return YX.Yolox(max_batch=2)


@pytest.fixture(scope="module")
def want():
    """the yardstick's decode of every scene, once"""
    return {name: Y.decode_vectorised(s["feat"], s["S"], *s["img"]) for name, s in SCENES.items()}


def image(w, h, seed):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def expected_pre(oracle, img, S, rgb):
    return Y.blob_vectorised(Y.letterbox(img, S, oracle.resize_linear)), Y.gray(img, rgb)


def hip_memcpy(dst, src, nbytes, kind):
    """hipMemcpy of the HIP runtime this process already holds (kind 1: host to device, 2: device to host)"""
    import ctypes
    path = next(ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln)
    hip = ctypes.CDLL(path)
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    assert hip.hipMemcpy(dst, src, nbytes, kind) == 0


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


# ---------------------------------------------------------------- pre-processing
PRE_640 = [(640, 480), (1064, 20), (320, 240), (1280, 40), (848, 480), (100, 700), (37, 23)]


@pytest.mark.parametrize("w,h", PRE_640)
def test_preprocess_640(h640, oracle, w, h):
    """identity, the padding column 639, x 2 up (offset -1), x 2 down, the two letterbox orientations, a small odd frame"""
    img = image(w, h, 100 + w)
    blob, gray = h640.preprocess(img, rgb=False, want_gray=True)
    eb, eg = expected_pre(oracle, img, 640, False)
    assert same_bits(blob[0], eb) and np.array_equal(gray[0], eg)
    if (w, h) == (640, 480):
        t = Y.blob_table()
        assert same_bits(blob[0][:, :480, :], np.stack([t[c][img[:, :, 2 - c]] for c in range(3)]))
    if (w, h) == (1064, 20):
        assert same_bits(blob[0][:, :, 639], np.repeat(Y.blob_table()[:, Y.PAD:Y.PAD + 1], 640, axis=1))


@pytest.mark.parametrize("w,h,rgb", [(37, 23, False), (37, 23, True), (64, 48, False), (128, 40, True), (100, 70, False), (9, 150, True)])
def test_preprocess_64(h64, oracle, w, h, rgb):
    img = image(w, h, 200 + w)
    blob, gray = h64.preprocess(img, rgb=rgb, want_gray=True)
    eb, eg = expected_pre(oracle, img, 64, rgb)
    assert same_bits(blob[0], eb) and np.array_equal(gray[0], eg)


def test_preprocess_stride_and_batch(h64, oracle):
    wide = np.random.RandomState(5).randint(0, 256, (3, 30, 60, 3)).astype(np.uint8)
    view = wide[:, :, 7:52]                                   # rows 180 bytes apart, 45 pixels used
    blobs, grays = h64.preprocess(view, rgb=True, want_gray=True)
    for f in range(3):
        eb, eg = expected_pre(oracle, np.ascontiguousarray(view[f]), 64, True)
        assert same_bits(blobs[f], eb) and np.array_equal(grays[f], eg)
        one = h64.preprocess(np.ascontiguousarray(view[f]))
        assert same_bits(one[0], eb)


def test_preprocess_refused_geometry_leaves_outputs(h64, YX):
    from eao_fusion_amd import _lib
    img = image(37, 23, 1)
    h64.preprocess(img)
    before = h64.blob(0)
    gray = np.full((1, 1, 200), 7, np.uint8)
    with pytest.raises(_lib.EaoError) as e:
        h64.preprocess(image(200, 1, 2), gray=gray)          # unpad_h = (int)(0.32 * 1) = 0
    assert e.value.status == _lib.EAO_ERR_INVALID and (gray == 7).all()
    with pytest.raises(_lib.EaoError):
        h64.blob(1)
    assert same_bits(h64.blob(0), before)


def test_gray_feeds_the_extractor(h640, YX):
    """the pitched grey buffer of eao_yolox_preprocess_device goes straight into eao_orb_extract_batch_device: the keypoints and descriptors of
    eao_orb_extract on the yardstick's grey image"""
    import torch
    import eao_fusion_amd as E
    from eao_fusion_amd import synth
    from eao_fusion_amd.orb import KP_DTYPE
    g = synth.synth_frames(1, seed0=1000)[0]
    hh, ww = g.shape
    rs = np.random.RandomState(3)
    img = np.stack([np.clip(g.astype(np.int32) + rs.randint(-20, 21, g.shape), 0, 255) for _ in range(3)], axis=2).astype(np.uint8)
    pitch = (ww + 63) // 64 * 64
    d_img = torch.from_numpy(img).cuda()
    d_blob = torch.zeros((1, 3, 640, 640), dtype=torch.float32, device="cuda")
    d_gray = torch.zeros((hh, pitch), dtype=torch.uint8, device="cuda")
    ext = E.ORBextractor(1000, 1.2, 8, 20, 7)
    cap = ext.max_keypoints(ww, hh)
    d_kps = torch.zeros(cap * KP_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    d_desc = torch.zeros((cap, 32), dtype=torch.uint8, device="cuda")
    d_n = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    h640.preprocess_device(d_img.data_ptr(), ww, hh, 3 * ww, 3 * ww * hh, 1, False, d_blob.data_ptr(), d_gray.data_ptr(), pitch, None)
    ext.extract_batch_device(d_gray.data_ptr(), ww, hh, pitch, pitch * hh, 1, d_kps.data_ptr(), d_desc.data_ptr(), cap, d_n.data_ptr(), None)
    torch.cuda.synchronize()
    eg = Y.gray(img, False)
    assert np.array_equal(d_gray.cpu().numpy()[:, :ww], eg)
    n = int(d_n.cpu()[0])
    kps = d_kps.cpu().numpy().view(KP_DTYPE)[:n]
    wk, wd = ext(eg)
    assert n == len(wk) > 100 and kps.tobytes() == wk.tobytes() and np.array_equal(d_desc.cpu().numpy()[:n], wd)


# ---------------------------------------------------------------- decode
def check_frame(got, w, props=None):
    assert got["n_proposals"] == len(w["proposals"]) and got["n_tied"] == w["n_tied"]
    assert Y.same_records(got["objects"].view(Y.OBJECT), w["objects"])
    if props is not None:
        assert Y.same_records(props.view(Y.OBJECT), w["proposals"])


@pytest.mark.parametrize("name", SMALL)
def test_decode_scene(h64, want, name):
    s = SCENES[name]
    got = h64.decode(s["feat"], [s["img"]])[0]
    check_frame(got, want[name], h64.proposals(0))
    assert s["reaches"](dict(want[name], ious=Y.decode_literal(s["feat"], 64, *s["img"], stable=True)["ious"])), s["branch"]


def test_decode_head_640(h640, want):
    s = SCENES["head_640"]
    check_frame(h640.decode(s["feat"], [s["img"]])[0], want["head_640"], h640.proposals(0))


def test_capacity(YX, want):
    from eao_fusion_amd import _lib
    h = YX.Yolox(input_size=64, max_proposals=128, max_batch=3)
    s = SCENES["capacity_128"]
    check_frame(h.decode(s["feat"], [s["img"]])[0], want["capacity_128"], h.proposals(0))
    # one more: the true count, and nothing else; alone and in a batch whose other frames fit
    o = SCENES["capacity_129"]
    for heads in ([o["feat"]], [SCENES["clusters"]["feat"], o["feat"], SCENES["one"]["feat"]]):
        out = dict(objects=np.full((len(heads), 128), -3, YX.OBJECT), n=np.full(len(heads), -5, np.int32), n_proposals=np.full(len(heads), -5, np.int32),
                   n_tied=np.full(len(heads), -5, np.int32))
        r = h.decode_raw(np.stack(heads), [(100, 80)] * len(heads), out=out)
        assert r["status"] == _lib.EAO_ERR_CAPACITY
        assert r["n_proposals"].tolist() == ([129] if len(heads) == 1 else [6, 129, 1])
        assert (out["objects"] == np.full(1, -3, YX.OBJECT)[0]).all() and (out["n"] == -5).all() and (out["n_tied"] == -5).all()
    with pytest.raises(_lib.EaoError):
        h.proposals(0)
    h.close()


def test_batch_equals_single_calls(h64, want):
    names = ["clusters", "random_64", "tie", "count_65"]
    got = h64.decode(np.stack([SCENES[n]["feat"] for n in names]), [SCENES[n]["img"] for n in names])
    for f, n in enumerate(names):
        check_frame(got[f], want[n], h64.proposals(f))


def test_host_and_device_entry_points_agree(h64, want):
    import torch
    names = ["nested", "random_64"]
    d = torch.from_numpy(np.stack([SCENES[n]["feat"] for n in names])).cuda()
    torch.cuda.synchronize()
    got = h64.decode_device(d.data_ptr(), 2, [SCENES[n]["img"] for n in names])
    for f, n in enumerate(names):
        check_frame(got[f], want[n])
    # through the handle's own buffers and stream, as the adapter does
    _, d_prob, stream = h64.buffers()
    s = SCENES["clusters"]
    hip_memcpy(d_prob, s["feat"].ctypes.data, s["feat"].nbytes, 1)
    check_frame(h64.decode_device(d_prob, 1, [s["img"]], stream=stream)[0], want["clusters"])


def test_determinism_across_calls_and_threads(YX, want):
    names = ["random_64", "tie", "clusters", "count_64"]
    shared = YX.Yolox(input_size=64)
    errors = []

    def work(k, handle):
        try:
            s = SCENES[names[k]]
            first = None
            for _ in range(20):
                r = handle.decode(s["feat"], [s["img"]])[0]
                check_frame(r, want[names[k]])
                first = first or r["objects"].tobytes()
                assert r["objects"].tobytes() == first
        except Exception as e:      # noqa: BLE001
            errors.append((k, repr(e)))

    for handles in ([YX.Yolox(input_size=64) for _ in range(4)], [shared] * 4):
        ts = [threading.Thread(target=work, args=(k, handles[k])) for k in range(4)]
        [t.start() for t in ts]
        [t.join() for t in ts]
    assert not errors, errors


def test_invalid_arguments(YX, h64):
    from eao_fusion_amd import _lib
    for kw in (dict(input_size=100), dict(input_size=0), dict(num_classes=0), dict(conf_thresh=-0.1), dict(max_proposals=0), dict(max_proposals=16385),
               dict(max_batch=0), dict(nms_thresh=float("nan"))):
        with pytest.raises(_lib.EaoError) as e:
            YX.Yolox(**kw)
        assert e.value.status == _lib.EAO_ERR_INVALID, kw
    s = SCENES["clusters"]

    def planted(b):
        return dict(objects=np.full((b, 8), -3, YX.OBJECT), n=np.full(b, -5, np.int32), n_proposals=np.full(b, -5, np.int32), n_tied=np.full(b, -5, np.int32))

    def untouched(o):
        return (o["objects"] == np.full(1, -3, YX.OBJECT)[0]).all() and all((o[k] == -5).all() for k in ("n", "n_proposals", "n_tied"))

    o = planted(1)
    assert h64.decode_raw(s["feat"], [(200, 1)], cap=8, out=o)["status"] == _lib.EAO_ERR_INVALID and untouched(o)        # no letterbox
    assert h64.decode_raw(s["feat"], [(0, 80)], cap=8, out=o)["status"] == _lib.EAO_ERR_INVALID and untouched(o)
    o5 = planted(5)
    assert h64.decode_raw(np.stack([s["feat"]] * 5), [(100, 80)] * 5, cap=8, out=o5)["status"] == _lib.EAO_ERR_INVALID and untouched(o5)   # max_batch = 4
    assert h64.decode_raw(s["feat"], [(100, 80)], cap=0, out=o)["status"] == _lib.EAO_ERR_INVALID and untouched(o)
    # fewer slots than objects: the counts, and no object
    r = h64.decode_raw(s["feat"], [(100, 80)], cap=2, out=planted(1))
    assert r["status"] == _lib.EAO_ERR_CAPACITY and r["n"].tolist() == [4] and (r["objects"][:, :2] == np.full(1, -3, YX.OBJECT)[0]).all()
    img = image(37, 23, 9)
    L = _lib.load()
    hd = h64._h
    assert L.eao_yolox_preprocess(hd, img.ctypes.data, 37, 23, 3 * 37 - 1, 0, 1, 0, None, 0) == _lib.EAO_ERR_INVALID      # stride below 3 * width
    assert L.eao_yolox_preprocess(hd, None, 37, 23, 111, 0, 1, 0, None, 0) == _lib.EAO_ERR_INVALID
    assert L.eao_yolox_preprocess(hd, img.ctypes.data, 37, 23, 111, 0, 9, 0, None, 0) == _lib.EAO_ERR_INVALID
    assert L.eao_yolox_preprocess_device(hd, 256, 37, 23, 111, 0, 1, 0, 256, 512, 100, None) == _lib.EAO_ERR_INVALID      # gray_stride no multiple of 64
    assert L.eao_yolox_preprocess_device(hd, 256, 37, 23, 111, 0, 1, 0, None, None, 0, None) == _lib.EAO_ERR_INVALID


def test_golden_files(h64, h640, oracle):
    for name, s in SCENES.items():
        if "max_proposals" in s:
            continue
        z = G.load(name)
        h = h640 if int(z["S"]) == 640 else h64
        got = h.decode(z["feat"], [tuple(int(v) for v in z["img"])])[0]
        assert Y.same_records(got["objects"].view(Y.OBJECT), z["objects"]) and got["n_tied"] == int(z["n_tied"]) and got["n_proposals"] == len(z["proposals"]), name
    z = G.load(G.FRAME)
    for rgb, key in ((False, "gray_bgr"), (True, "gray_rgb")):
        blob, gray = h64.preprocess(z["img"], rgb=rgb, want_gray=True)
        assert same_bits(blob[0], z["blob"]) and np.array_equal(gray[0], z[key])


def test_chain_frame_to_boxes(h64, oracle, want):
    """colour frame -> blob and grey on the device -> a stand-in network that copies a recorded head output into the handle's head buffer -> objects -> the
    BoxSE rows of Tracking::GrabImageRGBD, against the yardstick end to end"""
    import ctypes
    img = image(100, 80, 77)
    blob, gray = h64.preprocess(img, rgb=True, want_gray=True)
    eb, eg = expected_pre(oracle, img, 64, True)
    assert same_bits(blob[0], eb) and np.array_equal(gray[0], eg)
    d_blob, d_prob, stream = h64.buffers()
    s = SCENES["clusters"]
    back = np.zeros_like(eb)
    hip_memcpy(back.ctypes.data, d_blob, back.nbytes, 2)      # what the engine would read
    assert same_bits(back, eb)
    hip_memcpy(d_prob, s["feat"].ctypes.data, s["feat"].nbytes, 1)      # what it would write
    got = h64.decode_device(d_prob, 1, [(100, 80)], stream=stream)[0]
    check_frame(got, want["clusters"])
    boxes = Y.tracking_boxes(got["objects"].view(Y.OBJECT))
    assert Y.same_records(boxes, Y.tracking_boxes(want["clusters"]["objects"])) and len(boxes) >= 1
    assert (np.diff(boxes["prob"]) <= 0).all()


def test_adapter_tie_and_capacity_fallbacks_equal_the_literal_yardstick(tmp_path, want):
    """include/eaofusion/YOLOX.h on the device: the tie scene (n_tied > 0) and a frame beyond max_proposals come back as the LITERAL yardstick orders them"""
    exe = str(tmp_path / "yolox_adapter_gpu")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "yolox", "yolox_driver.cpp"),
                           os.path.join(ROOT, "tests", "cpp", "yolox", "yolox_upload_hip.cpp"), os.path.join(ROOT, "eao_fusion_amd", "libeaofusion_hip.so"), "-Wl,-rpath," + os.path.join(ROOT, "eao_fusion_amd"), "-Wl,-rpath,/opt/rocm/lib",
                           "-L/opt/rocm/lib", "-lamdhip64", "-lpthread", "-o", exe])
    for name, cap in (("tie", 4096), ("capacity_129", 128), ("clusters", 4096)):
        s = SCENES[name]
        text = "detect 64 %d %d %d %s\n" % (cap, s["img"][0], s["img"][1], G.hx(s["feat"]))
        out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr[-2000:]
        lines = out.stdout.strip().split("\n")
        lit = Y.decode_literal(s["feat"], 64, *s["img"])
        assert lines[:2] == ["frames 1 result 0", "frames 0 result 1 infer 1"] and lines[-1] == "result 0"
        assert lines[2] == "path %s" % ("device" if name == "clusters" else "literal")
        rows = ["%s %d" % (G.hx([o["x"], o["y"], o["w"], o["h"], o["prob"]]), o["label"]) for o in lit["objects"]]
        assert lines[3:-1] == ["objects %d" % len(rows)] + rows, name
