"""The class surface include/eaofusion/YOLOX.h without a device: tests/cpp/yolox/yolox_driver.cpp over a stand-in cv::Mat, linked with yolox_stub.cpp, which prints
the library call it receives and answers by script.  Checked: the call order of Detect (pre-processing, the network on the handle's buffers and stream, the
decode), the device's answer passed on when n_tied == 0, the host's literal decode taken exactly when n_tied > 0 or the library reports EAO_ERR_CAPACITY (and equal
to the yardstick's literal form), a refused frame leaving no result, the queue surface with Run() on a thread, and the filter of Tracking::GrabImageRGBD."""
import os
import subprocess

import numpy as np
import pytest

import yolox_reference as Y
import yolox_scenes as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = SC.scenes()
EAO_ERR_INVALID, EAO_ERR_CAPACITY = -1, -3
STUB_OBJECTS = ["objects 2", "3f800000 40000000 40400000 40800000 3f666666 7", "40a00000 40c00000 40e00000 41000000 3f4ccccd 9"]


def hx(a):
    return " ".join("%08x" % v for v in np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("yolox") / "yolox_surface")
    src = os.path.join(ROOT, "tests", "cpp", "yolox")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-DYOLOX_STUB", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "include"), os.path.join(src, "yolox_driver.cpp"), os.path.join(src, "yolox_stub.cpp"), "-pthread", "-o", path])
    return path


def run(exe, text):
    out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    return out.stdout.strip().split("\n")


def detect(scene, cap=4096):
    s = SCENES[scene]
    return "detect 64 %d %d %d %s\n" % (cap, s["img"][0], s["img"][1], hx(s["feat"]))


def literal_rows(scene):
    s = SCENES[scene]
    o = Y.decode_literal(s["feat"], 64, *s["img"])["objects"]
    return ["objects %d" % len(o)] + ["%s %d" % (hx([r["x"], r["y"], r["w"], r["h"], r["prob"]]), r["label"]) for r in o]


def test_call_order_and_the_device_answer(exe):
    got = run(exe, "script 0 0 6\n" + detect("clusters"))
    assert got[0] == "call create S 64 classes 80 max_proposals 4096 max_batch 1"
    assert got[1] == "frames 1 result 0"
    assert got[2].startswith("call preprocess 100 x 80 stride 300 batch 1 rgb 0 gray 0 first ")
    assert got[3] == "call decode_device own_buffer 1 batch 1 img 100 x 80 cap 4096 stream 1"
    assert got[4] == "frames 0 result 1 infer 1"
    assert got[5] == "path device" and got[6:9] == STUB_OBJECTS and got[9] == "result 0" and got[10] == "call destroy"
    assert not [ln for ln in got if ln.startswith("call head")]


@pytest.mark.parametrize("scene", ["tie", "clusters", "zero_area"])
def test_a_tie_takes_the_literal_decode(exe, scene):
    got = run(exe, "script 3 0 9\n" + detect(scene))
    calls = [ln.split()[1] for ln in got if ln.startswith("call")]
    assert calls == ["create", "preprocess", "decode_device", "head", "destroy"]
    at = got.index("path literal")
    rows = literal_rows(scene)
    assert got[at + 1:at + 1 + len(rows)] == rows


def test_an_overflow_takes_the_literal_decode(exe):
    got = run(exe, "script 0 %d 129\n" % EAO_ERR_CAPACITY + detect("capacity_129", cap=128))
    assert [ln.split()[1] for ln in got if ln.startswith("call")] == ["create", "preprocess", "decode_device", "head", "destroy"]
    at = got.index("path literal")
    rows = literal_rows("capacity_129")
    assert got[at + 1:at + 1 + len(rows)] == rows and rows[0] == "objects 1"


def test_refusals_leave_no_result(exe):
    got = run(exe, "script 0 %d 0\n" % EAO_ERR_INVALID + detect("clusters"))
    assert "no result" in got and not [ln for ln in got if ln.startswith("call head") or ln.startswith("path")]
    s = SCENES["clusters"]
    got = run(exe, "script 0 0 6\ndetect 64 4096 1000 80 %s\n" % hx(s["feat"]))      # the stub refuses frames 1000 wide: no network call, no decode
    assert "frames 0 result 0 infer 0" in got and "no result" in got and not [ln for ln in got if ln.startswith("call decode")]


def test_queue_surface(exe):
    s = SCENES["one"]
    got = run(exe, "script 0 0 1\nqueue 64 100 80 %s\n" % hx(s["feat"]))
    assert "finished 1 infer 1 frames 0 objects 2" in got      # two frames inserted, one detection: Detect clears the queue


def test_tracking_boxes(exe):
    rows = [(0.5, 0, 1.5, 2.5, 3.5, 4.5), (0.49999, 0, 1, 1, 1, 1), (0.9, 1, 1, 1, 1, 1), (0.7, 73, 10.9, 11.2, 12.7, 13.1), (0.8, 62, 5, 6, 7, 8)]
    text = "boxes %d %s\n" % (len(rows), " ".join("%s %d %s" % (hx([p]), c, hx([x, y, w, h])) for p, c, x, y, w, h in rows))
    got = run(exe, text)
    want = Y.tracking_boxes(Y.records([(x, y, w, h, p, c) for p, c, x, y, w, h in rows]))
    assert got == ["box %d %s %d %d %d %d" % (o["label"], hx([o["prob"]]), int(o["x"]), int(o["y"]), int(o["w"]), int(o["h"])) for o in want] + ["end"]
    assert [ln.split()[1] for ln in got[:-1]] == ["62", "73", "0"]
