"""include/eaofusion/YOLOXNet.h without a device: tests/cpp/detnet/detnet_driver.cpp linked with the recording stubs (tests/cpp/yolox/yolox_stub.cpp and
tests/cpp/detnet/detnet_stub.cpp).  Checked: the constructor takes the engine file path and nothing else it needs, the network is made before the detector and
destroyed after it, Detect runs pre-processing, the network on the handle's buffers and stream, and the decode, in that order; a refused file, a model with
another class count and a refused forward are errors, not stale results."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("detnet") / "detnet_surface")
    cpp = os.path.join(ROOT, "tests", "cpp")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                           os.path.join(ROOT, "include"), os.path.join(cpp, "detnet", "detnet_driver.cpp"), os.path.join(cpp, "detnet", "detnet_stub.cpp"),
                           os.path.join(cpp, "yolox", "yolox_stub.cpp"), "-pthread", "-o", path])
    return path


def run(exe, tmp_path, env=None, width=100):
    frame = tmp_path / "frame.bin"
    frame.write_bytes(bytes([9]) * (width * 80 * 3))
    out = subprocess.run([exe, "/some/where/yolox_s.detnet", "64", "4096", str(width), "80", str(frame)], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, **(env or {})))
    assert out.returncode == 0 and out.stderr == "", out.stdout[-2000:] + out.stderr[-3000:]
    return out.stdout.strip().split("\n")


def test_constructor_and_call_order(exe, tmp_path):
    got = run(exe, tmp_path)
    assert got == ["call detnet_create_from_file yolox_s.detnet S 64 max_batch 1",
                   "call create S 64 classes 80 max_proposals 4096 max_batch 1",
                   "engine classes 80 anchors 84",
                   "call preprocess 100 x 80 stride 300 batch 1 rgb 0 gray 0 first 9",
                   "call detnet_forward blob 1 prob 1 batch 1 stream 1",
                   "call decode_device own_buffer 1 batch 1 img 100 x 80 cap 4096 stream 1",
                   "result 1 path 1", "objects 2", "3f800000 40000000 40400000 40800000 3f666666 7", "40a00000 40c00000 40e00000 41000000 3f4ccccd 9",
                   "call destroy", "call detnet_destroy"]


def test_refusals_are_errors(exe, tmp_path):
    got = run(exe, tmp_path, {"DETNET_STUB_REFUSE": "1"})
    assert got[0].startswith("call detnet_create_from_file") and got[1].startswith("error: eao_detnet_create_from_file") and len(got) == 2
    got = run(exe, tmp_path, {"DETNET_STUB_CLASSES": "3"})
    assert got[-2] == "call detnet_destroy" and got[-1] == "error: the model has 3 classes, the detector is configured for 80" and not [g for g in got if g.startswith("call create")]
    got = run(exe, tmp_path, {"DETNET_STUB_FORWARD": "1"})
    assert got[-1].startswith("error: eao_detnet_forward") and not [g for g in got if g.startswith("call decode") or g.startswith("objects")]
    got = run(exe, tmp_path, width=1000)      # the stub refuses frames 1000 wide: no network call, no result
    assert "result 0 path 0" in got and not [g for g in got if g.startswith("call detnet_forward")]
