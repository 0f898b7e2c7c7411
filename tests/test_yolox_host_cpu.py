"""The host header of the yolox feature (eao_fusion_amd/csrc/yolox_internal.h) without a device: tools/yolox_walk.cpp is built with
g++ -fsanitize=address,undefined and run as a program of its own.  On every scene it must print what the yardstick (tests/yolox_reference.py) computes, under the
reference's own order and under the device's tie rule; its pre-processing must give the yardstick's blob and grey images; and yolox_exp_f32 must equal
(float)exp((double)x) on a seeded sample of 10^6 floats and on every exponent of every scene."""
import os
import subprocess

import numpy as np
import pytest

import yolox_reference as Y
import yolox_scenes as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = SC.scenes()


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("yolox") / "yolox_walk")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tools", "yolox_walk.cpp"), "-o", exe])
    return exe


def hx(a):
    return " ".join("%08x" % v for v in np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32))


def run_walk(walk, script):
    out = subprocess.run([walk], input=script, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, "exit %d\n%s" % (out.returncode, out.stderr[-3000:])
    return out.stdout.strip().split("\n")


def rows(o):
    return ["%s %d" % (hx([r["x"], r["y"], r["w"], r["h"], r["prob"]]), r["label"]) for r in o]


@pytest.mark.parametrize("stable", [0, 1])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_decode_scene(walk, name, stable):
    s = SCENES[name]
    got = run_walk(walk, "decode %d 80 %s %s %d %d %d 0 %s\n" % (s["S"], hx([Y.CONF]), hx([Y.NMS]), s["img"][0], s["img"][1], stable, hx(s["feat"])))
    if s["S"] > 64:      # (no ties in it: one order; the vectorised form is the quick one)
        w = Y.decode_vectorised(s["feat"], s["S"], *s["img"])
    else:
        w = Y.decode_literal(s["feat"], s["S"], *s["img"], stable=bool(stable))
    n = len(w["proposals"])
    assert got[0] == "n_proposals %d" % n and got[1] == "n_tied %d" % w["n_tied"]
    assert got[2] == "proposals %d" % n and got[3:3 + n] == rows(w["proposals"])
    assert got[3 + n] == "objects %d" % len(w["objects"]) and got[4 + n:] == rows(w["objects"])


def test_exp_is_the_double_exponential_rounded_once(walk):
    got = run_walk(walk, "sample 20261020 1000000\n")
    assert got[0] == "differs_from_double 0"
    xs = np.unique(np.concatenate([s["feat"][:, 2:4].reshape(-1) for s in SCENES.values()] + [np.float32([-104.5, -103.9, -87.4, 0, 88.7, 88.8, 89.5, 710, np.inf, -np.inf])]))
    ours, dbl = (run_walk(walk, "exp %d %d %s\n" % (kind, len(xs), hx(xs)))[0] for kind in (0, 2))
    assert ours == dbl == hx([Y.exp_double(x) for x in xs])
    nan = run_walk(walk, "exp 0 1 7fc00000\n")[0]
    assert int(nan, 16) & 0x7fffffff > 0x7f800000


def test_geometry(walk):
    got = run_walk(walk, "geometry 1064 20 640\ngeometry 848 480 640\ngeometry 100 700 640\ngeometry 5000 1 640\ngeometry 640 480 640\n")
    assert [g.split()[0] for g in got] == ["1", "1", "1", "0", "1"]
    assert [tuple(g.split()[2:]) for g in got] == [("639", "12"), ("640", "362"), ("91", "640"), ("0", "0"), ("640", "480")]
    assert got[0].split()[1] == hx([Y.geometry(1064, 20, 640)[0]])


@pytest.mark.parametrize("w,h,rgb", [(37, 23, 0), (64, 48, 1), (128, 40, 0), (32, 24, 1), (9, 150, 0)])
def test_preprocess(walk, oracle, w, h, rgb):
    """a down-scale, the identity, the exact halving, x 2 up (row offset -1), a tall frame"""
    img = np.random.RandomState(300 + w).randint(0, 256, (h, w, 3)).astype(np.uint8)
    got = run_walk(walk, "pre %d %d 64 %d %s\n" % (w, h, rgb, " ".join("%02x" % v for v in img.reshape(-1))))
    blob = Y.blob_vectorised(Y.letterbox(img, 64, oracle.resize_linear))
    assert got[0] == hx(blob)
    assert got[1] == " ".join("%02x" % v for v in Y.gray(img, bool(rgb)).reshape(-1))
