#!/usr/bin/env python3
"""Writes tests/golden/yolox/: per scene of tests/yolox_scenes.py the head output and what the yardstick (tests/yolox_reference.py) makes of it, and one small
frame with its blob and grey images.

    python tools/gen_golden_yolox.py            # writes the files
    python tools/gen_golden_yolox.py --check    # compares a fresh run with the files, writes nothing

Per scene <name>.npz: feat, S, img; objects / proposals / n_tied under the double-precision exponential and the device's tie rule (what the library returns);
objects_literal under the reference's own quicksort; expf_in / expf_out: the values of the generating machine's expf on the scene's exponents, recorded through
tools/yolox_walk.cpp (machine-dependent by nature: kept for the variant condition of tests/test_yolox_reference_cpu.py, never compared with a fresh run)."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import yolox_reference as Y  # noqa: E402
import yolox_scenes as SC  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "yolox")
FRAME = "frame_37x23"


def build_walk(path, flags=("-O2",)):
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", *flags, os.path.join(ROOT, "tools", "yolox_walk.cpp"), "-o", path])
    return path


def hx(a):
    return " ".join("%08x" % v for v in np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32))


def unhx(text):
    return np.array([int(t, 16) for t in text.split()], np.uint32).view(np.float32)


def walk_exp(walk, kind, xs):
    xs = np.ascontiguousarray(xs, np.float32).reshape(-1)
    out = subprocess.run([walk], input="exp %d %d %s\n" % (kind, len(xs), hx(xs)), capture_output=True, text=True, check=True).stdout
    return unhx(out)


def exponents(scene):
    return np.unique(scene["feat"][:, 2:4].reshape(-1).view(np.uint32)).view(np.float32)


def frame():
    """a 37 x 23 colour frame (down-scaled by 64 / 37 = 1.73 into 64 x 39) and what pre-processing makes of it at S = 64"""
    from oracle import oracle as O
    img = np.random.RandomState(3723).randint(0, 256, (23, 37, 3)).astype(np.uint8)
    canvas = Y.letterbox(img, 64, O.resize_linear)
    return dict(img=img, S=np.int32(64), blob=Y.blob_vectorised(canvas), gray_bgr=Y.gray(img, False), gray_rgb=Y.gray(img, True))


def scene_record(s):
    big = s["S"] > 64
    r = Y.decode_vectorised(s["feat"], s["S"], *s["img"])
    lit = r if big and r["n_tied"] == 0 else Y.decode_literal(s["feat"], s["S"], *s["img"])      # (without ties the two orders are one)
    return dict(feat=s["feat"], S=np.int32(s["S"]), img=np.array(s["img"], np.int32), objects=r["objects"], proposals=r["proposals"], n_tied=np.int32(r["n_tied"]),
                objects_literal=lit["objects"])


def load(name):
    z = np.load(os.path.join(OUT, name + ".npz"))
    return {k: z[k] for k in z.files}


def main():
    check = "--check" in sys.argv
    os.makedirs(OUT, exist_ok=True)
    bad = []
    with tempfile.TemporaryDirectory() as tmp:
        walk = None if check else build_walk(os.path.join(tmp, "yolox_walk"))
        todo = {name: scene_record(s) for name, s in SC.scenes().items()}
        if not check:
            for name, s in SC.scenes().items():
                xs = exponents(s)
                todo[name]["expf_in"], todo[name]["expf_out"] = xs, walk_exp(walk, 1, xs)
        todo[FRAME] = frame()
        for name, rec in todo.items():
            if check:
                have = load(name)
                bad += [name + "." + k for k, v in rec.items() if not (np.asarray(v).dtype == have[k].dtype and np.asarray(v).tobytes() == have[k].tobytes())]
            else:
                np.savez_compressed(os.path.join(OUT, name + ".npz"), **rec)
                print("wrote", name)
    if bad:
        raise SystemExit("differs from a fresh run: " + ", ".join(bad))


if __name__ == "__main__":
    main()
