"""A frame's 2D objects on the device against the host: eao_frame_objects over one frame of 1500 keypoints x 16 boxes (the shape of a tracked TUM frame with a
full detector output) and eao_frame_objects_batch over 64 such frames in one call (offline replay), against tools/frame_objects_walk.cpp -- upstream's literal
form: push_back, sort, erase -- built -O3 -ffp-contract=off where this runs, on one thread, over the same frames.

Per shape: host wall clock around the C entry point (ctypes, arrays packed beforehand; the call ends in the stream's waits and holds the upload, the two downloads
and the host's second loop of step 6) and the HIP-event times of the three kernels.  Median (min .. max) of --reps calls behind --warmup.  Before anything is timed
the device's records are held to the walk program's on every frame.  A record only: nothing is gated.

    python tools/bench_frame_objects.py [--reps 200] [--warmup 20] [--out profiles/frame_objects_timing.txt]
"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402,F401  (first: both runtimes resolve the same libamdhip64)

import frame_objects_reference as Y  # noqa: E402
import frame_objects_scenes as SC  # noqa: E402
from eao_fusion_amd import _lib  # noqa: E402
from eao_fusion_amd import frame_objects as FO  # noqa: E402

N_BATCH = 64


def spread(v):
    v = np.asarray(v)
    return "%9.1f (%.1f .. %.1f)" % (np.median(v), v.min(), v.max())


def time_call(frames, single, reps, warmup):
    keep, descs = FO._descs(frames)
    nB = sum(len(k[4]) for k in keep)
    worst = sum(len(k[4]) * int((k[2] >= 0).sum()) for k in keep)
    rec = np.zeros(nB, FO.RECORD_DTYPE)
    sa, sk, la, lk = np.zeros(nB + 1, np.int32), np.zeros(nB + 1, np.int32), np.zeros(worst, np.int32), np.zeros(worst, np.int32)
    out = _lib.FrameObjectsOut(_lib.ptr(rec), _lib.ptr(sa), _lib.ptr(la), worst, _lib.ptr(sk), _lib.ptr(lk), worst)
    L = _lib.load()

    def call():
        _lib.check(L.eao_frame_objects(descs, C.byref(out)) if single else L.eao_frame_objects_batch(len(frames), descs, C.byref(out)))

    FO.set_profiling(False)
    for _ in range(warmup):
        call()
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e6)
    FO.set_profiling(True)
    kern = []
    for _ in range(max(reps // 4, 5)):
        call()
        kern.append([m * 1e3 for m in FO.last_kernel_ms()])
    FO.set_profiling(False)
    return wall, np.array(kern), dict(records=rec.copy(), sa=sa.copy(), la=la.copy(), sk=sk.copy(), lk=lk.copy())


def host(exe, frames, reps):
    script = "".join("load" + Y.walk_script(fr)[len("frame"):] for fr in frames) + "time %d\n" % reps
    out = subprocess.run([exe], input=script, capture_output=True, text=True, check=True).stdout.split()
    assert out[0] == "time"
    return float(out[1])


def hold_to_the_walk(exe, frames, got):
    """the device's result of every frame against the literal walk (zero signs of the quartiles aside)"""
    out = subprocess.run([exe], input="".join(Y.walk_script(fr) for fr in frames), capture_output=True, text=True, check=True).stdout.strip().split("\n")
    b, at = 0, 0
    for fr in frames:
        m = len(fr["boxes"])
        res = dict(records=got["records"][b:b + m], assigned=[got["la"][got["sa"][k]:got["sa"][k + 1]] for k in range(b, b + m)],
                   kept=[got["lk"][got["sk"][k]:got["sk"][k + 1]] for k in range(b, b + m)])
        mine = Y.walk_lines(res, zero_signs=False)
        theirs = []
        for l in out[at:at + len(mine)]:
            t = l.split()
            if t[0] == "rec":
                for c in (21, 22, 23):
                    t[c] = "00000000" if t[c] == "80000000" else t[c]
            theirs.append(" ".join(t))
        if mine != theirs:
            raise SystemExit("the device and the host walk disagree on a frame")
        b += m
        at += len(mine)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_objects_timing.txt"))
    a = ap.parse_args()
    frames = [SC.timing_frame(100 + f) for f in range(N_BATCH)]
    lines = ["# tools/bench_frame_objects.py --reps %d --warmup %d: microseconds, median (min .. max); steps 2, 4, 5 and 6 of the object layer "
             "(src/Tracking.cc:1768-1973) for frames of 1500 keypoints (nine in ten with a map point) and 16 boxes" % (a.reps, a.warmup),
             "# device: host wall clock around the entry point (ends in the stream's waits; it holds the upload, both downloads and the host's second loop of "
             "step 6), HIP events around each kernel",
             "# host: tools/frame_objects_walk.cpp (upstream's literal form: push_back, sort, erase), one thread, -O3 -ffp-contract=off, built and run on the same "
             "machine in the same run over the same frames; every frame's device result was held to it first"]
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "frame_objects_walk")
        subprocess.check_call(["g++", "-O3", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tools", "frame_objects_walk.cpp"), "-o", exe])
        for title, fs, single in (("1 frame, eao_frame_objects", frames[:1], True), ("%d frames, one eao_frame_objects_batch call" % N_BATCH, frames, False)):
            wall, kern, got = time_call(fs, single, a.reps if single else max(a.reps // 4, 10), a.warmup)
            hold_to_the_walk(exe, fs, got)
            h = host(exe, fs, 200 if single else 10)
            n_a, n_k = int(got["sa"][-1]), int(got["sk"][-1])
            lines.append(title)
            lines.append("    device, wall clock of the call            %s us" % spread(wall))
            for k, name in enumerate(("k_frame_features", "k_frame_objects ", "k_frame_pack    ")):
                lines.append("    device, %s (HIP events)        %s us" % (name, spread(kern[:, k])))
            lines.append("    host, upstream's form, one thread         %9.1f us" % h)
            lines.append("    host / device wall                        %9.2f" % (h / np.median(wall)))
            lines.append("    boxes %d, list entries after step 2 / after the boxplot %d / %d, bad boxes %d" % (len(got["records"]), n_a, n_k, int(got["records"]["bad"].sum())))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
