"""The update of a map object's point list on the device against the host: eao_object_points_update over one DataAssociateUpdate (change gate, RADIUS append,
erase by projection) of 50, 500 and 2000 list points, eao_object_points_update_batch over a frame's 10 associated objects (50 .. 2000 list points, 20 .. 200
candidates), and one MergeTwoMapObjs append of 2000 x 2000 -- against tools/object_points_walk.cpp, upstream's literal form (the growing list, the `break`, the
erase while iterating) WITHOUT its cv::Mat clones and its mutex, built -O3 -ffp-contract=off where this runs, on one thread, over the same descs: the host
figure flatters the host.

Per shape: host wall clock around the C entry point (ctypes, descriptors packed beforehand; the call ends in the stream's wait and holds the upload and the
download) and, in separate calls, the HIP-event time of the kernel.  Median (min .. max) of --reps calls behind --warmup.  Before anything is timed the device's
outputs are held to the walk program's on every desc.  A record only: nothing is gated.

    python tools/bench_object_points.py [--reps 200] [--warmup 20] [--out profiles/object_points_timing.txt]
"""
import argparse
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

import object_points_reference as Y  # noqa: E402
import object_points_scenes as SC  # noqa: E402
from eao_fusion_amd import _lib  # noqa: E402
from eao_fusion_amd import object_points as OP  # noqa: E402


def spread(v):
    v = np.asarray(v)
    return "%9.1f (%.1f .. %.1f)" % (np.median(v), v.min(), v.max())


def time_update(descs, single, reps, warmup):
    keep, cd, co = OP._descs(descs, 0, True)
    L = _lib.load()

    def call():
        _lib.check(L.eao_object_points_update(cd, co) if single else L.eao_object_points_update_batch(len(descs), cd, co))

    OP.set_profiling(False)
    for _ in range(warmup):
        call()
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e6)
    OP.set_profiling(True)
    kern = []
    for _ in range(max(reps // 4, 5)):
        call()
        kern.append(sum(ms for ms in OP.last_kernel_ms() if ms >= 0) * 1e3)
    OP.set_profiling(False)
    return wall, kern, [OP.trim(d, k[4]) for d, k in zip(descs, keep)]


def host(exe, descs, reps):
    script = "".join(Y.walk_script(d, "load") for d in descs) + "time %d\n" % reps
    out = subprocess.run([exe], input=script, capture_output=True, text=True, check=True).stdout.split()
    assert out[0] == "time"
    return float(out[1])


def hold_to_the_walk(exe, descs, results):
    out = subprocess.run([exe], input="".join(Y.walk_script(d) for d in descs), capture_output=True, text=True, check=True).stdout.strip().split("\n")
    for line, res in zip(out, results):
        if line.split() != Y.walk_line(res).split():
            raise SystemExit("the device and the host walk disagree on a desc")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "object_points_timing.txt"))
    a = ap.parse_args()
    props = torch.cuda.get_device_properties(0)
    lines = ["# tools/bench_object_points.py --reps %d --warmup %d on %s (%s, %d compute units): microseconds, median (min .. max); the point-list update of "
             "Object_Map::DataAssociateUpdate (src/Object.cc:1364-1589) and MergeTwoMapObjs (:1766-1821)" % (
                 a.reps, a.warmup, props.name, getattr(props, "gcnArchName", "?"), props.multi_processor_count),
             "# device: host wall clock around the entry point (ends in the stream's wait; it holds the upload and the download); HIP events around the kernel(s), in "
             "separate calls",
             "# host: tools/object_points_walk.cpp (upstream's literal form without its cv::Mat clones and its mutex: it flatters the host), one thread, -O3 "
             "-ffp-contract=off, built and run on the same machine in the same run over the same descs; every desc's device outputs were held to it first"]
    rng = np.random.default_rng(2024)
    frame = [SC.frame_update(rng, M, C, repeats=C // 2) for M, C in ((50, 20), (120, 40), (200, 60), (350, 80), (500, 100), (700, 120), (900, 140), (1200, 160), (1600, 180),
                                                                     (2000, 200))]
    mp = SC.cloud(rng, 2000, (0, 0, 0))
    merge = SC.scene(mp, np.concatenate([mp[rng.choice(2000, 800, replace=False)], SC.cloud(rng, 1200, (0, 0, 0), (0.5, 0.5, 0.5))]), gate=Y.GATE_CUBOID, lenth=1.5, width=1.2,
                     height=1.8, sum_pos=mp.sum(axis=0), cand_count=np.zeros(2000, np.int32))
    shapes = [("1 update of 50 list points x 20 candidates, eao_object_points_update", [frame[0]], True),
              ("1 update of 500 list points x 100 candidates, eao_object_points_update", [frame[4]], True),
              ("1 update of 2000 list points x 200 candidates, eao_object_points_update", [frame[9]], True),
              ("a frame's 10 updates (50 .. 2000 list points, 20 .. 200 candidates), one eao_object_points_update_batch call", frame, False),
              ("1 merge of 2000 list points x 2000 candidates (CUBOID gate, no erase), eao_object_points_update", [merge], True)]
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "object_points_walk")
        subprocess.check_call(["g++", "-O3", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tools", "object_points_walk.cpp"), "-o", exe])
        for title, descs, single in shapes:
            wall, kern, results = time_update(descs, single, a.reps, a.warmup)
            hold_to_the_walk(exe, descs, results)
            h = host(exe, descs, 200)
            lines.append(title)
            lines.append("    device, wall clock of the call            %s us" % spread(wall))
            lines.append("    device, the kernel(s) (HIP events)        %s us" % spread(kern))
            lines.append("    host, upstream's form, one thread         %9.1f us" % h)
            lines.append("    host / device wall                        %9.2f" % (h / np.median(wall)))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
