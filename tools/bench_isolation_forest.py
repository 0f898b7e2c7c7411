"""Object_Map::IsolationForestDeleteOutliers on the device against the host: the time of one eao_object_iforest_outliers_batch call for one object of N = 30,
200, 1000 and 4000 points and for a batch of 16 objects of 500 points, against the same forests built and scored on one host thread in the same run
(tools/isolation_forest_walk.cpp: the library's own host header in the kernel's sort-free form, built -O3 -ffp-contract=off where this runs).

Gaussian clouds with planted far points (tests/isolation_forest_scenes.py).  Per shape: host wall clock around the C entry point (ctypes, arrays packed
beforehand; the call ends in the stream's wait), the HIP-event times of k_iforest_build and k_iforest_score, and inside k_iforest_build the mean over the trees
of seeding the generator, of the shuffle with the copy of the sample, and of the depth-first walk (the device's constant clock).  Median (min .. max) of --reps
calls behind --warmup.  A record only: nothing is gated.

    python tools/bench_isolation_forest.py [--reps 100] [--warmup 10] [--out profiles/isolation_forest_timing.txt]
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

import isolation_forest_scenes as SC  # noqa: E402
from eao_fusion_amd import isolation_forest as IF  # noqa: E402

SINGLE = (30, 200, 1000, 4000)
BATCH = (16, 500)


def spread(v):
    v = np.asarray(v)
    return "%9.1f (%.1f .. %.1f)" % (np.median(v), v.min(), v.max())


def device(objects, reps, warmup):
    cls = [0] * len(objects)
    IF.set_profiling(False)
    for _ in range(warmup):
        IF.outliers_batch(objects, cls)
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        IF.outliers_batch(objects, cls)
        wall.append((time.perf_counter() - t0) * 1e6)
    IF.set_profiling(True)
    build, score, stages = [], [], []
    for _ in range(max(reps // 4, 5)):
        IF.outliers_batch(objects, cls)
        b, s = IF.last_kernel_ms()
        build.append(b * 1e3)
        score.append(s * 1e3)
        stages.append(IF.last_stage_us())
    IF.set_profiling(False)
    return wall, build, score, np.median(np.array(stages), axis=0)


def host(exe, objects, repeats):
    total = 0.0
    for p in objects:
        line = "time %d %d %d %d %d %s\n" % (repeats, SC.TREE_COUNT, SC.SEED, len(p) // 2, len(p), " ".join("%08x" % v for v in p.reshape(-1).view(np.uint32)))
        out = subprocess.run([exe], input=line, capture_output=True, text=True, check=True).stdout.split()
        assert out[0] == "time_us"
        total += float(out[1])
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "isolation_forest_timing.txt"))
    a = ap.parse_args()
    lines = ["# tools/bench_isolation_forest.py --reps %d --warmup %d: microseconds, median (min .. max); the forest of Object_Map::IsolationForestDeleteOutliers "
             "(50 trees, seed 12345, N / 2)" % (a.reps, a.warmup),
             "# device: host wall clock around eao_object_iforest_outliers_batch (ends in the stream's wait), HIP events per kernel, and inside k_iforest_build the mean "
             "per tree of its three stages",
             "# host: tools/isolation_forest_walk.cpp, one thread, -O3 -ffp-contract=off, built and run on the same machine in the same run"]
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "isolation_forest_walk")
        subprocess.check_call(["g++", "-O3", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tools", "isolation_forest_walk.cpp"), "-o", exe])
        shapes = [("one object, N = %d" % n, [SC._cloud(n, 900 + n)]) for n in SINGLE]
        shapes.append(("batch: %d objects of %d points, one call" % BATCH, [SC._cloud(BATCH[1], 950 + k) for k in range(BATCH[0])]))
        for title, objects in shapes:
            wall, build, score, stages = device(objects, a.reps, a.warmup)
            h = host(exe, objects, max(3, min(50, 20000 // len(objects[0]))))
            lines.append("%s" % title)
            lines.append("    device, wall clock of the call            %s us" % spread(wall))
            lines.append("    device, k_iforest_build (HIP events)      %s us" % spread(build))
            lines.append("    device, k_iforest_score (HIP events)      %s us" % spread(score))
            lines.append("    inside k_iforest_build, mean per tree     seeding %.1f us, shuffle and sample %.1f us, walk %.1f us" % tuple(stages))
            lines.append("    host walk, one thread                     %9.1f us%s" % (h, "" if len(objects) == 1 else " (the objects one after another)"))
            lines.append("    host / device wall clock                  %9.2f" % (h / np.median(wall)))
        if len(shapes[-1][1]) > 1:
            objects = shapes[-1][1]
            IF.set_profiling(False)
            singles = []
            for _ in range(max(a.reps // 4, 5)):
                t0 = time.perf_counter()
                for p in objects:
                    IF.outliers_batch([p], [0])
                singles.append((time.perf_counter() - t0) * 1e6)
            lines.append("    device, %d single calls                   %s us" % (len(objects), spread(singles)))
    lines.append("# The CPU figures quoted when this work was proposed (0.44 ms at 30 points, 1.6 ms at 200, 9.8 ms at 1000, 54 ms at 4000) came from the reference's "
                 "own header built -O2 in a scratch driver on a CPU-only development machine, not on the GPU host; the host lines above are this run's yardstick.")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
