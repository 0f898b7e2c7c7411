"""A map object's cuboid on the device against the host: eao_object_cuboids over one object of 30, 300 and 3000 points, eao_object_cuboids_batch over a frame's 8
objects and over a map of 64 objects (300 points each), and eao_object_overlaps over the 64 records -- against tools/object_cuboid_walk.cpp, upstream's literal
form (push_back, sort, the early returns), built -O3 -ffp-contract=off where this runs, on one thread, over the same objects.

Per shape: host wall clock around the C entry point (ctypes, descriptors packed beforehand; the call ends in the stream's wait and holds the upload and the
download) and, in separate calls, the HIP-event time of the kernel.  Median (min .. max) of --reps calls behind --warmup.  Before anything is timed the device's
records are held to the walk program's on every object.  A record only: nothing is gated.

    python tools/bench_object_cuboid.py [--reps 200] [--warmup 20] [--out profiles/object_cuboid_timing.txt]
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

import object_cuboid_reference as Y  # noqa: E402
import object_cuboid_scenes as SC  # noqa: E402
from eao_fusion_amd import _lib  # noqa: E402
from eao_fusion_amd import object_cuboid as OC  # noqa: E402


def spread(v):
    v = np.asarray(v)
    return "%9.1f (%.1f .. %.1f)" % (np.median(v), v.min(), v.max())


def timing_object(n, m, seed):
    rng = np.random.default_rng(seed)
    return SC.obj(SC.cloud(rng, n, centre=rng.uniform(-3, 3, 3)), SC.cloud(rng, m, spread=(0.05, 0.05, 0.05)), Y.ryaw(0, 0, 0.1 * (seed % 7)), prev=(0.4, -0.2, 2.1))


def time_cuboids(objs, single, reps, warmup):
    keep, descs = OC._descs(objs)
    rec = np.zeros(len(objs), OC.RECORD_DTYPE)
    L = _lib.load()

    def call():
        _lib.check(L.eao_object_cuboids(descs, _lib.ptr(rec)) if single else L.eao_object_cuboids_batch(len(objs), descs, _lib.ptr(rec)))

    OC.set_profiling(False)
    for _ in range(warmup):
        call()
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e6)
    OC.set_profiling(True)
    kern = []
    for _ in range(max(reps // 4, 5)):
        call()
        kern.append(OC.last_kernel_ms()[0] * 1e3)
    OC.set_profiling(False)
    return wall, kern, rec.copy()


def time_overlaps(rows, eligible, reps, warmup):
    M = len(rows)
    verdict, extents = np.zeros(M * M, np.uint8), np.zeros(M * M * 3, np.float32)
    L = _lib.load()

    def call():
        _lib.check(L.eao_object_overlaps(M, _lib.ptr(rows), _lib.ptr(eligible), _lib.ptr(verdict), _lib.ptr(extents)))

    OC.set_profiling(False)
    for _ in range(warmup):
        call()
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e6)
    OC.set_profiling(True)
    kern = []
    for _ in range(max(reps // 4, 5)):
        call()
        kern.append(OC.last_kernel_ms()[1] * 1e3)
    OC.set_profiling(False)
    return wall, kern, verdict.reshape(M, M).copy(), extents.reshape(M, M, 3).copy()


def host(exe, objs, reps):
    script = "".join(Y.walk_script(o, "load") for o in objs) + "time %d\n" % reps
    out = subprocess.run([exe], input=script, capture_output=True, text=True, check=True).stdout.split()
    assert out[0] == "time"
    return float(out[1])


def hold_to_the_walk(exe, objs, recs):
    """the device's record of every object against the literal walk (the signs of the zeros the sorts decide aside)"""
    out = subprocess.run([exe], input="".join(Y.walk_script(o) for o in objs), capture_output=True, text=True, check=True).stdout.strip().split("\n")
    for o, line, rec in zip(objs, out, recs):
        drop = Y.zero_sign_fields(o)
        if Y.drop_line(line, drop) != Y.walk_line(rec, drop):
            raise SystemExit("the device and the host walk disagree on an object")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "object_cuboid_timing.txt"))
    a = ap.parse_args()
    props = torch.cuda.get_device_properties(0)
    lines = ["# tools/bench_object_cuboid.py --reps %d --warmup %d on %s (%s, %d compute units): microseconds, median (min .. max); "
             "Object_Map::ComputeMeanAndStandard with UpdateObjPose (src/Object.cc:999-1235, :2243-2303); 3 centroids per object" % (
                 a.reps, a.warmup, props.name, getattr(props, "gcnArchName", "?"), props.multi_processor_count),
             "# device: host wall clock around the entry point (ends in the stream's wait; it holds the upload and the download); HIP events around the kernel, in "
             "separate calls",
             "# host: tools/object_cuboid_walk.cpp (upstream's literal form: push_back, sort, the early returns), one thread, -O3 -ffp-contract=off, built and run on "
             "the same machine in the same run over the same objects; every object's device record was held to it first"]
    shapes = [("1 object of 30 points, eao_object_cuboids", [timing_object(30, 3, 1)], True), ("1 object of 300 points, eao_object_cuboids", [timing_object(300, 3, 2)], True),
              ("1 object of 3000 points, eao_object_cuboids", [timing_object(3000, 3, 3)], True),
              ("a frame's 8 objects of 300 points, one eao_object_cuboids_batch call", [timing_object(300, 3, 10 + k) for k in range(8)], False),
              ("a map of 64 objects of 300 points, one eao_object_cuboids_batch call", [timing_object(300, 3, 100 + k) for k in range(64)], False)]
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "object_cuboid_walk")
        subprocess.check_call(["g++", "-O3", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tools", "object_cuboid_walk.cpp"), "-o", exe])
        recs = None
        for title, objs, single in shapes:
            wall, kern, recs = time_cuboids(objs, single, a.reps, a.warmup)
            hold_to_the_walk(exe, objs, recs)
            h = host(exe, objs, 200)
            lines.append(title)
            lines.append("    device, wall clock of the call            %s us" % spread(wall))
            lines.append("    device, k_object_cuboids (HIP events)     %s us" % spread(kern))
            lines.append("    host, upstream's form, one thread         %9.1f us" % h)
            lines.append("    host / device wall                        %9.2f" % (h / np.median(wall)))
        rows, eligible = OC.rows_of(recs), np.ones(len(recs), np.uint8)
        wall, kern, verdict, extents = time_overlaps(rows, eligible, a.reps, a.warmup)
        wv, we = Y.overlaps_vectorised(rows, eligible)
        if not (np.array_equal(verdict, wv) and np.array_equal(extents[wv == 1].view(np.uint32), we[wv == 1].view(np.uint32))):
            raise SystemExit("the device and the yardstick disagree on the overlap matrix")
        lines.append("the overlap matrix of the map's 64 records, eao_object_overlaps with extents")
        lines.append("    device, wall clock of the call            %s us" % spread(wall))
        lines.append("    device, k_object_overlaps (HIP events)    %s us" % spread(kern))
        lines.append("    verdicts set %d of %d" % (int(verdict.sum()), verdict.size))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
