"""The object layer's per-frame data association on the device against the host: eao_object_np_association_batch at the workload of a frame -- 10 detections of
300 good points against 30 map objects of 2700 (sampled to 900 by upstream's rule) -- and at one detection against the 30 objects (the one call upstream's
per-detection loop allows), and eao_object_project_rects_batch over the 30 objects, against tools/object_association_walk.cpp built -O3 -ffp-contract=off where
this runs, on one thread: the library's host header counting in the kernel's form, and upstream's form (sort each axis, stride, three compares per pair).

Per shape: host wall clock around the C entry point (ctypes, arrays packed beforehand; the call ends in the stream's wait) and the HIP-event time of the kernel.
Median (min .. max) of --reps calls behind --warmup.  A record only: nothing is gated.

    python tools/bench_object_association.py [--reps 100] [--warmup 10] [--out profiles/object_association_timing.txt]
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

import torch  # noqa: E402,F401  (first: both runtimes resolve the same libamdhip64)

from eao_fusion_amd import _lib  # noqa: E402
from eao_fusion_amd import object_association as OA  # noqa: E402

N_DET, M, N_MAP, N_GOOD = 10, 300, 30, 2700


def spread(v):
    v = np.asarray(v)
    return "%9.1f (%.1f .. %.1f)" % (np.median(v), v.min(), v.max())


def clouds(count, n, seed):
    rs = np.random.RandomState(seed)
    return [np.ascontiguousarray(rs.uniform(-1, 1, 3) + rs.normal(0, 0.3, (n, 3)), np.float32) for _ in range(count)]


def time_np(dets, maps, reps, warmup):
    pairs = [(d, j) for d in range(len(dets)) for j in range(len(maps))]
    keep, args, P = OA._lists(dets, maps, None, pairs)
    verdict = np.zeros(P, np.int32)
    L = _lib.load()

    def call():
        _lib.check(L.eao_object_np_association_batch(*args, _lib.ptr(verdict), None, None))

    OA.set_profiling(False)
    for _ in range(warmup):
        call()
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e6)
    OA.set_profiling(True)
    kern = []
    for _ in range(max(reps // 4, 5)):
        call()
        kern.append(OA.last_kernel_ms()[0] * 1e3)
    OA.set_profiling(False)
    return wall, kern, verdict.copy()


def time_rects(maps, reps, warmup):
    T = np.eye(4, dtype=np.float32)
    T[:3, 3] = (0.1, -0.2, 4.0)
    start, xyz = OA._pack(maps)
    rect, status = np.zeros((len(maps), 4), np.int32), np.zeros(len(maps), np.uint8)
    L = _lib.load()

    def call():
        _lib.check(L.eao_object_project_rects_batch(len(maps), _lib.ptr(start), _lib.ptr(xyz), _lib.ptr(T), 517.3, 516.5, 318.6, 255.3, 640, 480, _lib.ptr(rect),
                                                    _lib.ptr(status), None))

    OA.set_profiling(False)
    for _ in range(warmup):
        call()
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e6)
    OA.set_profiling(True)
    kern = []
    for _ in range(max(reps // 4, 5)):
        call()
        kern.append(OA.last_kernel_ms()[1] * 1e3)
    OA.set_profiling(False)
    return wall, kern


def host(exe, n_det, reps):
    out = subprocess.run([exe], input="time %d %d %d %d %d\n" % (n_det, M, N_MAP, N_GOOD, reps), capture_output=True, text=True, check=True).stdout.split()
    assert out[0] == "time"
    return float(out[1]), float(out[2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "object_association_timing.txt"))
    a = ap.parse_args()
    lines = ["# tools/bench_object_association.py --reps %d --warmup %d: microseconds, median (min .. max); Object_2D::NoParaDataAssociation for detections of %d good "
             "points against %d map objects of %d good points each (step 3, a sample of 900), and Object_Map::ComputeProjectRectFrame over the %d objects"
             % (a.reps, a.warmup, M, N_MAP, N_GOOD, N_MAP),
             "# device: host wall clock around the entry point (ends in the stream's wait; it holds the upload of the points), HIP events around the kernel",
             "# host: tools/object_association_walk.cpp, one thread, -O3 -ffp-contract=off, built and run on the same machine in the same run, over uniform points "
             "of its own: the kernel's form (lb / ub over all good points) and upstream's form (sort, stride, three compares per pair)"]
    dets, maps = clouds(N_DET, M, 1), clouds(N_MAP, N_GOOD, 2)
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "object_association_walk")
        subprocess.check_call(["g++", "-O3", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tools", "object_association_walk.cpp"), "-o", exe])
        for title, nd in (("%d detections x %d objects, one call (%d pairs)" % (N_DET, N_MAP, N_DET * N_MAP), N_DET), ("1 detection x %d objects, one call" % N_MAP, 1)):
            wall, kern, verdict = time_np(dets[:nd], maps, a.reps, a.warmup)
            h_kernel_form, h_upstream = host(exe, nd, 3 if nd > 1 else 10)
            lines.append(title)
            lines.append("    device, wall clock of the call            %s us" % spread(wall))
            lines.append("    device, k_np_counts (HIP events)          %s us" % spread(kern))
            lines.append("    host, upstream's form, one thread         %9.1f us" % h_upstream)
            lines.append("    host, the kernel's form, one thread       %9.1f us" % h_kernel_form)
            lines.append("    host (upstream's form) / device wall      %9.2f" % (h_upstream / np.median(wall)))
            lines.append("    verdicts 0 / 1 / 2 / 3                    %d / %d / %d / %d" % tuple(int((verdict == v).sum()) for v in range(4)))
    wall, kern = time_rects(maps, a.reps, a.warmup)
    lines.append("projected boxes of %d objects of %d points, one call" % (N_MAP, N_GOOD))
    lines.append("    device, wall clock of the call            %s us" % spread(wall))
    lines.append("    device, k_project_rects (HIP events)      %s us" % spread(kern))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
