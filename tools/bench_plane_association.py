"""The plane association on the device against the host loop it replaces: the time of one eao_plane_map_associate call and of the literal single-thread walk
(tools/plane_association_walk.cpp, built -O3 -march=native -ffp-contract=off where this runs) at three shapes, and of eao_plane_map_update_boundary at 1000 points.

    tracked frame        10 rows, 30 planes x 1000 points, 1 set        Map::AssociatePlanesByBoundary, up to three times per frame
    large map            10 rows, 300 planes x 2000 points, 1 set
    SearchAndFuse batch  20 sets x 8 rows, 60 candidates x 1000 points   one call against 20 single calls (LoopClosing::SearchAndFuse)

Planes with random unit normals (a fifth of all pairs pass the 0.8 gate), clouds on the planes, every row a plane of the map seen with the identity pose; the
walk draws its own scene of the same distribution.  Host wall clock around the C entry points (ctypes, arrays packed beforehand); every device call ends in the
stream's wait and downloads match and match_dis only.  Median (min .. max) of --reps calls behind --warmup.
A record only: nothing is gated.

    python tools/bench_plane_association.py [--reps 200] [--warmup 20] [--out profiles/plane_association_timing.txt]
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

import torch  # noqa: E402  (first: both runtimes resolve the same libamdhip64)

from eao_fusion_amd import _lib  # noqa: E402
from eao_fusion_amd.plane_map import PlaneMap  # noqa: E402

SHAPES = [("tracked frame", 10, 30, 1000, 1), ("large map", 10, 300, 2000, 1), ("SearchAndFuse batch", 8, 60, 1000, 20)]


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e6)
    return np.array(out)


def spread(v):
    return "%9.1f (%.1f .. %.1f)" % (np.median(v), v.min(), v.max())


def scene(rs, planes, points):
    out = []
    for k in range(planes):
        n = rs.normal(size=3)
        n /= np.linalg.norm(n)
        d = 0.5 + 3.5 * k / planes
        p = rs.uniform(-1.5, 1.5, (points, 3))
        p -= (p @ n + d)[:, None] * n
        out.append((np.array([n[0], n[1], n[2], d], np.float32), p.astype(np.float32)))
    return out


def measure(label, rows, planes, points, sets, reps, warmup):
    L, p = _lib.load(), _lib.ptr
    rs = np.random.RandomState(planes)
    sc = scene(rs, planes, points)
    pm = PlaneMap()
    t_add = []
    for k, (w, xyz) in enumerate(sc):
        t0 = time.perf_counter()
        pm.add(k, w, xyz)
        t_add.append((time.perf_counter() - t0) * 1e6)
    M = np.tile(np.eye(4, dtype=np.float32).reshape(1, 16), (sets, 1))
    coef = np.array([sc[(s * rows + r) % planes][0] for s in range(sets) for r in range(rows)], np.float32)
    start = (np.arange(sets + 1) * rows).astype(np.int32)
    match, mdis = np.zeros(sets * rows, np.int32), np.zeros(sets * rows, np.float32)

    def call(n_sets, M, start, coef, match, mdis):
        assert L.eao_plane_map_associate(pm.h, n_sets, p(M), p(start), p(coef), planes, None, 0.2, 0.8, p(match), p(mdis), None, None, None) == 0

    t = timed(lambda: call(sets, M, start, coef, match, mdis), reps, warmup)
    assert (match == np.array([(s * rows + r) % planes for s in range(sets) for r in range(rows)])).mean() > 0.5      # (another plane's cloud may cross nearer)
    lines = ["%s: %d set(s) x %d rows, %d planes x %d points (%.1f MB resident)" % (label, sets, rows, planes, points, planes * points * 16 / 1e6),
             "    device, one call                                   %s us" % spread(t)]
    if sets > 1:
        one_start = np.array([0, rows], np.int32)
        parts = [(M[s:s + 1].copy(), coef[s * rows:(s + 1) * rows].copy(), np.zeros(rows, np.int32), np.zeros(rows, np.float32)) for s in range(sets)]

        def singles():
            for Ms, cs, ms, ds in parts:
                call(1, Ms, one_start, cs, ms, ds)

        t1 = timed(singles, max(reps // 4, 5), max(warmup // 4, 2))
        assert np.array_equal(np.concatenate([q[2] for q in parts]), match)
        lines.append("    device, %d single calls                            %s us" % (sets, spread(t1)))
    lines.append("    add (one plane, %d points)                        %s us" % (points, spread(np.array(t_add[len(t_add) // 2:]))))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "no device: nothing is measured without one"
    lines = ["# tools/bench_plane_association.py --reps %d --warmup %d: microseconds per call, median (min .. max); host wall clock around the C entry points, each device call ends in the stream's wait" % (a.reps, a.warmup)]
    for label, rows, planes, points, sets in SHAPES:
        lines += measure(label, rows, planes, points, sets, a.reps, a.warmup)
    # update_boundary at 1000 points on the tracked-frame map
    rs = np.random.RandomState(1)
    pm = PlaneMap()
    for k, (w, xyz) in enumerate(scene(rs, 30, 1000)):
        pm.add(k, w, xyz)
    new = [scene(rs, 1, 1000)[0][1] for _ in range(8)]
    T = np.eye(4, dtype=np.float32)
    T[:3, 3] = [0.1, -0.2, 0.3]
    L, p = _lib.load(), _lib.ptr
    k = [0]

    def update():
        k[0] += 1
        assert L.eao_plane_map_update_boundary(pm.h, k[0] % 30, 1000, p(new[k[0] % 8]), p(T.reshape(16))) == 0

    lines.append("update_boundary (1000 points, with the transform, compactions included)   %s us" % spread(timed(update, a.reps, a.warmup)))
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "plane_association_walk")
        subprocess.check_call(["g++", "-O3", "-march=native", "-ffp-contract=off", "-std=c++17", os.path.join(ROOT, "tools", "plane_association_walk.cpp"), "-o", exe])
        lines.append("# host walk (1 thread, -O3 -march=native -ffp-contract=off): the literal loops of src/Map.cc:155-292 over the same table, all sets in one go")
        for label, rows, planes, points, sets in SHAPES:
            r = max(min(a.reps, 2000000 // (rows * sets * planes * points // 50 + 1)), 5)
            lines.append("%s: %s" % (label, subprocess.run([exe, "bench", str(rows), str(planes), str(points), str(sets), str(r)], capture_output=True, text=True,
                                                           check=True).stdout.strip()))
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
