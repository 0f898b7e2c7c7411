#!/usr/bin/env python3
"""The timing record of the plane segmentation: eao_plane_seg_run on the VGA room of tests/plane_segmentation_scenes.py, per stage and end
to end, beside tools/plane_segmentation_walk.cpp's `bench` (the whole function on one host thread, -O3 -march=native -ffp-contract=off) on the same machine's
CPU.  Median (min .. max) of --calls calls after --warmup calls.  A record, no bar.

    python tools/bench_plane_segmentation.py [--calls 200] [--warmup 20] [--out profiles/plane_segmentation_timing.txt]
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
STAGES = ("upload of the depth image", "k_ps_block_init + record download", "host middle", "membership + voxel stage")


def fmt(us):
    us = np.asarray(us, np.float64)
    return "%9.1f us (%.1f .. %.1f)" % (np.median(us), us.min(), us.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plane_segmentation_timing.txt"))
    a = ap.parse_args()
    import torch  # noqa: F401  (first, so that both runtimes resolve the same HIP library)
    import plane_segmentation_reference as R
    import plane_segmentation_scenes as S
    from eao_fusion_amd.plane_seg import PlaneSegmenter, cfg_from
    scene = S.scenes()["room_vga"]
    c, depth = scene["cfg"], scene["depth"]
    ps = PlaneSegmenter(cfg_from(c))

    def read_back():
        planes = ps.planes()
        return planes, [ps.cloud(k) for k, p in enumerate(planes) if p["kept"]]      # what include/eaofusion/PlaneExtractor.h reads

    def timed(profiling):
        ps.set_profiling(profiling)
        stages, back, total = [], [], []
        for k in range(a.warmup + a.calls):
            t0 = time.perf_counter()
            ps.run(depth)
            t1 = time.perf_counter()
            read_back()
            t2 = time.perf_counter()
            if k >= a.warmup:
                if profiling:
                    stages.append(ps.last_timing())
                back.append((t2 - t1) * 1e6)
                total.append((t2 - t0) * 1e6)
        return np.array(stages), back, total

    stages, back, _ = timed(True)
    _, _, total = timed(False)
    planes, clouds = read_back()
    info = ps.info()
    with tempfile.TemporaryDirectory() as d:
        exe, sc = os.path.join(d, "walk"), os.path.join(d, "room_vga.bin")
        subprocess.check_call(["g++", "-std=c++17", "-O3", "-march=native", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tools", "plane_segmentation_walk.cpp")])
        open(sc, "wb").write(R.scene_bytes(c, depth))
        walk = subprocess.run([exe, "bench", sc, str(a.calls)], capture_output=True, text=True, check=True).stdout.strip()
    lines = ["plane segmentation, %d x %d room (tests/plane_segmentation_scenes.py room_vga): %d planes (%d kept), %d member pixels, %d flood-fill claims, %d voxels"
             % (c.width, c.height, len(planes), sum(p["kept"] for p in planes), sum(p["n_pixels"] for p in planes), info["n_claims"], info["n_points"]),
             "median (min .. max) of %d calls after %d warm-up calls; host clock around stages that each end in a wait" % (a.calls, a.warmup), ""]
    for k, name in enumerate(STAGES):
        lines.append("%-40s %s" % (name, fmt(stages[:, k])))
    lines.append("%-40s %s" % ("read-back (plane table, kept clouds)", fmt(back)))
    lines.append("%-40s %s" % ("end to end (run + read-back), no profiling", fmt(total)))
    lines.append("")
    lines.append("host walk, one thread, same scene:       " + walk)
    share = float(np.median(stages[:, 2]) / np.median(stages.sum(axis=1)))
    lines.append("host middle's share of eao_plane_seg_run: %.0f %%" % (100 * share))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
