"""The chained update of a map object (eao_object_update_chain / _batch: point update, erase of the bad points, cuboid, isolation forest in one device call)
against the three existing entries called in sequence and against the host, over the four update shapes of profiles/object_points_timing.txt: one
DataAssociateUpdate of 50 x 20, 500 x 100 and 2000 x 200 points, and a frame's ten updates in one call.

Per shape, median (min .. max) of --reps calls behind --warmup:
    chain       host wall clock around the C entry point (ctypes, descriptors packed beforehand; the call ends in the stream's wait and holds the upload and the
                download) and, in separate calls, the HIP-event time of each of its kernels
    sequence    eao_object_points_update[_batch] -> eao_object_cuboids[_batch] -> eao_object_iforest_outliers_batch back to back in the same run, every
                descriptor packed beforehand: the cuboid and the forest are handed the final lists (known from the chain's result), so the figure holds NO host
                work between the calls -- no erase of the bad points, no second gather.  It flatters the sequence.
    host        tools/object_chain_walk.cpp (the three HIP-free headers chained, upstream's literal forms WITHOUT cv::Mat clones and the mutex), -O3
                -ffp-contract=off, one thread, the same descs.  It flatters the host; upstream's own loop is not measured.
Before anything is timed the chain's outputs are held to the walk program's on every desc.  A record only: nothing is gated.

    python tools/bench_object_chain.py [--reps 200] [--warmup 20] [--out profiles/object_chain_timing.txt]
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

import object_chain_reference as Y  # noqa: E402
import object_chain_scenes as SC  # noqa: E402
from eao_fusion_amd import _lib  # noqa: E402
from eao_fusion_amd import isolation_forest as IFB  # noqa: E402
from eao_fusion_amd import object_chain as CH  # noqa: E402
from eao_fusion_amd import object_cuboid as OCB  # noqa: E402
from eao_fusion_amd import object_points as OPB  # noqa: E402


def spread(v):
    v = np.asarray(v)
    return "%9.1f (%.1f .. %.1f)" % (np.median(v), v.min(), v.max())


def timed(call, reps, warmup):
    for _ in range(warmup):
        call()
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e6)
    return wall


def time_chain(descs, single, reps, warmup):
    keep, cd, co = CH._descs(descs, 0, True)
    L = _lib.load()

    def call():
        _lib.check(L.eao_object_update_chain(cd, co) if single else L.eao_object_update_chain_batch(len(descs), cd, co))

    CH.set_profiling(False)
    wall = timed(call, reps, warmup)
    CH.set_profiling(True)
    kern = []
    for _ in range(max(reps // 4, 5)):
        call()
        kern.append([ms * 1e3 for ms in CH.last_kernel_ms()])
    CH.set_profiling(False)
    return wall, np.array(kern), [CH.trim(d, k[5]) for d, k in zip(descs, keep)]


def time_sequence(descs, results, single, reps, warmup):
    """the three entries back to back over descriptors packed beforehand; returns the wall clock of the three calls together and of each"""
    L = _lib.load()
    pdescs = [dict(d, map_count=Y.raised_counts(d)) for d in descs]      # the caller that needs the incremented count passes it in map_count
    _pk, pd, po = OPB._descs(pdescs, 0, True)
    objs = [Y.final_object(d, r) for d, r in zip(descs, results)]
    _ck, cdesc = OCB._descs(objs)
    crec = np.zeros(len(objs), OCB.RECORD_DTYPE)
    start, xyz = IFB._pack([o["points"] for o in objs])
    cls = np.ascontiguousarray([d["class_id"] for d in descs], np.int32)
    flags, removed = np.zeros(max(int(start[-1]), 1), np.uint8), np.zeros(len(objs), np.int32)
    n = len(descs)
    calls = [lambda: _lib.check(L.eao_object_points_update(pd, po) if single else L.eao_object_points_update_batch(n, pd, po)),
             lambda: _lib.check(L.eao_object_cuboids(cdesc, _lib.ptr(crec)) if single else L.eao_object_cuboids_batch(n, cdesc, _lib.ptr(crec))),
             lambda: _lib.check(L.eao_object_iforest_outliers_batch(n, _lib.ptr(start), _lib.ptr(xyz), _lib.ptr(cls), 1, _lib.ptr(flags), _lib.ptr(removed), None))]

    def call():
        for c in calls:
            c()

    total = timed(call, reps, warmup)
    each = [timed(c, reps, 5) for c in calls]
    for r, rec, f0, f1 in zip(results, crec, start[:-1], start[1:]):      # the same results, or the comparison compares nothing
        if not (Y.OC.same_records(rec, r["cuboid"]) and np.array_equal(flags[f0:f1], r["forest_flags"])):
            raise SystemExit("the sequence and the chain disagree on a desc")
    return total, each


def host(exe, descs, reps):
    script = "".join(Y.walk_script(d, "load") for d in descs) + "time %d\n" % reps
    out = subprocess.run([exe], input=script, capture_output=True, text=True, check=True).stdout.split()
    assert out[0] == "time"
    return float(out[1])


def hold_to_the_walk(exe, descs, results):
    out = subprocess.run([exe], input="".join(Y.walk_script(d) for d in descs), capture_output=True, text=True, check=True).stdout.strip().split("\n")
    for line, d, res in zip(out, descs, results):
        if line.split() != Y.walk_tokens(d, res):
            raise SystemExit("the device and the host walk disagree on a desc")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "object_chain_timing.txt"))
    a = ap.parse_args()
    props = torch.cuda.get_device_properties(0)
    lines = ["# tools/bench_object_chain.py --reps %d --warmup %d on %s (%s, %d compute units): microseconds, median (min .. max); the point update, the erase of the bad "
             "points, the cuboid and the isolation forest of Object_Map::DataAssociateUpdate (src/Object.cc:1352-1601)" % (
                 a.reps, a.warmup, props.name, getattr(props, "gcnArchName", "?"), props.multi_processor_count),
             "# chain: host wall clock around eao_object_update_chain[_batch] (ends in the stream's wait; it holds the upload and the download); HIP events around each of "
             "its kernels, in separate calls",
             "# sequence: eao_object_points_update -> eao_object_cuboids -> eao_object_iforest_outliers_batch back to back in the same run, descriptors packed beforehand "
             "and the final lists handed in: NO host work between the calls (no erase of the bad points, no second gather): it flatters the sequence",
             "# host: tools/object_chain_walk.cpp (the three host walks chained, upstream's literal forms without cv::Mat clones and the mutex: it flatters the host), one "
             "thread, -O3 -ffp-contract=off, same machine, same run, same descs; every desc's chain outputs were held to it first.  Upstream's own loop is not measured."]
    rng = np.random.default_rng(2024)
    frame = []
    for M, C in ((50, 20), (120, 40), (200, 60), (350, 80), (500, 100), (700, 120), (900, 140), (1200, 160), (1600, 180), (2000, 200)):
        d = SC.frame(rng, M, C)
        d["map_bad"][rng.choice(M, max(M // 50, 1), replace=False)] = 1
        frame.append(d)
    shapes = [("1 update of 50 list points x 20 candidates", [frame[0]], True), ("1 update of 500 list points x 100 candidates", [frame[4]], True),
              ("1 update of 2000 list points x 200 candidates", [frame[9]], True), ("a frame's 10 updates (50 .. 2000 list points, 20 .. 200 candidates), one call per entry", frame, False)]
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "object_chain_walk")
        subprocess.check_call(["g++", "-O3", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tools", "object_chain_walk.cpp"), "-o", exe])
        for title, descs, single in shapes:
            wall, kern, results = time_chain(descs, single, a.reps, a.warmup)
            hold_to_the_walk(exe, descs, results)
            total, each = time_sequence(descs, results, single, a.reps, a.warmup)
            h = host(exe, descs, 50)
            lines.append("%s; n_final %s, forests run: %d" % (title, " ".join(str(int(r["chain"]["n_final"])) for r in results),
                                                              sum(int(r["chain"]["forest_status"]) == CH.FOREST_DONE for r in results)))
            lines.append("    chain, wall clock of the call             %s us" % spread(wall))
            for k, name in enumerate(CH.KERNELS):
                col = kern[:, k]
                lines.append("        %-38s%s us" % (name, spread(col) if (col >= 0).all() else "        - (did not run)"))
            lines.append("        the kernels together                  %s us" % spread(np.where(kern >= 0, kern, 0).sum(axis=1)))
            lines.append("    sequence, wall clock of the three calls   %s us" % spread(total))
            for name, w in zip(("eao_object_points_update", "eao_object_cuboids", "eao_object_iforest_outliers_batch"), each):
                lines.append("        %-38s%s us" % (name, spread(w)))
            lines.append("    host, the three walks chained, one thread %9.1f us" % h)
            lines.append("    sequence / chain                          %9.2f" % (np.median(total) / np.median(wall)))
            lines.append("    host / chain                              %9.2f" % (h / np.median(wall)))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
