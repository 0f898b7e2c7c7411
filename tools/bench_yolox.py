#!/usr/bin/env python3
"""Times the yolox feature on the device and the -O3 single-thread host walk in one run, and writes profiles/yolox_timing.txt.

    python tools/bench_yolox.py [--out profiles/yolox_timing.txt] [--reps 200]

Shapes: a 640 x 480 colour frame into the 640 x 640 blob (with the grey image), and the decode of a 640 head with about 300 proposals; one frame and a batch of
64.  Device times are the handle's kernel clock (HIP events around each kernel, eao_yolox_last_kernel_ms): after 20 warm-up calls, the median and the 10th / 90th
percentile over --reps calls.  Call times are a host clock around the synchronous entry points (upload, kernels, copy back, wait).  The host walk is
tools/yolox_walk.cpp built with g++ -O3 (its best of 20 repetitions).  Algorithmic bytes of the pre-processing: it reads 3 w h bytes and writes 12 S^2 (+ w h)."""
import argparse
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KERNELS = ("k_yolox_pre", "k_yolox_proposals", "k_yolox_rank", "k_yolox_mask", "k_yolox_scan")


def bench_head(seed=1):
    """the head of tools/yolox_walk.cpp's bench: 300 anchors 28 apart, one class each above the threshold"""
    f = np.zeros((8400, 85), np.float32)
    rs = np.random.RandomState(seed)
    for a in range(0, 8400, 28):
        f[a, :5] = (0.5, 0.5, 1.0 + rs.randint(0, 256) / 256.0, 1.5, 0.9)
        f[a, 5 + a % 80] = 0.4 + rs.randint(0, 1024) / 2048.0
    return f


def pct(v):
    v = np.sort(np.asarray(v, np.float64))
    return "%8.4f  [%.4f .. %.4f]" % (np.median(v), v[int(0.1 * (len(v) - 1))], v[int(0.9 * (len(v) - 1))])


def measure(h, batch, reps, lines):
    frames = np.random.RandomState(2).randint(0, 256, (batch, 480, 640, 3)).astype(np.uint8)
    heads = np.stack([bench_head(f) for f in range(batch)])
    sizes = [(640, 480)] * batch
    gray = np.zeros((batch, 480, 640), np.uint8)
    from eao_fusion_amd import _lib
    L = _lib.load()

    def pre():
        _lib.check(L.eao_yolox_preprocess(h._h, frames.ctypes.data, 640, 480, 1920, 1920 * 480, batch, 0, gray.ctypes.data, 640))

    out = None
    for _ in range(20):
        pre()
        out = h.decode_raw(heads, sizes)
    assert out["status"] == 0
    h.set_profiling(True)
    ms, call_pre, call_dec = [], [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        pre()
        t1 = time.perf_counter()
        h.decode_raw(heads, sizes, out=out)
        t2 = time.perf_counter()
        ms.append(h.last_kernel_ms())
        call_pre.append((t1 - t0) * 1e3)
        call_dec.append((t2 - t1) * 1e3)
    h.set_profiling(False)
    ms = np.array(ms)
    lines.append("batch %d (%d proposals, %d objects per frame; %d calls after 20 warm-up calls), ms: median [p10 .. p90]" % (batch, out["n_proposals"][0], out["n"][0], reps))
    for k, name in enumerate(KERNELS):
        lines.append("  %-18s %s" % (name, pct(ms[:, k])))
    lines.append("  %-18s %s" % ("decode kernels", pct(ms[:, 1:].sum(axis=1))))
    lines.append("  %-18s %s   (host clock: upload of %d x 921600 bytes, kernel, grey copy back, wait)" % ("preprocess call", pct(call_pre), batch))
    lines.append("  %-18s %s   (host clock: upload of %d x 2856000 bytes, four kernels, copies back, two waits)" % ("decode call", pct(call_dec), batch))
    rd, wr = 3 * 640 * 480 * batch, (12 * 640 * 640 + 640 * 480) * batch
    lines.append("  k_yolox_pre algorithmic bytes: reads %d, writes %d; over the median kernel time %.1f GB/s" % (rd, wr, (rd + wr) / (np.median(ms[:, 0]) * 1e-3) / 1e9))
    return float(np.median(ms[:, 0])), float(np.median(ms[:, 1:].sum(axis=1)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yolox_timing.txt"))
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    import torch  # noqa: F401
    from eao_fusion_amd import yolox
    lines = ["yolox: pre-processing of a 640 x 480 frame into 640 x 640 and the decode of a 640 head (tools/bench_yolox.py)", ""]
    dev = {}
    for batch in (1, 64):
        h = yolox.Yolox(max_batch=batch)
        dev[batch] = measure(h, batch, a.reps, lines)
        h.close()
        lines.append("")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "yolox_walk")
        subprocess.check_call(["g++", "-O3", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tools", "yolox_walk.cpp"), "-o", exe])
        got = dict(ln.split() for ln in subprocess.run([exe], input="bench 20\n", capture_output=True, text=True, check=True).stdout.strip().split("\n"))
    lines.append("host walk (tools/yolox_walk.cpp, g++ -O3, one thread, best of 20, one frame; %s proposals, %s objects):" % (got["proposals"], got["objects"]))
    lines.append("  pre-processing %s ms, decode %s ms" % (got["host_pre_ms"], got["host_decode_ms"]))
    lines.append("  device kernels, one frame: pre-processing %.4f ms, decode %.4f ms; per frame of the batch of 64: %.4f ms, %.4f ms" % (
        dev[1][0], dev[1][1], dev[64][0] / 64, dev[64][1] / 64))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
