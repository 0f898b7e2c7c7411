"""OptimizeSim3 on the device: call time (host wall clock around eao_optimize_sim3 / _batch) and device time (HIP events around the
launch, eao_last_lm_timing) for 100, 300 and 1000 matches, single and batched (16 problems), median over --reps after --warmup calls.

    python tools/bench_sim3.py [--reps 50] [--warmup 10] [--out profiles/sim3_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402,F401  (first: both runtimes resolve the same libamdhip64)

from eao_fusion_amd.optimizer import optimize_sim3, optimize_sim3_batch, pack_sim3_batch  # noqa: E402
import sim3_scenes as SC  # noqa: E402


def measure(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    wall, dev = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        wall.append((time.perf_counter() - t0) * 1e3)
        tm = (out[0] if isinstance(out, list) else out)["timing"]
        dev.append(tm["device_ms"])
    return float(np.median(wall)), float(np.median(dev)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    for n in (100, 300, 1000):
        p = SC.scene(n=n, seed=7000 + n, fix_scale=True, outlier_frac=0.1)
        call, dev, o = measure(lambda: optimize_sim3(p), a.reps, a.warmup)
        rows.append(dict(n=n, batch=1, call_ms=call, device_ms=dev, iters=[int(v) for v in o["iters"]]))
        probs = [SC.scene(n=n, seed=7100 + n + k, fix_scale=(k % 2 == 0), outlier_frac=0.1) for k in range(16)]
        pk = pack_sim3_batch(probs)
        call, dev, o = measure(lambda: optimize_sim3_batch(probs, packed=pk), a.reps, a.warmup)
        rows.append(dict(n=n, batch=16, call_ms=call, device_ms=dev, iters=[int(v) for v in o[0]["iters"]]))
    for r in rows:
        print("n %5d  batch %2d  call %.3f ms  device %.3f ms  iters %s" % (r["n"], r["batch"], r["call_ms"], r["device_ms"], r["iters"]))
    res = dict(tool="bench_sim3", reps=a.reps, warmup=a.warmup, rows=rows)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
