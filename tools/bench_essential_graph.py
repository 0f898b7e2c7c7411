#!/usr/bin/env python3
"""Device time and call time of eao_optimize_essential_graph on ring graphs of 100 and 1000 keyframes (tests/essential_graph_scenes.ring, both fix_scale values).
Writes profiles/essential_graph_bench.json (or --out); nothing is gated on these numbers.  --once N: one call on the N-keyframe graph and nothing else -- the
program a `rocprofv3 --kernel-trace --stats` run wraps for the kernel list stored beside the numbers (--kernel-stats FILE merges such a CSV into the record)."""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def graph(n, fs):
    import essential_graph_scenes as SC
    return SC.ring(n=n, seed=900 + n, fix_scale=fs, rot_drift=1e-3, trans_drift=3e-3, n_chords=n // 2, chord_span=10, n_points=20 * n)


def measure(n, fs, reps):
    import numpy as np
    from eao_fusion_amd.optimizer import essential_graph_plan, optimize_essential_graph
    prob = graph(n, fs)
    plan = essential_graph_plan(prob)
    out = optimize_essential_graph(prob)      # warm-up: context, plan, workspace
    dev, call = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = optimize_essential_graph(prob)
        call.append((time.perf_counter() - t0) * 1e3)
        dev.append(float(out["timing"]["device_ms"]))
    return dict(keyframes=n, edges=int(len(prob["edges"])), points=int(len(prob["Xw"])), fix_scale=bool(fs), lm_iterations=out["lm_iterations"],
                trials=[int(t) for t in out["trials"]], plan={k: plan[k] for k in ("rows", "tiles", "segments", "separators", "launches")}, device_ms_median=float(np.median(dev)), call_ms_median=float(np.median(call)),
                device_ms_min=float(min(dev)), call_ms_min=float(min(call)), reps=reps)


def kernel_stats(path):
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            rows.append({k: r[k] for k in r if k in ("Name", "Calls", "TotalDurationNs", "AverageNs", "Percentage")})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--once", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "essential_graph_bench.json"))
    ap.add_argument("--kernel-stats", default=None)
    a = ap.parse_args()
    import torch  # noqa: F401  (first, so that both runtimes resolve the same libamdhip64)
    if a.once:
        from eao_fusion_amd.optimizer import optimize_essential_graph
        o = optimize_essential_graph(graph(a.once, False))
        print("once: %d keyframes, %d iterations, trials %s" % (a.once, o["lm_iterations"], list(o["trials"])))
        return
    rec = dict(what="eao_optimize_essential_graph on one MI355X: ring graphs with chords, 20 map points per keyframe", runs=[measure(n, fs, a.reps) for n in (100, 1000) for fs in (False, True)])
    if a.kernel_stats and os.path.exists(a.kernel_stats):
        rec["kernel_stats_1000_keyframes_one_call"] = kernel_stats(a.kernel_stats)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec["runs"]))


if __name__ == "__main__":
    main()
