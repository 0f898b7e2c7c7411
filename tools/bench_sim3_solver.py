"""Sim3Solver on the device: call time (host wall clock around eao_sim3_solver_iterate / _batch, which end in a stream synchronise) of
  - one iterate(5) at N = 100,
  - one 300-hypothesis find at N = 100 and at N = 1000 (min_inliers = N, so that none returns early and all 300 are counted),
  - one batch of 8 candidates x 5 hypotheses at N = 100,
each the median of --reps runs behind --warmup calls, quoted with min and max.  A record only: the parent commit has nothing to compare against, and the
reference's Sim3Solver needs OpenCV, which the build image lacks, so its time is not taken either.

    python tools/bench_sim3_solver.py [--reps 5] [--warmup 2] [--out profiles/sim3_solver_timing.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402,F401  (first: both runtimes resolve the same libamdhip64)

from eao_fusion_amd.sim3_solver import sim3_solver_iterate, sim3_solver_iterate_batch  # noqa: E402
import sim3_solver_scenes as SC  # noqa: E402


def measure(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    p100 = SC.scene(n=100, seed=8100, fix_scale=True, outlier_frac=0.3)
    p1000 = SC.scene(n=1000, seed=8101, fix_scale=True, outlier_frac=0.3)
    t100, t1000 = SC.drawn_triples(100, 300, 1), SC.drawn_triples(1000, 300, 2)
    cands = [SC.scene(n=100, seed=8200 + k, fix_scale=True, outlier_frac=0.3) for k in range(8)]
    ctri = [SC.drawn_triples(100, 5, 10 + k) for k in range(8)]
    rows = [("iterate(5) N=100", lambda: sim3_solver_iterate(p100, None, t100[:5], min_inliers=100)),
            ("find 300 hypotheses N=100", lambda: sim3_solver_iterate(p100, None, t100, min_inliers=100)),
            ("find 300 hypotheses N=1000", lambda: sim3_solver_iterate(p1000, None, t1000, min_inliers=1000)),
            ("batch 8 candidates x 5 hypotheses N=100", lambda: sim3_solver_iterate_batch(cands, [None] * 8, ctri, min_inliers=100))]
    lines = ["# tools/bench_sim3_solver.py --reps %d --warmup %d: host wall clock per call (Python binding included), milliseconds; a record, no bar" % (a.reps, a.warmup),
             "# the reference's Sim3Solver was not timed (it needs OpenCV): no speed-up is claimed"]
    for name, fn in rows:
        med, lo, hi = measure(fn, a.reps, a.warmup)
        lines.append("%-42s median %.3f ms  min %.3f  max %.3f" % (name, med, lo, hi))
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
