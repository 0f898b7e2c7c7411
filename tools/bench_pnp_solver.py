"""PnPsolver on the device: the time of one eao_pnp_solver_iterate call (host wall clock around the Python binding; the call ends in the stream's wait) and of each
of its four kernels (HIP events under EAO_PNP_EVENTS=1, eao_pnp_solver_last_kernel_ms), at N = 100 and N = 500 correspondences with Relocalization's parameters
(SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991): 35 hypotheses, min_set 4), and of five such candidates through eao_pnp_solver_iterate_batch: the median of --reps
calls behind --warmup calls.  Beside it the single-threaded numpy yardstick's time for the same scene (tests/pnp_solver_reference.py, jacobi variant, one run),
labelled as such: it is a restatement for checking, not an implementation anybody would ship, so no speed-up is claimed from it.  A record only: the parent commit has
nothing to compare against, and the reference's PnPsolver needs OpenCV.

    python tools/bench_pnp_solver.py [--reps 200] [--warmup 20] [--out profiles/pnp_solver_timing.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

os.environ["EAO_PNP_EVENTS"] = "1"      # read once, at the library's first call
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402,F401  (first: both runtimes resolve the same libamdhip64)

from eao_fusion_amd.pnp_solver import last_kernel_ms, pnp_solver_iterate, pnp_solver_iterate_batch  # noqa: E402
import pnp_solver_reference as Y  # noqa: E402
import pnp_solver_scenes as SC  # noqa: E402

KERNELS = ("hypotheses", "scan", "refine", "finish")


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    call, kern = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        call.append((time.perf_counter() - t0) * 1e3)
        kern.append(last_kernel_ms())
    return r, np.array(call), np.array(kern)


def report(lines, call, kern):
    lines.append("  call            %8.3f (%.3f .. %.3f)" % (np.median(call), call.min(), call.max()))
    for k, name in enumerate(KERNELS):
        lines.append("  k_pnp_%-10s %7.3f (%.3f .. %.3f)" % (name, np.median(kern[:, k]), kern[:, k].min(), kern[:, k].max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = ["# tools/bench_pnp_solver.py --reps %d --warmup %d: milliseconds, median (min .. max); call = host wall clock of the Python binding, kernels = HIP events" % (a.reps, a.warmup),
             "# numpy yardstick = tests/pnp_solver_reference.py (jacobi), single thread, one run: a checking restatement, not a baseline; the reference's PnPsolver needs OpenCV and was not timed"]
    cases = {}
    for n in (100, 500):
        c = cases[n] = SC.case(n, 200 + n, 4, 0, noise_px=1.0, outlier_frac=0.3, kind="min4", params=SC.RELOCALIZATION)
        r, call, kern = timed(lambda: pnp_solver_iterate(c["prob"], None, c["sets"], c["min_inliers"], c["max_its"]), a.reps, a.warmup)
        t0 = time.perf_counter()
        ref = Y.iterate(c["prob"], None, c["sets"], c["min_inliers"], c["max_its"], "jacobi")
        ref_ms = (time.perf_counter() - t0) * 1e3
        lines.append("N=%d hypotheses=%d min_set=4 min_inliers=%d: returned %d refined %d inliers %d (yardstick %d %d %d)"
                     % (n, len(c["sets"]), c["min_inliers"], r["returned"], r["refined"], r["n_inliers"], ref["returned"], ref["refined"], ref["n_inliers"]))
        report(lines, call, kern)
        lines.append("  numpy yardstick %8.1f" % ref_ms)
    for n in (100, 500):
        cs = [SC.case(n, 300 + n + b, 4, 0, noise_px=1.0, outlier_frac=0.3, kind="min4", params=SC.RELOCALIZATION) for b in range(5)]
        args = ([c["prob"] for c in cs], [None] * 5, [c["sets"] for c in cs], [c["min_inliers"] for c in cs], [c["max_its"] for c in cs])
        r, call, kern = timed(lambda: pnp_solver_iterate_batch(*args), a.reps, a.warmup)
        lines.append("batch of 5 candidates, N=%d, 35 hypotheses each: returned %s" % (n, [o["returned"] for o in r]))
        report(lines, call, kern)
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
