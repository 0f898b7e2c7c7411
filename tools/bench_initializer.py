"""Initializer on the device: the time of one eao_initializer_initialize call (host wall clock around the Python binding; the call ends in the stream's wait) and of each
of its five kernels (HIP events under EAO_INIT_EVENTS=1, eao_initializer_last_kernel_ms), at N = 500 and N = 2000 matches with 200 sets: the median of --reps calls behind --warmup calls.  Beside it
the single-threaded numpy yardstick's time for the same scene (tests/initializer_reference.py, one run), labelled as such: it is a restatement for checking, not an
implementation anybody would ship, so no speed-up is claimed from it.  A record only: the parent commit has nothing to compare against.

    python tools/bench_initializer.py [--reps 200] [--warmup 20] [--out profiles/initializer_bench.txt]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

os.environ["EAO_INIT_EVENTS"] = "1"      # read once, at the library's first call
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402,F401  (first: both runtimes resolve the same libamdhip64)

from eao_fusion_amd import _lib  # noqa: E402
from eao_fusion_amd.initializer import initialize  # noqa: E402
import initializer_reference as R  # noqa: E402
import initializer_scenes as SC  # noqa: E402

KERNELS = ("hypotheses", "scores", "select", "check_rt", "finish")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = ["# tools/bench_initializer.py --reps %d --warmup %d: milliseconds, median (min .. max); call = host wall clock of the Python binding, kernels = HIP events" % (a.reps, a.warmup),
             "# numpy yardstick = tests/initializer_reference.py, single thread, one run: a checking restatement, not a baseline; the reference's Initializer needs OpenCV and was not timed"]
    L = _lib.load()
    for n in (500, 2000):
        prob = SC.scene(n=n, seed=120, extra=0, extra2=0, iterations=200)
        for _ in range(a.warmup):
            initialize(prob, prob["sets"])
        call, kern = [], []
        ms = (C.c_float * 5)()
        for _ in range(a.reps):
            t0 = time.perf_counter()
            r = initialize(prob, prob["sets"])
            call.append((time.perf_counter() - t0) * 1e3)
            _lib.check(L.eao_initializer_last_kernel_ms(ms))
            kern.append(list(ms))
        kern = np.array(kern)
        t0 = time.perf_counter()
        ref = R.initialize(prob, prob["sets"], "f64jacobi")
        ref_ms = (time.perf_counter() - t0) * 1e3
        lines.append("N=%d sets=200 returned %d (yardstick %d)" % (n, r["returned"], ref["returned"]))
        lines.append("  call            %8.3f (%.3f .. %.3f)" % (np.median(call), min(call), max(call)))
        for k, name in enumerate(KERNELS):
            lines.append("  k_init_%-10s %6.3f (%.3f .. %.3f)" % (name, np.median(kern[:, k]), kern[:, k].min(), kern[:, k].max()))
        lines.append("  numpy yardstick %8.1f" % ref_ms)
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
