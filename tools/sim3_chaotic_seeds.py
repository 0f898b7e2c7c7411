"""Which OptimizeSim3 parity families (tests/sim3_scenes.FAMILIES) are rounding-sensitive in the reference itself: each family is run
through tests/sim3_reference.py as generated and with every observation moved by one float32 ulp, and what changed is printed.
The evidence behind sim3_scenes.ITERS_UNSTABLE.

    python tools/sim3_chaotic_seeds.py > profiles/r07_sim3_chaotic_seeds.txt
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import sim3_reference as R  # noqa: E402
import sim3_scenes as SC  # noqa: E402


def main():
    print("family n seed | iters (as generated) | iters (one ulp) | removed same | n_inliers same | early_exit same | displacement / update")
    for name, kw in SC.FAMILIES:
        p = SC.scene(**kw)
        a, b = R.optimize_sim3(p), R.optimize_sim3(SC.ulp_perturbed(p))
        upd = max(np.abs(a["q"] - p["q"]).max(), np.abs(a["t"] - p["t"]).max(), abs(a["s"] - p["s"]))
        disp = max(np.abs(a["q"] - b["q"]).max(), np.abs(a["t"] - b["t"]).max(), abs(a["s"] - b["s"]))
        mark = "  ITERS MOVE" if list(a["iters"]) != list(b["iters"]) else ""
        print("%-10s %4d %3d | %-7s | %-7s | %s | %s | %s | %.2e%s" % (name, kw["n"], kw["seed"], list(map(int, a["iters"])), list(map(int, b["iters"])),
              bool(np.array_equal(a["removed"], b["removed"])), a["n_inliers"] == b["n_inliers"], a["early_exit"] == b["early_exit"],
              disp / upd if upd else 0.0, mark))


if __name__ == "__main__":
    main()
