"""Which OptimizeSim3 parity families are rounding-sensitive in the reference itself: each family is run through tests/sim3_reference.py
as generated and with every observation moved by one float32 ulp, and what changed is printed.

    python tools/sim3_chaotic_seeds.py > profiles/r07_sim3_chaotic_seeds.txt
        tests/sim3_scenes.FAMILIES, one perturbation: the evidence behind sim3_scenes.ITERS_UNSTABLE
    python tools/sim3_chaotic_seeds.py --irregular > profiles/sim3_irregular_bands.txt
        tests/sim3_scenes.IRREGULAR, ulp_perturbed seeds 0..3: the evidence behind IRREGULAR_ITERS_UNSTABLE and IRREGULAR_BANDED
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import sim3_reference as R  # noqa: E402
import sim3_scenes as SC  # noqa: E402
from lm_tolerances import UPDATE_REL  # noqa: E402

PROBE_SEEDS = (0, 1, 2, 3)


def update_norm(p, a):
    return max(np.abs(a["q"] - p["q"]).max(), np.abs(a["t"] - p["t"]).max(), abs(a["s"] - p["s"]))


def displacement(a, b):
    return max(np.abs(a["q"] - b["q"]).max(), np.abs(a["t"] - b["t"]).max(), abs(a["s"] - b["s"]))


def probe(p, seeds=PROBE_SEEDS):
    """The yardstick on p and on its one-ulp copies: (result, results of the copies, same removed / n_inliers / early_exit on every copy,
    iteration counts moved on some copy, largest displacement relative to the update)."""
    a = R.optimize_sim3(p)
    bs = [R.optimize_sim3(SC.ulp_perturbed(p, s)) for s in seeds]
    same = all(np.array_equal(a["removed"], b["removed"]) and a["n_inliers"] == b["n_inliers"] and a["early_exit"] == b["early_exit"] for b in bs)
    moved = any(list(a["iters"]) != list(b["iters"]) for b in bs)
    upd = update_norm(p, a)
    band = max(displacement(a, b) for b in bs) / upd if upd else 0.0
    return a, bs, same, moved, band


def main_families():
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


def main_irregular():
    print("family n seed | iters (as generated) | iters (one ulp, seeds 0..3) | removed | n_inliers | early_exit | removed, n_inliers, early_exit same"
          " | largest displacement / update")
    for name, kw, edit in SC.IRREGULAR:
        p = SC.irregular_scene(kw, edit)
        a, bs, same, moved, band = probe(p)
        mark = ("  ITERS MOVE" if moved else "") + ("  BANDED" if band > UPDATE_REL else "") + ("" if same else "  SCHEDULE MOVES")
        print("%-18s %5d %3d | %-7s | %-32s | %5d | %5d | %-5s | %s | %.2e%s" % (
            name, kw["n"], kw["seed"], list(map(int, a["iters"])), " ".join(str(list(map(int, b["iters"]))) for b in bs),
            int(a["removed"].sum()), a["n_inliers"], a["early_exit"], same, band, mark))


if __name__ == "__main__":
    main_irregular() if "--irregular" in sys.argv[1:] else main_families()
