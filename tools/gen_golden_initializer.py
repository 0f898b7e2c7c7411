#!/usr/bin/env python3
"""Writes tests/golden/initializer/*.npz: three problems of tests/initializer_scenes.py with the yardstick's result (tests/initializer_reference.py, variant f64jacobi,
the double-sum score): one that takes the F branch, one that takes the H branch, one that leaves ReconstructH at the d1/d2 return.  tests/test_gpu_initializer.py
and smoke() hold the device to them: the outcome exactly, the motion and the points within the bands of tests/initializer_tolerances.py.  CPU only."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import initializer_reference as R      # noqa: E402
import initializer_scenes as SC         # noqa: E402

CASES = {
    "f_branch_n96": lambda: SC.scene(n=96, seed=101, iterations=64),
    "h_branch_n96": lambda: SC.scene(n=96, seed=111, planar=True, iterations=64),
    "pure_rotation_n96": lambda: SC.irregular("pure_rotation"),
}


def record(prob):
    r = R.initialize(prob, prob["sets"], "f64jacobi")
    return dict(keys1=prob["keys1"], keys2=prob["keys2"], matches12=prob["matches12"], K=np.array(prob["K"], np.float32), sigma=np.float32(prob["sigma"]),
                min_parallax=np.float32(prob["min_parallax"]), min_triangulated=np.int32(prob["min_triangulated"]), sets=prob["sets"],
                returned=np.bool_(r["returned"]), branch=np.int32(r["branch"]), best_h=np.int32(r["best_h"]), best_f=np.int32(r["best_f"]),
                degenerate=np.bool_(r["degenerate"]), no_model=np.bool_(r["no_model"]), SH=np.float32(r["SH"]), SF=np.float32(r["SF"]), RH=np.float32(r["RH"]),
                R21=r["R21"], t21=r["t21"], p3d=r["p3d"], triangulated=r["triangulated"], n_good=np.int32(r["n_good"]), parallax=np.float32(r["parallax"]))


def main():
    out = os.path.join(ROOT, "tests", "golden", "initializer")
    os.makedirs(out, exist_ok=True)
    for name, make in CASES.items():
        z = record(make())
        np.savez_compressed(os.path.join(out, name + ".npz"), **z)
        print(name, "returned", bool(z["returned"]), "branch", int(z["branch"]), "degenerate", bool(z["degenerate"]), "n_good", int(z["n_good"]))


if __name__ == "__main__":
    main()
