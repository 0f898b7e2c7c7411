"""Writes tests/golden/pnp_solver/<family>.npz: a few PnPsolver problems of tests/pnp_solver_scenes.py, their sets and what the numpy restatement
tests/pnp_solver_reference.py (jacobi variant) returns for them: every hypothesis' pose, reprojection errors, choice, error2 per correspondence, flags and count,
which hypotheses are CONDITIONED (the yardstick's own runs agree on the pose within pnp_solver_tolerances.RT_BOUND), and the outcome of iterate.  Data only.

    python tools/gen_golden_pnp_solver.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pnp_solver_reference as Y  # noqa: E402
import pnp_solver_scenes as SC  # noqa: E402
from pnp_solver_tolerances import RT_BOUND  # noqa: E402

CASES = SC.PARITY + ["x4_n100"]


def record(name):
    c = SC.FAMILIES[name]()
    prob = c["prob"]
    rs = SC.yardstick_runs(c)
    cond = SC.pose_spread(rs) <= RT_BOUND
    h = rs[2]      # jacobi
    o = Y.iterate(prob, None, c["sets"], c["min_inliers"], c["max_its"], "jacobi", hyp=h)
    return dict(p3d_w=prob["p3d_w"], p2d=prob["p2d"], sigma2=prob["sigma2"], K=np.asarray(prob["K"], np.float32), th2=np.float32(prob["th2"]), sets=c["sets"],
                min_inliers=np.int32(c["min_inliers"]), max_its=np.int32(c["max_its"]), true_inlier=c["true_inlier"].astype(np.uint8),
                hyp_R=h["R"], hyp_t=h["t"], hyp_rep_err=h["rep"], hyp_choice=h["choice"], hyp_inliers=h["inliers"], hyp_inlier=h["inlier"], hyp_err=h["err"],
                conditioned=cond.astype(np.uint8), returned=np.int32(o["returned"]), refined=np.int32(o["refined"]), n_inliers=np.int32(o["n_inliers"]),
                no_more=np.int32(o["no_more"]), Tcw=o["Tcw"], inlier=o["inlier"], records=np.array(o["records"], np.int32),
                iterations=np.int32(o["state"]["iterations"]), best_inliers=np.int32(o["state"]["best_inliers"]))


def main():
    os.makedirs(os.path.join(ROOT, "tests", "golden", "pnp_solver"), exist_ok=True)
    for name in CASES:
        g = record(name)
        np.savez_compressed(os.path.join(ROOT, "tests", "golden", "pnp_solver", name + ".npz"), **g)
        print(name, "n", len(g["sigma2"]), "counts", list(g["hyp_inliers"]), "conditioned", int(g["conditioned"].sum()), "returned", int(g["returned"]), "refined", int(g["refined"]))


if __name__ == "__main__":
    main()
