"""Writes tests/golden/sim3_solver/sim3_solver_*.npz: a few Sim3Solver problems, their triples and what the numpy restatement
tests/sim3_solver_reference.py returns for them (float64 eigh variant).  Of each family's drawn stream only hypotheses are kept that are conditioned
(tests/sim3_solver_tolerances.GAP_MIN) and have no correspondence inside MARGIN_REL of a gate, so that flags and counts are exact expectations.

    python tools/gen_golden_sim3_solver.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import sim3_solver_reference as R  # noqa: E402
import sim3_solver_scenes as SC  # noqa: E402
from sim3_solver_tolerances import GAP_MIN, MARGIN_REL  # noqa: E402

# name -> (family, hypotheses kept)
CASES = {"sim3_solver_n64_fs1": ("n64-fs1", 5), "sim3_solver_n21_fs0": ("n21-fs0", 6), "sim3_solver_n257_fs0": ("n257-fs0", 8),
         "sim3_solver_pure_translation": ("pure_translation", 7)}


def clear_of_the_gates(pre, h):
    e1, e2 = R.errors(pre, h["T12"], h["T21"])
    with np.errstate(all="ignore"):
        m = np.minimum(np.abs(e1.astype(np.float64) / pre["max1"] - 1), np.abs(e2.astype(np.float64) / pre["max2"] - 1))
    return not (m < MARGIN_REL).any()


def main():
    for name, (family, keep) in CASES.items():
        prob, triples = dict(SC.all_families())[family]()
        pre = R.prepare(prob)
        kept = []
        for tr in triples:
            h = R.compute_sim3(pre["X1c"][tr].T, pre["X2c"][tr].T, pre["fix_scale"])
            ev = h["eigenvalues"]
            if (ev[0] - ev[1]) / (abs(ev[0]) + abs(ev[3])) >= GAP_MIN and (np.isnan(h["T12"]).any() or clear_of_the_gates(pre, h)):
                kept.append(tr)
        assert len(kept) >= keep, (name, len(kept))
        tri = np.array(kept[:keep], np.int32)
        o = R.iterate(prob, None, tri, min_inliers=SC.MIN_INLIERS, max_its=300, pre=pre)
        n_eval = o["state"]["iterations"]
        assert n_eval == len(tri) or o["returned"] == n_eval - 1
        # the inspection arrays cover every hypothesis of the chunk, also those after a return (the device evaluates them all)
        full = R.iterate(prob, None, tri, min_inliers=pre["n"], max_its=300, pre=pre)
        np.savez_compressed(os.path.join(ROOT, "tests", "golden", "sim3_solver", name + ".npz"),
                            T1w=prob["T1w"], T2w=prob["T2w"], Xw1=prob["Xw1"], Xw2=prob["Xw2"], sigma2_1=prob["sigma2_1"], sigma2_2=prob["sigma2_2"],
                            K1=np.asarray(prob["K1"], np.float32), K2=np.asarray(prob["K2"], np.float32), fix_scale=np.int32(prob["fix_scale"]),
                            triples=tri, min_inliers=np.int32(SC.MIN_INLIERS), max_its=np.int32(300),
                            hyp_inliers=full["hyp_inliers"], hyp_T12=full["hyp_T12"], hyp_T21=full["hyp_T21"], hyp_inlier=full["hyp_inlier"],
                            returned=np.int32(o["returned"]), n_inliers=np.int32(o["n_inliers"]), no_more=np.int32(o["no_more"]), T12=o["T12"],
                            inlier=o["inlier"], iterations=np.int32(o["state"]["iterations"]), best_inliers=np.int32(o["state"]["best_inliers"]))
        print(name, "n", pre["n"], "counts", list(full["hyp_inliers"]), "returned", o["returned"], "iterations", o["state"]["iterations"])


if __name__ == "__main__":
    main()
