#!/usr/bin/env python3
"""The yardstick's own bands on the PnPsolver families (tests/pnp_solver_scenes.py), from tests/pnp_solver_reference.py alone: its three eigen-solve variants
(eigh, svd, jacobi) against each other, and every float input moved one ulp up or down (ulp_perturbed seeds 0..3).  Per family, over all its hypotheses:
  - the pose spread: the largest |dR|, |dt| (absolute; R is a rotation and t is in metres of a 2 .. 8 m scene) between the base run (eigh) and each other run,
  - the largest |d error2| / gate between the same runs over (conditioned hypothesis, correspondence) pairs whose error lies within a factor 4 of its gate,
  - the largest |d rep_error| (pixels) of the two smallest of a hypothesis' three reprojection errors (the two the choice of N turns on; the third can belong to a
    solution that is far off, and then moves by hundreds of pixels) between the same runs on conditioned hypotheses,
  - the share of (hypothesis, correspondence) pairs inside MARGIN_REL.
The pose spread has a heavy tail: a sampled set that holds an outlier is inconsistent data, and EPnP's answer on it moves by up to 1e-3 under one ulp.  The tests
let at most UNCONDITIONED_MAX_SHARE = 5 % of the hypotheses of a min_set >= 6 family be unconditioned, so the measured value behind RT_BOUND is the spread that
95 % of all min_set >= 6 hypotheses stay inside (the 95th percentile), and a hypothesis is CONDITIONED when its own spread is within RT_BOUND.  Every bound is
lm_tolerances.CHAOTIC_BANDS_ALLOWED = 4 times its measured value: one float-rounding choice on the device may differ from every run here.
The min_set = 4 families are measured too, to show what the issue states: there the variants disagree by O(1).
Writes profiles/pnp_solver_bands.txt and tests/pnp_solver_tolerances.py; tests/test_pnp_solver_reference_cpu.py keeps the two equal.  CPU only."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pnp_solver_reference as Y      # noqa: E402
import pnp_solver_scenes as SC         # noqa: E402
from lm_tolerances import CHAOTIC_BANDS_ALLOWED     # noqa: E402

ULP_SEEDS = SC.ULP_SEEDS
runs, pose_spread = SC.yardstick_runs, SC.pose_spread
NEAR_GATE = 4.0
UNCONDITIONED_MAX_SHARE = 0.05
IN_MARGIN_MAX_SHARE = 0.01
MIN4_DISAGREE_MIN_SHARE = 0.25


def measure(case, rs, rt_bound):
    """(error spread near the gate / gate, rep_error spread) over the conditioned hypotheses of a case"""
    gate = Y.max_error(case["prob"]).astype(np.float64)
    cond = pose_spread(rs) <= rt_bound
    base = rs[0]
    e_sp, r_sp = 0.0, 0.0
    for a in rs[1:]:
        with np.errstate(all="ignore"):
            near = (base["err"] > gate / NEAR_GATE) & (base["err"] < gate * NEAR_GATE) & cond[:, None]
            d = np.abs(a["err"] - base["err"]) / gate
            if near.any():
                e_sp = max(e_sp, float(np.nanmax(d[near])))
            if cond.any():
                r_sp = max(r_sp, float(np.nanmax(np.abs(np.sort(a["rep"], axis=1)[:, :2] - np.sort(base["rep"], axis=1)[:, :2])[cond])))
    return e_sp, r_sp, cond


def in_margin_share(case, rs, margin):
    gate = Y.max_error(case["prob"]).astype(np.float64)
    with np.errstate(all="ignore"):
        return float((np.abs(rs[0]["err"] - gate) <= margin * gate).mean())


def main():
    lines = ["# written by tools/pnp_solver_bands.py: the yardstick's own bands (variants eigh / svd / jacobi; ulp_perturbed seeds %s)" % (ULP_SEEDS,)]
    all_runs = {name: runs(SC.FAMILIES[name]()) for name in SC.PARITY + SC.MIN4}
    spreads = np.concatenate([pose_spread(all_runs[name]) for name in SC.PARITY])
    p95 = float(np.quantile(spreads, 1.0 - UNCONDITIONED_MAX_SHARE, method="higher"))
    rt_bound = CHAOTIC_BANDS_ALLOWED * p95
    lines.append("pose spread over the %d hypotheses of the min_set >= 6 families: median %.3e, 95th percentile %.3e, largest %.3e" % (len(spreads), np.median(spreads), p95, spreads.max()))
    e_max, r_max = 0.0, 0.0
    for name in SC.PARITY:
        case = SC.FAMILIES[name]()
        e_sp, r_sp, cond = measure(case, all_runs[name], rt_bound)
        sp = pose_spread(all_runs[name])
        var = pose_spread(all_runs[name], all_runs[name][1:3])
        e_max, r_max = max(e_max, e_sp), max(r_max, r_sp)
        lines.append("family %-16s hypotheses %3d  conditioned %3d  spread: variants %.3e  all runs median %.3e max %.3e   |d err|/gate near the gate %.3e   |d rep| %.3e px"
                     % (name, len(sp), int(cond.sum()), var.max(), np.median(sp), sp.max(), e_sp, r_sp))
    margin = CHAOTIC_BANDS_ALLOWED * e_max
    rep_band = CHAOTIC_BANDS_ALLOWED * r_max
    for name in SC.PARITY:
        lines.append("family %-16s share of (hypothesis, correspondence) pairs inside MARGIN_REL: %.4f" % (name, in_margin_share(SC.FAMILIES[name](), all_runs[name], margin)))
    for name in SC.MIN4:
        var = pose_spread(all_runs[name], all_runs[name][1:3])
        lines.append("family %-16s (min_set 4) hypotheses %3d  variants disagree beyond RT_BOUND on %3d (share %.2f), median spread %.3e"
                     % (name, len(var), int((var > rt_bound).sum()), float((var > rt_bound).mean()), np.median(var)))
    lines.append("constant RT_BOUND = %.3e        # %d x the 95th percentile of the pose spread" % (rt_bound, CHAOTIC_BANDS_ALLOWED))
    lines.append("constant MARGIN_REL = %.3e       # %d x the largest |d err| / gate near the gate" % (margin, CHAOTIC_BANDS_ALLOWED))
    lines.append("constant REP_BAND = %.3e         # %d x the largest |d rep_error|, pixels" % (rep_band, CHAOTIC_BANDS_ALLOWED))
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "pnp_solver_bands.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    with open(os.path.join(ROOT, "tests", "pnp_solver_tolerances.py"), "w") as f:
        f.write('''"""The bounds of the PnPsolver parity tests (tests/test_gpu_pnp_solver.py and tests/test_pnp_solver_reference_cpu.py import every number they use from here).
The first three are the `constant` lines of profiles/pnp_solver_bands.txt, written by tools/pnp_solver_bands.py from the yardstick alone
(tests/test_pnp_solver_reference_cpu.py keeps this file equal to that one and holds the conditions on the families)."""

# |dR|, |dt| (absolute) of a pose on a conditioned hypothesis.  A hypothesis is CONDITIONED when the yardstick's own runs -- its three eigen-solve variants, its inputs
# under ulp_perturbed seeds 0..3 -- agree on its pose within this bound; 4 x the spread that 95 %% of the hypotheses of the min_set >= 6 families stay inside.
RT_BOUND = %.3e

# (hypothesis, correspondence) pairs whose error2 lies closer than this to its gate, relative to the gate, are left out when flags are compared against the
# yardstick's OWN pose: 4 x the largest |d error2| / gate between the same runs over pairs near their gate.
MARGIN_REL = %.3e

# hyp_choice is compared where the yardstick's two smallest reprojection errors differ by more than this (pixels): 4 x the largest |d rep_error| of those two between the runs.
REP_BAND = %.3e

# the conditions the scenes are held to (set by the issue, not measured)
UNCONDITIONED_MAX_SHARE = %.2f      # of the hypotheses of a min_set >= 6 family
IN_MARGIN_MAX_SHARE = %.2f          # of its (hypothesis, correspondence) pairs
MIN4_DISAGREE_MIN_SHARE = %.2f      # of the hypotheses of a min_set = 4 family on which the variants disagree beyond RT_BOUND: why no per-hypothesis parity is asked there
''' % (rt_bound, margin, rep_band, UNCONDITIONED_MAX_SHARE, IN_MARGIN_MAX_SHARE, MIN4_DISAGREE_MIN_SHARE))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
