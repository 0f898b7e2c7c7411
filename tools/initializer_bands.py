#!/usr/bin/env python3
"""The yardstick's own bands on the friendly Initializer families (tests/initializer_scenes.py): per family, the base run (variant f64) against the variants f32 and
f64jacobi and against the inputs under ulp_perturbed seeds 0..3 (variant f64),
  - the share of hypotheses whose system is conditioned: (s8 - s9) / s1 >= GAP_MIN for ComputeH21, s8 / s1 >= GAP_MIN for ComputeF21,
  - hf: the largest distance between H21i / F21i of conditioned hypotheses, each scaled to unit Frobenius norm, the sign free (the smaller of |a - b|, |a + b|),
  - chi: the largest |d chi-square| / gate over (conditioned hypothesis, pair, gate) triples whose chi-square lies within 10 % of its gate (the spread grows with the chi-square; it is read where a flag can turn),
  - rt / x3d: the largest |dR21|, |dt21| and |dX| / |X| of the returned motion and of the points triangulated in both runs,
  - in_margin: the share of (hypothesis, pair, gate) triples closer than MARGIN_REL to their gate,
  - same: whether both winners, branch, returned, the winning motion (matched by nearest (R, t)) are identical under every variant, perturbation and both score sums,
    and the distance of RH from the 0.40 of src/Initializer.cc:115.
HF_REL, MARGIN_REL, RT_REL and X3D_REL are lm_tolerances.CHAOTIC_BANDS_ALLOWED times the largest spread over the families; GAP_MIN is chosen here, with its reason.
Writes profiles/initializer_bands.txt and tests/initializer_tolerances.py (tests/test_initializer_reference_cpu.py keeps the two equal).  CPU only, the device is
never asked."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import initializer_reference as R      # noqa: E402
import initializer_scenes as SC         # noqa: E402
from lm_tolerances import CHAOTIC_BANDS_ALLOWED     # noqa: E402

ULP_SEEDS = (0, 1, 2, 3)
# A float32 SVD returns the singular vector of a value separated by a relative gap g to about eps32 / g: 6e-5 at g = 1e-3.  Below it the variants return different
# answers rather than different roundings of one (and the Jacobi solve of A^T A, which squares the gap, is at eps64 / g^2 = 2e-10 there: far inside).
GAP_MIN = 1e-3
NEAR_GATE = 1.1
CONDITIONED_MIN_SHARE = 0.90
IN_MARGIN_MAX_SHARE = 0.01
RH_CLEARANCE = 0.03


def ulp_perturbed(prob, seed):
    """every keypoint coordinate moved by -1, 0 or +1 ulp"""
    rng = np.random.default_rng(1000 + seed)
    p = dict(prob)
    for k in ("keys1", "keys2"):
        a = np.asarray(prob[k], np.float32)
        d = rng.integers(-1, 2, a.shape)
        p[k] = np.where(d > 0, np.nextafter(a, np.float32(np.inf)), np.where(d < 0, np.nextafter(a, np.float32(-np.inf)), a)).astype(np.float32)
    return p


def hf_dist(a, b):
    """per matrix: the largest entry of the difference of the unit-norm matrices, the sign free"""
    ua, ub = R.unit(a).reshape(len(a), -1), R.unit(b).reshape(len(b), -1)
    with np.errstate(all="ignore"):
        return np.minimum(np.abs(ua - ub).max(1), np.abs(ua + ub).max(1))


def motion_dist(Ra, ta, Rb, tb):
    return max(float(np.abs(np.asarray(Ra, np.float64) - Rb).max()), float(np.abs(np.asarray(ta, np.float64) - tb).max()))


def outcome(r):
    return (r["best_h"], r["best_f"], r["branch"], bool(r["returned"]), bool(r["no_model"]), bool(r["degenerate"]))


def same_motion(a, b, tol=1e-2):
    """the winning motion hypotheses of two runs are the same (R, t): the index order follows the SVD's signs and is not held"""
    if a["motion"] < 0 or b["motion"] < 0:
        return a["motion"] == b["motion"]
    Ra, ta = a["motions"][a["motion"]]
    Rb, tb = b["motions"][b["motion"]]
    return motion_dist(Ra, ta, Rb, tb) < tol


def probe(prob):
    sets = prob["sets"]
    base = R.initialize(prob, sets, "f64")
    cond_h, cond_f = base["hyp"]["gap_h"] >= GAP_MIN, base["hyp"]["gap_f"] >= GAP_MIN
    out = dict(n=len(prob["matches12"]), hyp=len(sets), cond_h=float(cond_h.mean()), cond_f=float(cond_f.mean()), hf=0.0, chi=0.0, rt=0.0, x3d=0.0, same=1,
               rh=float(base["RH"]), returned=int(base["returned"]), branch=int(base["branch"]))
    runs = [R.initialize(prob, sets, v) for v in ("f32", "f64jacobi")] + [R.initialize(ulp_perturbed(prob, s), sets, "f64") for s in ULP_SEEDS]
    floats = [R.initialize(prob, sets, "f64", how="float", pk=base["pk"], hyp=base["hyp"])]
    ratios = []
    for key, gate, cond in (("hyp_chi_H", R.CHI2_H, cond_h), ("hyp_chi_F", R.CHI2_F, cond_f)):
        with np.errstate(all="ignore"):
            b = base[key].astype(np.float64) / float(gate)
        ratios.append(b[np.isfinite(b)])
        for v in runs:
            with np.errstate(all="ignore"):
                w = v[key].astype(np.float64) / float(gate)
                near = (b > 1 / NEAR_GATE) & (b < NEAR_GATE) & np.isfinite(w) & cond[:, None, None]
            if near.any():
                out["chi"] = max(out["chi"], float(np.abs(b - w)[near].max()))
    for v in runs:
        for key, cond in (("H21", cond_h), ("F21", cond_f)):
            d = hf_dist(base["hyp"][key], v["hyp"][key])[cond]
            if len(d) and np.isfinite(d).any():
                out["hf"] = max(out["hf"], float(np.nanmax(d)))
        if base["returned"] and v["returned"]:
            out["rt"] = max(out["rt"], motion_dist(base["R21"], base["t21"], v["R21"], v["t21"]))
            both = (base["triangulated"] > 0) & (v["triangulated"] > 0)
            if both.any():
                X, Y = base["p3d"][both].astype(np.float64), v["p3d"][both].astype(np.float64)
                out["x3d"] = max(out["x3d"], float((np.linalg.norm(X - Y, axis=1) / np.linalg.norm(X, axis=1)).max()))
    for v in runs + floats:
        if outcome(v) != outcome(base) or not same_motion(base, v):
            out["same"] = 0
    out["ratios"] = np.concatenate(ratios)
    return out


def in_margin(o, margin_rel):
    return float((np.abs(o["ratios"] - 1) < margin_rel).mean()) if len(o["ratios"]) else 0.0


def line_of(name, o, margin_rel):
    return "family %s n %d hyp %d conditioned_h %.4f conditioned_f %.4f hf %.3e chi %.3e rt %.3e x3d %.3e in_margin %.5f same %d rh %.5f branch %d returned %d" % (
        name, o["n"], o["hyp"], o["cond_h"], o["cond_f"], o["hf"], o["chi"], o["rt"], o["x3d"], in_margin(o, margin_rel), o["same"], o["rh"], o["branch"], o["returned"])


def summary(probes):
    r = lambda k: float("%.3e" % (CHAOTIC_BANDS_ALLOWED * max(o[k] for o in probes.values())))      # noqa: E731
    return dict(GAP_MIN=GAP_MIN, HF_REL=r("hf"), MARGIN_REL=r("chi"), RT_REL=r("rt"), X3D_REL=r("x3d"))


def parse(path):
    fams, consts = {}, {}
    for line in open(path):
        f = line.split()
        if f and f[0] == "family":
            fams[f[1]] = {f[k]: float(f[k + 1]) for k in range(2, len(f), 2)}
        elif f and f[0] == "constant":
            consts[f[1]] = float(f[2])
    return fams, consts


TOLERANCES = '''"""The bounds of the Initializer parity tests (tests/test_gpu_initializer.py imports every number it uses from here; it carries no literal tolerance of its own).
All are the `constant` lines of profiles/initializer_bands.txt, written by tools/initializer_bands.py from the yardstick alone
(tests/test_initializer_reference_cpu.py keeps this file equal to that one and holds the conditions on the friendly families).  GENERATED by that tool."""

# Singular-value gap relative to s1 -- (s8 - s9) / s1 of ComputeH21's system, s8 / s1 of ComputeF21's -- below which a hypothesis is "ill-conditioned": a float32 SVD
# returns the null vector to about eps32 / gap, 6e-5 at this value.  Such a hypothesis is not compared with the yardstick's matrix; its flags and score are still held,
# bit for bit, to CheckHomography / CheckFundamental on the device's own matrix.
GAP_MIN = 1e-3

# H21i / F21i of conditioned hypotheses, scaled to unit Frobenius norm, the sign free: the largest spread between yardstick variants (f64 against f32 and f64jacobi;
# inputs under ulp-perturbation seeds 0..3) over the friendly families, times lm_tolerances.CHAOTIC_BANDS_ALLOWED = 4.
HF_REL = %(HF_REL).3e

# (hypothesis, pair, gate) triples whose chi-square lies closer than this to its gate, relative to the gate, are left out when flags are compared against the
# yardstick's OWN matrix: the largest |d chi-square| / gate between the same variants over triples near their gate, times 4.  CheckRT's gates likewise.
MARGIN_REL = %(MARGIN_REL).3e

# |dR21|, |dt21| (largest entry) of the returned motion between the same variants, times 4
RT_REL = %(RT_REL).3e

# |dX| / |X| of the points triangulated in both runs between the same variants, times 4
X3D_REL = %(X3D_REL).3e

# the conditions the scenes are held to (not measurements)
CONDITIONED_MIN_SHARE = %(CONDITIONED_MIN_SHARE).2f
IN_MARGIN_MAX_SHARE = %(IN_MARGIN_MAX_SHARE).2f
RH_CLEARANCE = %(RH_CLEARANCE).2f
'''


def main():
    probes = {}
    for name in SC.FRIENDLY:      # (the scene of the workload's size is run against these bands by the GPU test; it is not measured here)
        probes[name] = probe(SC.friendly(name))
        print(name, "done", flush=True)
    c = summary(probes)
    lines = ["# tools/initializer_bands.py: the yardstick (tests/initializer_reference.py) against itself; see the tool's docstring for the columns"]
    lines += [line_of(name, o, c["MARGIN_REL"]) for name, o in probes.items()]
    lines += ["constant %s %.3e" % (k, v) for k, v in c.items()]
    with open(os.path.join(ROOT, "profiles", "initializer_bands.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    with open(os.path.join(ROOT, "tests", "initializer_tolerances.py"), "w") as f:
        f.write(TOLERANCES % dict(c, CONDITIONED_MIN_SHARE=CONDITIONED_MIN_SHARE, IN_MARGIN_MAX_SHARE=IN_MARGIN_MAX_SHARE, RH_CLEARANCE=RH_CLEARANCE))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
