#!/usr/bin/env python3
"""The yardstick's own bands on the Sim3Solver families (tests/sim3_solver_scenes.py): per family, over all its hypotheses,
  - the relative eigen-gap (l1 - l2) / (|l1| + |l4|) of N: smallest, first decile, median, and the share of hypotheses at or above GAP_MIN ("conditioned"),
  - the largest |dT12| / max |T12| on conditioned hypotheses between yardstick variants: the float64 eigh against the float32 Jacobi eigen solve, and the inputs
    under ulp_perturbed seeds 0..3,
  - the largest |d err| / gate between the same variants over (conditioned hypothesis, correspondence) pairs whose error lies within a factor 4 of its gate,
  - the smallest relative margin |err - gate| / gate over all (hypothesis, correspondence) pairs, and the share of pairs inside MARGIN_REL.
T12_REL and MARGIN_REL are 4 x (lm_tolerances.CHAOTIC_BANDS_ALLOWED) the largest spread over all families; GAP_MIN is chosen here, with its reason.  Writes
profiles/sim3_solver_bands.txt; tests/sim3_solver_tolerances.py is written from it and tests/test_sim3_solver_reference_cpu.py keeps the two equal.  CPU only."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sim3_solver_reference as R      # noqa: E402
import sim3_solver_scenes as SC         # noqa: E402
from lm_tolerances import CHAOTIC_BANDS_ALLOWED     # noqa: E402

ULP_SEEDS = (0, 1, 2, 3)
# A float32 eigen solve of a symmetric matrix whose top eigenvalue is separated by a relative gap g returns the eigenvector to about eps32 / g.  At g = 1e-3 that is
# 6e-5, the order of the spread this file records; below it the variants return different answers rather than different roundings of one.
GAP_MIN = 1e-3
NEAR_GATE = 4.0


def rel_gap(ev):
    """(l1 - l2) / (|l1| + |l4|) per hypothesis; NaN where N is zero or not finite"""
    ev = np.asarray(ev, np.float64).reshape(-1, 4)
    with np.errstate(all="ignore"):
        return (ev[:, 0] - ev[:, 1]) / (np.abs(ev[:, 0]) + np.abs(ev[:, 3]))


def conditioned(ev):
    with np.errstate(all="ignore"):
        return rel_gap(ev) >= GAP_MIN          # NaN: not conditioned


def t_spread(a, b):
    """|dT| / max |T| per hypothesis (NaN where either is not finite)"""
    with np.errstate(all="ignore"):
        a, b = np.asarray(a, np.float64).reshape(len(a), -1), np.asarray(b, np.float64).reshape(len(b), -1)
        return np.abs(a - b).max(axis=1) / np.abs(a).max(axis=1)


def margins(pre, T12, T21):
    """|err - gate| / gate of both errors per correspondence (inf where the gate is 0), and the errors over the gates"""
    e1, e2 = R.errors(pre, T12, T21)
    with np.errstate(all="ignore"):
        r1, r2 = e1.astype(np.float64) / pre["max1"], e2.astype(np.float64) / pre["max2"]
    return r1, r2


def probe(make):
    """one family: dict of the figures above (before MARGIN_REL is known: `margin_all` holds every finite margin)"""
    prob, triples = make()
    pre = R.prepare(prob)
    n, nh = pre["n"], len(triples)
    out = dict(n=n, n_hyp=nh, gaps=np.zeros(0), cond=0, t_eigen=0.0, t_ulp=0.0, e_eigen=0.0, e_ulp=0.0, margin_all=np.zeros(0))
    if n < SC.MIN_INLIERS or nh == 0:
        return out
    base = R.iterate(prob, None, triples, max_its=nh, min_inliers=n, eigen="f64", pre=pre)     # min_inliers = n: never returns, every hypothesis is evaluated
    cond = conditioned(base["hyp_eigenvalues"])
    out["gaps"], out["cond"] = rel_gap(base["hyp_eigenvalues"]), int(cond.sum())
    variants = [("eigen", R.iterate(prob, None, triples, max_its=nh, min_inliers=n, eigen="f32jacobi", pre=pre), pre)]
    for s in ULP_SEEDS:
        pp = SC.ulp_perturbed(prob, s)
        ppre = R.prepare(pp)
        variants.append(("ulp", R.iterate(pp, None, triples, max_its=nh, min_inliers=n, eigen="f64", pre=ppre), ppre))
    base_r = [margins(pre, base["hyp_T12"][h], base["hyp_T21"][h]) for h in range(nh)]
    for kind, var, vpre in variants:
        sp = np.maximum(t_spread(base["hyp_T12"], var["hyp_T12"]), t_spread(base["hyp_T21"], var["hyp_T21"]))
        if cond.any() and np.isfinite(sp[cond]).any():
            out["t_" + kind] = max(out["t_" + kind], float(np.nanmax(sp[cond])))
        for h in np.nonzero(cond)[0]:
            vr = margins(vpre, var["hyp_T12"][h], var["hyp_T21"][h])
            for b, v in zip(base_r[h], vr):
                with np.errstate(all="ignore"):
                    near = (b > 1 / NEAR_GATE) & (b < NEAR_GATE) & np.isfinite(v)
                    if near.any():
                        out["e_" + kind] = max(out["e_" + kind], float(np.abs(b - v)[near].max()))
    m = np.concatenate([np.abs(np.concatenate(base_r[h]) - 1) for h in range(nh)])
    out["margin_all"] = m[np.isfinite(m)]
    return out


def line_of(name, o, margin_rel):
    g = o["gaps"][np.isfinite(o["gaps"])]
    q = (lambda p: float(np.percentile(g, p))) if len(g) else (lambda p: float("nan"))
    m = o["margin_all"]
    return "family %s n %d hyp %d conditioned %d gap_min %.3e gap_p10 %.3e gap_median %.3e t12_eigen %.3e t12_ulp %.3e err_eigen %.3e err_ulp %.3e margin_min %.3e in_margin %.5f" % (
        name, o["n"], o["n_hyp"], o["cond"], q(0), q(10), q(50), o["t_eigen"], o["t_ulp"], o["e_eigen"], o["e_ulp"],
        float(m.min()) if len(m) else float("nan"), float((m < margin_rel).mean()) if len(m) else 0.0)


def summary(probes):
    t12 = max(max(o["t_eigen"], o["t_ulp"]) for o in probes.values())
    err = max(max(o["e_eigen"], o["e_ulp"]) for o in probes.values())
    return float("%.3e" % (CHAOTIC_BANDS_ALLOWED * t12)), float("%.3e" % (CHAOTIC_BANDS_ALLOWED * err))


def parse(path):
    """(family -> dict of its figures, dict(GAP_MIN, T12_REL, MARGIN_REL)) of a bands file"""
    fams, consts = {}, {}
    for line in open(path):
        f = line.split()
        if f and f[0] == "family":
            fams[f[1]] = {f[k]: float(f[k + 1]) for k in range(2, len(f), 2)}
        elif f and f[0] == "constant":
            consts[f[1]] = float(f[2])
    return fams, consts


def main():
    probes = {}
    for name, make in SC.all_families():
        probes[name] = probe(make)
        print(name, "done", flush=True)
    t12_rel, margin_rel = summary(probes)
    lines = ["# tools/sim3_solver_bands.py: the yardstick (tests/sim3_solver_reference.py) against itself; see the tool's docstring for the columns"]
    lines += [line_of(name, o, margin_rel) for name, o in probes.items()]
    lines += ["constant GAP_MIN %.3e" % GAP_MIN, "constant T12_REL %.3e" % t12_rel, "constant MARGIN_REL %.3e" % margin_rel]
    with open(os.path.join(ROOT, "profiles", "sim3_solver_bands.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
