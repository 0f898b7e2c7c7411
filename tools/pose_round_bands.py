#!/usr/bin/env python3
"""The oracle's own bands on the PoseOptimization round scenes (tests/pose_scenes.py), from oracle/lm_cpu.cpp alone.  Every scene is run thirteen times: as built and
under the twelve one-ulp perturbations of its float32 inputs (pose_scenes.perturbed).  Per scene: do the outlier table, the return value and the round structure
survive all runs; the decided iterations per round (same trial count in all thirteen runs, counted from the start of the round); the largest relative spread of chi2
and of lambda over the decided iterations, base run against each other run; the band on the returned pose relative to the largest update.
The bounds of tests/test_gpu_pose_rounds.py are lm_tolerances.CHAOTIC_BANDS_ALLOWED = 4 times the largest spread over all scenes -- the device differs from the oracle by
the order of its sums, the runs from each other by input ulps -- and a scene whose own pose band exceeds UPDATE_REL is listed with that band.
Writes profiles/pose_round_bands.txt and the block between the two `pose rounds` marker lines of tests/lm_tolerances.py; tests/test_lm_tolerances.py keeps the two
equal.  CPU only:
    python3 tools/pose_round_bands.py            (a minute)
    python3 tools/pose_round_bands.py --search   (prints the candidate scenes the lists of tests/pose_scenes.py were picked from; writes nothing)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pose_scenes as S                                   # noqa: E402
from lm_tolerances import CHAOTIC_BANDS_ALLOWED, UPDATE_REL    # noqa: E402
from oracle import oracle as O                            # noqa: E402

BEGIN = "# ---- pose rounds: written by tools/pose_round_bands.py, do not edit (tests/test_lm_tolerances.py compares it with profiles/pose_round_bands.txt)"
END = "# ---- pose rounds: end"


def measure(n, prob):
    with np.errstate(all="ignore"):
        runs = S.oracle_runs(O, prob)
    dec = S.decided(runs)
    sc, sl = S.spread(runs, dec)
    t = runs[0]["trace"]
    return dict(stable=S.tables_agree(runs), dec=dec, lens=[e - s for s, e in S.rounds_of(t)], active=[int(x) for x in t["round_active"]], chi2=sc, lam=sl,
                band=S.pose_band(runs, prob), stats=S.stats(n, runs, dec))


def fmt(name, m):
    st = m["stats"]
    return "%-42s tables %-9s iterations %-16s decided %-16s level-0 edges %-22s chi2 spread %.3e  lambda spread %.3e  pose band %.3e  | trials 2-5: %d  6-9: %d  kRefresh rounds: %d" % (
        name, "same" if m["stable"] else "DIFFERENT", m["lens"], m["dec"], m["active"], m["chi2"], m["lam"], m["band"], st["few"], st["many"], st["refresh"])


def search():
    for n in S.FAR_OFF_N:
        for of in (0.0, 0.1, 0.3):
            for mf in (0.0, 0.3, 1.0):
                for seed in range(5000, 5008):
                    print(fmt("far_off n=%d seed=%d out=%g mono=%g" % (n, seed, of, mf), measure(n, S.far_off(n, seed, of, mf))), flush=True)
    for n in S.SCATTERED_N:
        for seed in range(60):
            print(fmt("scattered n=%d seed=%d" % (n, seed), measure(n, S.scattered(n, seed))), flush=True)
    # second sweep: round 1 ends on an accepted retrial in front of the end of its candidate batch (picked on the base run, then measured)
    for n in (200, 256, 257, 512, 513, 1024):
        for of in (0.0, 0.1, 0.3):
            for mf in (0.0, 0.3, 1.0):
                for seed in range(5072, 5272):
                    p = S.far_off(n, seed, of, mf)
                    with np.errstate(all="ignore"):
                        o = O.pose_optimization(p)
                    t = o["trace"]
                    st = S.stats(n, [o], [e - s for s, e in S.rounds_of(t)])
                    if 1 in st["refresh_rounds"]:
                        print(fmt("far_off n=%d seed=%d out=%g mono=%g" % (n, seed, of, mf), measure(n, p)), flush=True)


def main():
    O.build()
    if "--search" in sys.argv:
        return search()
    lines = ["# written by tools/pose_round_bands.py: the oracle's own thirteen runs (the problem as built + twelve one-ulp perturbations) on the scenes of tests/pose_scenes.py"]
    fam_c, fam_l, chaotic = {}, {}, {}
    for name, (family, fn, args) in S.all_scenes().items():
        prob = fn(*args)
        m = measure(len(prob["points"]), prob)
        lines.append(fmt(name, m))
        fam_c[family] = max(fam_c.get(family, 0.0), m["chi2"])
        fam_l[family] = max(fam_l.get(family, 0.0), m["lam"])
        if m["band"] > UPDATE_REL:
            chaotic[name] = m["band"]
    for family in fam_c:
        lines.append("family %-12s largest chi2 spread %.3e  largest lambda spread %.3e" % (family, fam_c[family], fam_l[family]))
    consts = [("POSE_ROUNDS_CHI2_REL", CHAOTIC_BANDS_ALLOWED * max(fam_c.values()), "%d x the largest chi2 spread" % CHAOTIC_BANDS_ALLOWED),
              ("POSE_ROUNDS_LAMBDA_REL", CHAOTIC_BANDS_ALLOWED * max(fam_l.values()), "%d x the largest lambda spread" % CHAOTIC_BANDS_ALLOWED)]
    for name, band in chaotic.items():
        consts.append(("POSE_ROUNDS_CHAOTIC_BAND[%r]" % name, band, "the scene's own pose band exceeds UPDATE_REL = %g" % UPDATE_REL))
    for key, val, why in consts:
        lines.append("constant %s = %.3e        # %s" % (key, val, why))
    with open(os.path.join(ROOT, "profiles", "pose_round_bands.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    block = [BEGIN,
             "# chi2 and lambda of a DECIDED iteration (same trial count in the oracle's thirteen runs) of the scenes of tests/pose_scenes.py, relative; chi2 relative to",
             "# max(chi2, pose_scenes.CHI2_FLOOR).  Values that are not finite (zero_depth: chi2 is inf in every run) must be the same value.",
             "# POSE_ROUNDS_CHAOTIC_BAND: scenes whose returned pose moves by more than UPDATE_REL of the update among the oracle's own runs -- held to CHAOTIC_BANDS_ALLOWED x this",
             "# band instead; at most a quarter of the scenes may be listed (tests/test_pose_scenes_cpu.py)",
             "POSE_ROUNDS_CHAOTIC_BAND = {}"]
    block += ["%s = %.3e" % (key, val) for key, val, _ in consts]
    block.append(END)
    path = os.path.join(ROOT, "tests", "lm_tolerances.py")
    src = open(path).read()
    if BEGIN in src:
        src = src[:src.index(BEGIN)] + "\n".join(block) + src[src.index(END) + len(END):]
    else:
        src = src.rstrip("\n") + "\n\n" + "\n".join(block) + "\n"
    with open(path, "w") as f:
        f.write(src)
    print("\n".join(lines))


if __name__ == "__main__":
    main()
