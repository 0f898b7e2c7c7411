#!/usr/bin/env python3
"""The yardstick's own bands on the OptimizeEssentialGraph families (tests/essential_graph_scenes.CASES): every case as generated, under
ulp_perturbed seeds 0..3 and under a permuted elimination order of the dense solve.  Per case: the largest displacement of the result
relative to the update, whether the iteration / trial counts moved, the relative spread of the last chi2.  Writes
profiles/essential_graph_bands.txt; tests/essential_graph_scenes.py (ITERS_UNSTABLE, BANDED) and tests/essential_graph_tolerances.py
(CHI2_LAST_SPREAD) are written from it and tests/test_essential_graph_reference_cpu.py keeps them equal to it.  CPU only."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import essential_graph_reference as R      # noqa: E402
import essential_graph_scenes as SC         # noqa: E402

ULP_SEEDS = (0, 1, 2, 3)


def probe(name, fs):
    """(band relative to the update, counts moved, relative chi2 spread, update) of one case."""
    prob = SC.case(name, fs)
    base = R.optimize_essential_graph(prob)
    upd = float(np.abs(base["Scw"] - np.asarray(prob["Scw"])).max())
    others = [R.optimize_essential_graph(SC.ulp_perturbed(prob, s)) for s in ULP_SEEDS]
    others.append(R.optimize_essential_graph(prob, perm=SC.permutation(prob, 0)))
    band = max(float(np.abs(o["Scw"] - base["Scw"]).max()) for o in others) / upd
    moved = any(o["lm_iterations"] != base["lm_iterations"] or list(o["trials"]) != list(base["trials"]) for o in others)
    chis = [float(o["chi2"][-1]) for o in others + [base]]
    spread = (max(chis) - min(chis)) / max(chis)
    return band, moved, spread, upd


def parse(path):
    """case id -> (band, moved, spread) of a bands file."""
    out = {}
    for line in open(path):
        f = line.split()
        if len(f) >= 5 and f[0] == "case":
            out[f[1]] = (float(f[2]), f[3] == "moved", float(f[4]))
    return out


def main():
    lines = ["# tools/essential_graph_bands.py: case <id> <band / update> <counts: moved | steady> <relative spread of the last chi2> <update>"]
    for (name, fs), cid in zip(SC.CASES, SC.case_ids()):
        band, moved, spread, upd = probe(name, fs)
        lines.append("case %s %.3e %s %.3e %.3e" % (cid, band, "moved" if moved else "steady", spread, upd))
        print(lines[-1], flush=True)
    rows = parse_lines(lines)
    lines.append("# largest band %.3e, largest chi2 spread %.3e, counts moved on: %s"
                 % (max(r[0] for r in rows.values()), max(r[2] for r in rows.values()), " ".join(k for k, r in rows.items() if r[1]) or "none"))
    with open(os.path.join(ROOT, "profiles", "essential_graph_bands.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


def parse_lines(lines):
    out = {}
    for line in lines:
        f = line.split()
        if len(f) >= 5 and f[0] == "case":
            out[f[1]] = (float(f[2]), f[3] == "moved", float(f[4]))
    return out


if __name__ == "__main__":
    main()
