#!/usr/bin/env python3
"""Writes tests/golden/essential_graph/ring300_fs{0,1}.npz: the yardstick's result (tests/essential_graph_reference.py) on the 300-keyframe ring of
essential_graph_scenes.FAMILIES, which takes several seconds to compute -- too long for a GPU test case.  tests/test_essential_graph_reference_cpu.py re-derives
the files.  CPU only."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import essential_graph_reference as R      # noqa: E402
import essential_graph_scenes as SC         # noqa: E402

GOLDEN_CASES = [("ring300", False), ("ring300", True)]


def main():
    out = os.path.join(ROOT, "tests", "golden", "essential_graph")
    os.makedirs(out, exist_ok=True)
    for name, fs in GOLDEN_CASES:
        prob = SC.case(name, fs)
        o = R.optimize_essential_graph(prob)
        np.savez_compressed(os.path.join(out, "%s_fs%d.npz" % (name, int(fs))), Scw_in=prob["Scw"], edges=prob["edges"], Scw=o["Scw"],
                            lm_iterations=o["lm_iterations"], trials=o["trials"], chi2=o["chi2"], chi2_initial=o["chi2_initial"], n_active=o["n_active"])
        print(name, fs, o["lm_iterations"], list(o["trials"]))


if __name__ == "__main__":
    main()
