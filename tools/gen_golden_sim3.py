"""Writes tests/golden/sim3/sim3_*.npz (a directory of its own: tests/test_golden.py owns the top level of tests/golden): hand-sized OptimizeSim3 problems solved by the numpy restatement tests/sim3_reference.py --
inputs, the LM trace of both optimize() calls (lambda, robust chi2, trials per iteration) and the outputs.

    python tools/gen_golden_sim3.py [name ...]          (all of them, or only the named ones)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import sim3_reference as R  # noqa: E402
import sim3_scenes as SC  # noqa: E402

CASES = {
    "sim3_rgbd_40": dict(n=40, seed=1201, fix_scale=True, outlier_frac=0.1),
    "sim3_mono_60": dict(n=60, seed=1202, fix_scale=False, outlier_frac=0.1),
    "sim3_early_exit_12": dict(n=12, seed=1203, fix_scale=True, outlier_frac=0.6),
}
# ... and three of sim3_scenes.IRREGULAR, by family name: map points behind camera 2, exactly ten survivors of the first inlier pass,
# edges with zero information
IRREGULAR_CASES = {"sim3_behind_camera_200": "behind_cam2", "sim3_ten_survive_15": "ten_survive", "sim3_zero_info_200": "zero_info"}


def problems(only):
    for name, kw in CASES.items():
        if not only or name in only:
            yield name, SC.scene(**kw)
    for name, family in IRREGULAR_CASES.items():
        if not only or name in only:
            (kw, edit), = [(kw, edit) for f, kw, edit in SC.IRREGULAR if f == family]
            yield name, SC.irregular_scene(kw, edit)


def main():
    for name, p in problems(sys.argv[1:]):
        o = R.optimize_sim3(p)
        tr = np.array(o["trace"], np.float64).reshape(-1, 3)
        np.savez_compressed(os.path.join(ROOT, "tests", "golden", "sim3", name + ".npz"),
                            T1w=p["T1w"], T2w=p["T2w"], Xw1=p["Xw1"], Xw2=p["Xw2"], obs1=p["obs1"], obs2=p["obs2"],
                            inv_sigma2_1=p["inv_sigma2_1"], inv_sigma2_2=p["inv_sigma2_2"], K1=p["K1"], K2=p["K2"],
                            q0=np.asarray(p["q"], np.float64), t0=np.asarray(p["t"], np.float64), s0=np.float64(p["s"]),
                            th2=np.float32(p["th2"]), fix_scale=np.int32(p["fix_scale"]),
                            q=o["q"], t=o["t"], s=np.float64(o["s"]), removed=o["removed"], n_inliers=np.int32(o["n_inliers"]),
                            iters=o["iters"], early_exit=np.int32(o["early_exit"]), trace_lambda=tr[:, 0], trace_chi2=tr[:, 1],
                            trace_trials=tr[:, 2].astype(np.int32))
        print(name, list(o["iters"]), o["n_inliers"], int(o["removed"].sum()), o["early_exit"])


if __name__ == "__main__":
    main()
