#!/usr/bin/env python3
"""Writes tests/golden/triangulation/{inputs,verdicts,points}.npz: the stereo_mix scene of tests/triangulation_scenes.py, the yardstick's verdicts and its points.
They freeze this repository's restatement (tests/triangulation_reference.py), not a run of the reference.

    python tools/gen_golden_triangulation.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import triangulation_reference as Y  # noqa: E402
import triangulation_scenes as S  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "triangulation")
FRAME_KEYS = ("kp_x", "kp_y", "kp_octave", "u_right", "depth", "raw_x", "raw_y", "scale_factors", "level_sigma2")
CAM_KEYS = ("Rcw", "tcw", "Ow") + Y.CAMERA_SCALARS


def pack(sc):
    """the scene as flat arrays (frame k = 0 is keyframe 1, k >= 1 neighbour k - 1)"""
    a = {"match12": sc["match12"], "ratio_factor": np.float32(sc["ratio_factor"]), "n_nb": np.int32(len(sc["K2s"]))}
    for k, (K, c) in enumerate(zip([sc["K1"]] + sc["K2s"], [sc["cam1"]] + sc["cams2"])):
        for key in FRAME_KEYS:
            src = key if K.get(key) is not None else {"raw_x": "kp_x", "raw_y": "kp_y"}[key]      # (no mvKeys of its own: they equal mvKeysUn)
            a["f%d_%s" % (k, key)] = np.asarray(K[src])
        for key in CAM_KEYS:
            a["c%d_%s" % (k, key)] = np.asarray(c[key], np.float32)
    return a


def unpack(z):
    n_nb = int(z["n_nb"])
    frames = [{key: z["f%d_%s" % (k, key)] for key in FRAME_KEYS} for k in range(n_nb + 1)]
    cams = [{key: z["c%d_%s" % (k, key)] for key in CAM_KEYS} for k in range(n_nb + 1)]
    return dict(K1=frames[0], cam1=cams[0], K2s=frames[1:], cams2=cams[1:], match12=z["match12"], ratio_factor=np.float32(z["ratio_factor"]))


def build():
    sc = S.all_scenes()["stereo_mix"]
    v, x, _ = Y.triangulate_batch(sc["K1"], sc["cam1"], sc["K2s"], sc["cams2"], sc["match12"], sc["ratio_factor"])
    return {"inputs.npz": pack(sc), "verdicts.npz": {"verdict": v}, "points.npz": {"x3d": x}}


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    for fn, arrays in build().items():
        np.savez_compressed(os.path.join(OUT, fn), **arrays)
        print("wrote", fn, os.path.getsize(os.path.join(OUT, fn)), "bytes")
