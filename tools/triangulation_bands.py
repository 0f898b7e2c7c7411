#!/usr/bin/env python3
"""Measures the triangulation yardstick (tests/triangulation_reference.py) against itself over the friendly scenes of tests/triangulation_scenes.py and writes
profiles/triangulation_bands.txt.  Variants compared with the base run (float64 eigh of A^T A, inputs as given):
  * the float32 one-sided Jacobi SVD (OpenCV's JacobiSVD) on the same inputs;
  * the base SVD on inputs of which EVERY float (keypoints, right coordinates, depths, raw keypoints, scale factors, level sigmas, poses, intrinsics) moved by one ulp up or down, seeds 0..3.
Recorded: the largest movement of x3D as a share of its distance to Ow1, over pairs that keep their branch; the largest movement of any comparison's signed
relative margin, over pairs whose base margin lies within NEAR of the comparison (a side far from its gate moves in proportion to its size and decides nothing).
tests/triangulation_tolerances.py is written from the `constant` lines (four times each band: the device sums in another order and solves with another Jacobi).
The point band is taken over all scenes (X3D_REL) and per scene (X3D_REL_<scene>): a float32 coordinate 100 m from the origin resolves 8e-6 m, so the far scene's
band is some 50 times that of the scenes at the origin, and a point check at the far scene's band would not bite on them;
tests/test_triangulation_reference_cpu.py keeps file, tolerances and this probe equal.

    python tools/triangulation_bands.py            # writes the profile
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import triangulation_reference as Y  # noqa: E402
import triangulation_scenes as S  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "triangulation_bands.txt")
NEAR = 0.5
FACTOR = 4
ULP_SEEDS = (0, 1, 2, 3)
FRAME_FLOATS = ("kp_x", "kp_y", "u_right", "depth", "raw_x", "raw_y")
LEVEL_FLOATS = ("scale_factors", "level_sigma2")      # (drawn from a generator of their own)
CAM_FLOATS = ("Rcw", "tcw", "Ow") + Y.CAMERA_SCALARS


def _ulp(rng, a):
    """every element one float32 ulp up or down (zeros and the -1 markers of `no stereo` / `no depth` keep their sign: they stay what they mark)"""
    a = np.asarray(a, np.float32)
    up = rng.random(a.shape) < 0.5
    moved = np.where(up, np.nextafter(a, np.float32(np.inf)), np.nextafter(a, np.float32(-np.inf))).astype(np.float32)
    keep = (a == 0) | (a == -1) | ~np.isfinite(a)
    return np.where(keep, a, moved).astype(np.float32)


def ulp_perturbed(sc, seed):
    rng, rng_levels = np.random.default_rng(9000 + seed), np.random.default_rng(19000 + seed)

    def frame(K):
        K = dict(K)
        for k in FRAME_FLOATS:
            if K.get(k) is not None:
                K[k] = _ulp(rng, K[k])
        for k in LEVEL_FLOATS:
            K[k] = _ulp(rng_levels, K[k])
        return K

    def cam(c):
        c = dict(c)
        for k in CAM_FLOATS:
            c[k] = _ulp(rng, c[k]) if np.ndim(c[k]) else np.float32(_ulp(rng, np.array([c[k]]))[0])
        return c
    out = dict(sc)
    out["K1"], out["cam1"] = frame(sc["K1"]), cam(sc["cam1"])
    out["K2s"], out["cams2"] = [frame(K) for K in sc["K2s"]], [cam(c) for c in sc["cams2"]]
    return out


def _run(sc, svd):
    return Y.triangulate_batch(sc["K1"], sc["cam1"], sc["K2s"], sc["cams2"], sc["match12"], sc["ratio_factor"], svd)[2]


def measure():
    """{'point': band, 'gate': band, 'rows': [(scene, variant, point, gate, verdict changes)]}"""
    rows = []
    for name, sc in S.all_scenes().items():
        if not sc["friendly"]:
            continue
        base = _run(sc, "eigh")
        variants = [("jacobi32", _run(sc, "jacobi32"))] + [("ulp seed %d" % s, _run(ulp_perturbed(sc, s), "eigh")) for s in ULP_SEEDS]
        Ow1 = np.asarray(sc["cam1"]["Ow"], np.float64)
        for vname, var in variants:
            pt = gt = 0.0
            flips = 0
            for b, v in zip(base, var):
                if len(b["idx1"]) == 0:
                    continue
                flips += int((b["pair_verdict"] != v["pair_verdict"]).sum())
                same = (b["branch"] == v["branch"]) & np.isin(b["branch"], Y.ACCEPTING)
                Xb, Xv = b["x3d"][b["idx1"]].astype(np.float64), v["x3d"][v["idx1"]].astype(np.float64)
                d = np.linalg.norm(Xb - Ow1, axis=1)
                if same.any():
                    pt = max(pt, float((np.linalg.norm(Xv - Xb, axis=1)[same] / d[same]).max()))
                with np.errstate(all="ignore"):
                    mb, mv = b["margins"], v["margins"]
                    near = np.isfinite(mb) & np.isfinite(mv) & (np.abs(mb) < NEAR)
                    if near.any():
                        gt = max(gt, float(np.abs(mv - mb)[near].max()))
            rows.append((name, vname, pt, gt, flips))
    by_scene = {}
    for r in rows:
        by_scene[r[0]] = max(by_scene.get(r[0], 0.0), r[2])
    return dict(point=max(r[2] for r in rows), gate=max(r[3] for r in rows), point_by_scene=by_scene, rows=rows)


def render(m):
    lines = ["# tools/triangulation_bands.py: the triangulation yardstick against itself (friendly scenes of tests/triangulation_scenes.py)",
             "# point: largest |dX| / |X - Ow1| over pairs that keep their branch; gate: largest movement of a signed relative margin within %.2f of its comparison" % NEAR,
             "# scene            variant        point        gate         verdicts changed"]
    for name, vname, pt, gt, flips in m["rows"]:
        lines.append("%-18s %-14s %.3e    %.3e    %d" % (name, vname, pt, gt, flips))
    lines.append("band point %.3e" % m["point"])
    lines.append("band gate %.3e" % m["gate"])
    lines.append("constant X3D_REL %.3e      # %d x band point" % (FACTOR * m["point"], FACTOR))
    lines.append("constant MARGIN_REL %.3e   # %d x band gate" % (FACTOR * m["gate"], FACTOR))
    for name, pt in m["point_by_scene"].items():
        lines.append("constant X3D_REL_%s %.3e   # %d x the scene's own point band" % (name, FACTOR * pt, FACTOR))
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    txt = render(measure())
    with open(OUT, "w") as f:
        f.write(txt)
    sys.stdout.write(txt)
