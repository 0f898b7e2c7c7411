"""Stand-in keyframes for include/eaofusion/Sim3Solver.h: a flattened Sim3Solver problem (tests/sim3_solver_scenes.py) embedded in two keyframes among
entries the constructor's filters must skip, as the text tests/cpp/sim3_solver/sim3_solver_driver.cpp reads; the driver's counting generator restated;
and the three-candidate scene of the loop-closing test."""
import numpy as np

import sim3_solver_reference as R
import sim3_solver_scenes as SC

# the entries the constructor skips (src/Sim3Solver.cc:64-79)
NO_MATCH, NO_MP1, BAD_MP1, BAD_MP2, NOT_IN_KF1, NOT_IN_KF2 = 1, 2, 3, 4, 5, 6


def candidate_text(prob, seed=0, n_extra=None):
    """(scene block, index of each correspondence in vpMatched12, N1)"""
    rng = np.random.default_rng(seed)
    n = len(prob["Xw1"])
    n_extra = n // 3 + 6 if n_extra is None else n_extra
    kinds = np.array([0] * n + list(rng.integers(1, 7, n_extra)), np.int64)
    rng.shuffle(kinds)
    N1 = len(kinds)
    sig = SC.level_sigma2()
    level = {float(v): k for k, v in enumerate(sig)}
    pre = R.prepare(prob)
    pool, entries, keys1, keys2, index = [], [], [], [], []
    c = 0
    for i, kind in enumerate(kinds):
        if kind == 0:
            X1, X2, o1, o2 = prob["Xw1"][c], prob["Xw2"][c], level[float(prob["sigma2_1"][c])], level[float(prob["sigma2_2"][c])]
            uv1, uv2 = pre["im1"][c], pre["im2"][c]
            index.append(i)
            c += 1
        else:
            X1, X2, o1, o2 = rng.normal(size=3).astype(np.float32), rng.normal(size=3).astype(np.float32), int(rng.integers(0, 8)), int(rng.integers(0, 8))
            uv1 = uv2 = np.array([100.0, 100.0], np.float32)
        keys1.append((uv1[0], uv1[1], o1))       # key i of KF1 belongs to entry i
        mp1 = mt = -1
        if kind != NO_MP1:
            pool.append((X1, kind == BAD_MP1, -1 if kind == NOT_IN_KF1 else i, -1))
            mp1 = len(pool) - 1
        if kind != NO_MATCH:
            keys2.append((uv2[0], uv2[1], o2))
            pool.append((X2, kind == BAD_MP2, -1, -1 if kind == NOT_IN_KF2 else len(keys2) - 1))
            mt = len(pool) - 1
        entries.append((mp1, mt))
    assert c == n
    f = lambda a: " ".join("%.9g" % float(v) for v in np.asarray(a).ravel())       # noqa: E731
    lines = ["%d %d" % (N1, 1 if prob["fix_scale"] else 0), f(prob["K1"]) + " " + f(prob["K2"]), f(prob["T1w"]), f(prob["T2w"]), f(sig), str(len(pool))]
    lines += ["%s %d %d %d" % (f(X), int(bad), i1, i2) for X, bad, i1, i2 in pool]
    lines += ["%d %d" % e for e in entries]
    for keys in (keys1, keys2):
        lines.append(str(len(keys)))
        lines += ["%.9g %.9g %d" % (float(x), float(y), o) for x, y, o in keys]
    return "\n".join(lines) + "\n", index, N1


class CountingRandom:
    """the driver's standin::Random: a 64-bit LCG, RandomInt(min, max) = min + (state >> 33) % (max - min + 1)"""

    def __init__(self, seed):
        self.state, self.calls = int(seed), 0

    def __call__(self, lo, hi):
        self.calls += 1
        self.state = (self.state * 6364136223846793005 + 1442695040888963407) % (1 << 64)
        return lo + (self.state >> 33) % (hi - lo + 1)


def loop_scene(seed=12345):
    """Three candidates for ComputeSim3's loop: 12 correspondences (dropped at once: fewer than 20), 25 correspondences that are all outliers (mRansacMaxIts = 7:
    dropped in the second round, when its iterations are used up) and 100 correspondences with 60 % outliers, which closes in the fifth round under this seed
    (the yardstick over the same draw stream: 38 inliers at its 24th iteration, 96 draws in all)."""
    cands = [SC.scene(n=12, seed=6101, fix_scale=True), SC.scene(n=25, seed=6102, fix_scale=True, outlier_frac=1.0),
             SC.scene(n=100, seed=6111, fix_scale=True, outlier_frac=0.6)]
    return "3 %d\n" % seed + "".join(candidate_text(p, seed=6200 + k)[0] for k, p in enumerate(cands))
