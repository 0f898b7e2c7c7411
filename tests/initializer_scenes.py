"""Two-view scenes for the Initializer tests: a 640 x 480 camera, points seen from a reference and a current pose, keypoints with noise and outliers, unmatched
keypoints on both sides (Normalize runs over all of them), the pairs ascending in `first`, and the sets of a seeded draw loop.

Friendly families (end-to-end parity): `general` (3-D scene, F branch, returns true) and `planar` (H branch, returns true), 0.5 px noise and 15 % outliers.
Irregular families: IRREGULAR, each with the line of src/Initializer.cc it is built to reach."""
import numpy as np

import initializer_reference as R

f32 = np.float32
K = (500.0, 500.0, 320.0, 240.0)
W, H = 640.0, 480.0


def _rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    return (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))


def _project(X):
    return np.stack([K[0] * X[:, 0] / X[:, 2] + K[2], K[1] * X[:, 1] / X[:, 2] + K[3]], 1)


def sets_of(n, iterations, seed):
    rng = np.random.default_rng(seed)
    return R.draw_sets(n, iterations, lambda lo, hi: int(rng.integers(lo, hi + 1)))


def scene(n, seed, planar=False, noise=0.5, outliers=0.15, rot=(0.02, -0.03, 0.01), t=(0.9, 0.1, 0.15), extra=40, far=False, sigma=1.0, iterations=48,
          min_parallax=None, min_triangulated=None, plane=(0.25, 0.15), depth=(4.0, 12.0), extra2=None):
    """n matched pairs.  Returns the problem dict of eao_fusion_amd.initializer.initialize with `sets` and the truth (R, t, plane) beside it."""
    rng = np.random.default_rng(seed)
    Rm, tv = _rot(*rot), np.asarray(t, np.float64)
    X = np.zeros((0, 3))
    while len(X) < n:      # points both cameras see
        u, v = rng.uniform(20, W - 20, 4 * n), rng.uniform(20, H - 20, 4 * n)
        x, y = (u - K[2]) / K[0], (v - K[3]) / K[1]
        z = 8.0 / (1 + plane[0] * x + plane[1] * y) if planar else rng.uniform(depth[0], depth[1], 4 * n)      # the plane a x + b y + z = 8
        c = np.stack([x * z, y * z, z], 1)
        p2 = _project(c @ Rm.T + tv)
        ok = (p2[:, 0] > 5) & (p2[:, 0] < W - 5) & (p2[:, 1] > 5) & (p2[:, 1] < H - 5) & ((c @ Rm.T + tv)[:, 2] > 0.5)
        X = np.concatenate([X, c[ok]])[:n]
    p1 = _project(X) + noise * rng.standard_normal((n, 2))
    p2 = _project(X @ Rm.T + tv) + noise * rng.standard_normal((n, 2))
    out = rng.permutation(n)[:int(round(outliers * n))]
    p2[out] = np.stack([rng.uniform(0, W, len(out)), rng.uniform(0, H, len(out))], 1)
    e1 = np.stack([rng.uniform(0, W, extra), rng.uniform(0, H, extra)], 1)
    extra2 = extra + 7 if extra2 is None else extra2
    e2 = np.stack([rng.uniform(0, W, extra2), rng.uniform(0, H, extra2)], 1)
    if far:      # never matched, far outside the image: they move Normalize's mean and scale
        e1[: extra // 2] = e1[: extra // 2] * 9 + np.array([5000.0, -3000.0])
        e2[: extra // 2] = e2[: extra // 2] * 7 - np.array([4000.0, 2500.0])
    # frame 1: matched and unmatched keypoints interleaved, `first` ascending; frame 2: in another order
    n1 = n + extra
    slots1 = np.sort(rng.permutation(n1)[:n])
    keys1 = np.zeros((n1, 2))
    keys1[slots1] = p1
    keys1[np.setdiff1d(np.arange(n1), slots1)] = e1
    n2 = n + extra2
    slots2 = rng.permutation(n2)[:n]
    keys2 = np.zeros((n2, 2))
    keys2[slots2] = p2
    keys2[np.setdiff1d(np.arange(n2), slots2)] = e2
    prob = dict(keys1=keys1.astype(f32), keys2=keys2.astype(f32), matches12=np.stack([slots1, slots2], 1).astype(np.int32), K=K, sigma=sigma,
                min_parallax=R.MIN_PARALLAX if min_parallax is None else min_parallax, min_triangulated=R.MIN_TRIANGULATED if min_triangulated is None else min_triangulated)
    prob["sets"] = sets_of(n, iterations, seed + 1)
    prob["truth"] = dict(R=Rm, t=tv, outlier=out, planar=planar)
    return prob


FRIENDLY = {
    "general_96": dict(n=96, seed=101, iterations=200), "general_150": dict(n=150, seed=124, iterations=200), "general_257": dict(n=257, seed=103, iterations=200),
    "planar_96": dict(n=96, seed=111, planar=True, iterations=200), "planar_257": dict(n=257, seed=130, planar=True, plane=(0.9, -0.2), iterations=200),
}


def friendly(name):
    return scene(**FRIENDLY[name])


def workload():
    """the workload's own size: 2000 matches among 2 x 2000 keypoints, 200 sets"""
    return scene(n=2000, seed=120, extra=0, extra2=0, iterations=200)


def _duplicated(seed):
    """eight matches that are copies of one keypoint pair, and a set that draws exactly them: ComputeH21's system has rank 2"""
    p = scene(n=64, seed=seed, iterations=6)
    m = p["matches12"]
    for i in range(8):
        p["keys1"][m[i, 0]] = p["keys1"][m[0, 0]]
        p["keys2"][m[i, 1]] = p["keys2"][m[0, 1]]
    p["sets"][0] = np.arange(8)
    return p


def _singular(seed):
    """Integer keypoints; the eight pairs of set 0 are copies of one pair that sits exactly at each frame's mean (one unmatched keypoint per frame balances the sum,
    and every partial sum is an integer below 2^24, so Normalize's float sums are exact).  Normalize maps those pairs to (0, 0) exactly, A^T A of either system is
    already diagonal and its null vector is a unit vector: Hn has one non-zero row, H21i is exactly singular (the zero inverse, NaN chi-squares, a NaN score that never
    wins) and its zero third row is an exactly zero transfer denominator for every match."""
    p = scene(n=64, seed=seed, iterations=6)
    m = p["matches12"]
    for key, col, mean in (("keys1", 0, (320.0, 240.0)), ("keys2", 1, (300.0, 250.0))):
        k = np.round(p[key]).astype(np.float64)
        k[m[:8, col]] = mean
        free = np.setdiff1d(np.arange(len(k)), m[:, col])[0]      # an unmatched keypoint
        k[free] = 0
        k[free] = len(k) * np.array(mean) - k.sum(0)
        p[key] = k.astype(f32)
    p["sets"][0] = np.arange(8)
    return p


def _ambiguous(seed):
    """a plane facing the camera moved along its own normal: two of Faugeras' solutions keep every point in front of both cameras"""
    return scene(n=96, seed=seed, planar=True, noise=0.0, outliers=0.0, rot=(0.0, 0.0, 0.0), t=(0.0, 0.0, -1.5), iterations=8)


IRREGULAR = {
    # name: (builder, what it is built to reach)
    "n8": (lambda: scene(n=8, seed=201, noise=0.0, outliers=0.0, iterations=4, min_triangulated=4), "N = 8: every set is a permutation of all matches"),
    "n9": (lambda: scene(n=9, seed=202, noise=0.0, outliers=0.0, iterations=4, min_triangulated=4), "N = 9"),
    "n63": (lambda: scene(n=63, seed=203, iterations=12), "one short of a wavefront"),
    "n64": (lambda: scene(n=64, seed=204, iterations=12), "a wavefront"),
    "n65": (lambda: scene(n=65, seed=205, iterations=12), "one past a wavefront"),
    "n255": (lambda: scene(n=255, seed=206, iterations=12), "one short of a workgroup"),
    "n256": (lambda: scene(n=256, seed=207, iterations=12), "a workgroup"),
    "n257": (lambda: scene(n=257, seed=208, planar=True, iterations=12), "one past a workgroup"),
    "one_iteration": (lambda: scene(n=96, seed=209, iterations=1), "iterations = 1"),
    "pure_rotation": (lambda: scene(n=96, seed=210, noise=0.0, outliers=0.0, rot=(0.03, -0.05, 0.02), t=(0.0, 0.0, 0.0), iterations=8), ":597 d1/d2 < 1.00001"),
    "low_parallax": (lambda: scene(n=96, seed=211, noise=0.05, outliers=0.0, t=(0.08, 0.02, 0.0), iterations=16), ":525-565 a clear winner whose parallax > minParallax fails"),
    "all_outliers": (lambda: scene(n=96, seed=212, outliers=1.0, iterations=12), ":517 / :721 too few triangulated"),
    "ambiguous": (lambda: _ambiguous(213), ":721 secondBestGood < 0.75 * bestGood fails (or :517 nsimilar > 1)"),
    "duplicated": (lambda: _duplicated(214), ":159 / :210 rank-deficient systems: eight copies of one pair in a set"),
    "singular": (lambda: _singular(219), ":161 a singular H21i: the zero inverse, NaN chi-squares, a NaN score that never wins; :368 a transfer denominator exactly zero"),
    "vanishing": (lambda: scene(n=96, seed=215, planar=True, rot=(0.5, -0.6, 0.05), t=(2.5, 0.3, 2.0), iterations=12), ":352 / :368 transfer denominators near zero"),
    "far_keypoints": (lambda: scene(n=96, seed=216, far=True, iterations=24), ":757-779 Normalize sums over unmatched keypoints far away"),
    "no_model": (lambda: scene(n=96, seed=217, sigma=1e-20, iterations=8), "no hypothesis scores above 0: no_model"),
    "sigma_2": (lambda: scene(n=150, seed=218, noise=1.0, sigma=2.0, iterations=32), "sigma != 1"),
}


def irregular(name):
    return IRREGULAR[name][0]()
