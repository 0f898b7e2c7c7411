"""Scenes for the Sim3Solver tests (tests/test_sim3_solver_reference_cpu.py, tests/test_gpu_sim3_solver.py): two keyframes, a true Sim3
between their camera frames, points in front of both cameras, pixel noise put in through the world points, an outlier fraction, octaves
over 8 levels of 1.2; and the triples of every family as explicit arrays, made from a seeded stream through the reference's sampling
loop (sim3_solver_reference.draw_triple) plus hand-made ones."""
import numpy as np

import sim3_solver_reference as R

F = np.float32
K_DEFAULT = (525.0, 525.0, 319.5, 239.5)
MIN_INLIERS = 20


def level_sigma2():
    """mvLevelSigma2 as ORBextractor makes it: float scale factors multiplied up by 1.2f, squared in float"""
    sf = [F(1)]
    for _ in range(7):
        sf.append(F(sf[-1] * F(1.2)))
    return np.array([F(s * s) for s in sf], F)


def _rot(axis, ang):
    axis = np.asarray(axis, np.float64)
    axis = axis / np.linalg.norm(axis)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * (Kx @ Kx)


def _pose(rng, identity):
    T = np.eye(4)
    if not identity:
        T[:3, :3] = _rot(rng.normal(size=3), rng.uniform(0.1, 0.6))
        T[:3, 3] = rng.uniform(-1, 1, 3)
    return T


def scene(n, seed, fix_scale, noise_px=0.5, outlier_frac=0.2, scale=None, identity_cam1=False):
    """One flattened Sim3Solver problem (the dict eao_fusion_amd.sim3_solver takes) plus `true_T12` (4,4) f64 and `octave1` / `octave2`."""
    rng = np.random.default_rng(seed)
    K = K_DEFAULT
    s = 1.0 if fix_scale else (float(scale) if scale is not None else rng.uniform(0.8, 1.25))
    R12 = _rot(rng.normal(size=3), rng.uniform(0.05, 0.3))
    t12 = rng.uniform(-0.3, 0.3, 3)
    # camera-1 points in front of camera 1; camera-2 points X2 = (1 / s) R12^T (X1 - t12), in front of camera 2 as well for these ranges
    z = rng.uniform(2.0, 8.0, n)
    X1c = np.stack([rng.uniform(-0.5, 0.5, n) * z, rng.uniform(-0.4, 0.4, n) * z, z], axis=1)
    X2c = ((X1c - t12) @ R12) / s
    sig = level_sigma2()
    o1, o2 = rng.integers(0, 8, n), rng.integers(0, 8, n)
    if noise_px > 0 and n:
        # pixel noise through the points: each point moves sideways at its own depth by noise_px * scale[octave] pixels
        for X, o in ((X1c, o1), (X2c, o2)):
            d = rng.normal(size=(n, 2)) * noise_px * np.sqrt(sig[o].astype(np.float64))[:, None]
            X[:, 0] += d[:, 0] * X[:, 2] / K[0]
            X[:, 1] += d[:, 1] * X[:, 2] / K[1]
    n_out = int(round(outlier_frac * n))
    if n_out:
        bad = rng.choice(n, n_out, replace=False)
        zb = rng.uniform(2.0, 8.0, n_out) / s
        X2c[bad] = np.stack([rng.uniform(-0.5, 0.5, n_out) * zb, rng.uniform(-0.4, 0.4, n_out) * zb, zb], axis=1)
    T1w, T2w = _pose(rng, identity_cam1), _pose(rng, False)
    T2w[:3, 3] /= s          # map 2 lives at its own scale: the camera's distance from its origin goes with the size of its points
    Xw1 = (X1c - T1w[:3, 3]) @ T1w[:3, :3]
    Xw2 = (X2c - T2w[:3, 3]) @ T2w[:3, :3]
    T12 = np.eye(4)
    T12[:3, :3], T12[:3, 3] = s * R12, t12
    return dict(T1w=T1w.astype(F), T2w=T2w.astype(F), Xw1=Xw1.astype(F).reshape(-1, 3), Xw2=Xw2.astype(F).reshape(-1, 3), sigma2_1=sig[o1], sigma2_2=sig[o2],
                K1=K, K2=K, fix_scale=bool(fix_scale), true_T12=T12, octave1=o1, octave2=o2)


def counting_stream(seed):
    """rand_ints(lo, hi) over a seeded generator, the stand-in for DUtils::Random::RandomInt"""
    rng = np.random.default_rng(seed)
    return lambda lo, hi: int(rng.integers(lo, hi + 1))


def drawn_triples(n, n_hyp, seed):
    rnd = counting_stream(seed)
    return np.array([R.draw_triple(n, rnd) for _ in range(n_hyp)], np.int32).reshape(-1, 3)


def ulp_perturbed(prob, seed=0):
    """The same problem with every world point coordinate moved by one float32 ulp up or down"""
    rng = np.random.default_rng(seed)
    p = dict(prob)
    for k in ("Xw1", "Xw2"):
        a = np.asarray(prob[k], F)
        direction = np.where(rng.random(a.shape) < 0.5, F(-np.inf), F(np.inf))
        p[k] = np.nextafter(a, direction).astype(F)
    return p


# ---------------------------------------------------------------------- friendly families
FRIENDLY_N = (20, 21, 63, 64, 65, 257, 2000)
FRIENDLY_HYP = 24
FRIENDLY = [("n%d-fs%d" % (n, fs), dict(n=n, seed=4000 + 2 * n + fs, fix_scale=bool(fs))) for n in FRIENDLY_N for fs in (1, 0)]


def friendly(name):
    """(problem, triples) of a friendly family"""
    kw = dict(FRIENDLY)[name]
    return scene(**kw), drawn_triples(kw["n"], FRIENDLY_HYP, kw["seed"] + 7)


# ---------------------------------------------------------------------- irregular families
def _spread_triple(prob, exclude=()):
    """three correspondences far apart in the image of camera 1 (a well-conditioned hand-made triple)"""
    pre = R.prepare(prob)
    im = pre["im1"].astype(np.float64)
    ok = [i for i in range(pre["n"]) if i not in exclude]
    a = min(ok, key=lambda i: im[i, 0] + im[i, 1])
    b = max(ok, key=lambda i: im[i, 0] - 0.3 * im[i, 1])
    c = max((i for i in ok if i not in (a, b)), key=lambda i: abs((im[b] - im[a])[0] * (im[i] - im[a])[1] - (im[b] - im[a])[1] * (im[i] - im[a])[0]))
    return (a, b, c)


def _small(n):
    def make():
        p = scene(n=n, seed=5100 + n, fix_scale=True)
        tr = np.zeros((5, 3), np.int32) if n < 3 else drawn_triples(n, 5, 11)
        return p, tr
    return make


def _n_equals_min():
    p = scene(n=MIN_INLIERS, seed=5201, fix_scale=True, outlier_frac=0.0)
    return p, drawn_triples(MIN_INLIERS, 5, 12)


def _depth_edge():
    """correspondence 5 at z = 0 in camera 1 (1 / z = inf: its image point is inf or NaN), correspondence 6 behind camera 1, 7 behind camera 2"""
    p = scene(n=64, seed=5301, fix_scale=True, identity_cam1=True)
    for k in ("Xw1", "Xw2"):
        p[k] = p[k].copy()
    p["Xw1"][5, 2] = 0.0
    p["Xw1"][6, 2] = -2.0
    X2 = R.transform_points(p["T2w"], p["Xw2"][7:8]).astype(np.float64)[0]
    X2[2] = -3.0
    T2 = p["T2w"].astype(np.float64)
    p["Xw2"][7] = ((X2 - T2[:3, 3]) @ T2[:3, :3]).astype(F)
    tr = np.concatenate([drawn_triples(64, 10, 13), np.array([[5, 1, 2], [6, 7, 8], [5, 6, 7]], np.int32)])
    return p, tr


TRUNCATION_INDEX = 9


def _truncation():
    """Noise-free; correspondence 9 sits on octave 1 in camera 1 (sigma2 = 1.44: 9.21 * 1.44 = 13.26, the gate is 13) and on octave 4 in camera 2
    (gate 39), and its camera-1 point is moved sideways by 3.62 px: err1 = 13.10 under a transform that is exact to well below a pixel."""
    p = scene(n=64, seed=5401, fix_scale=True, noise_px=0.0, outlier_frac=0.0, identity_cam1=True)
    j = TRUNCATION_INDEX
    sig = level_sigma2()
    p["sigma2_1"], p["sigma2_2"], p["Xw1"] = p["sigma2_1"].copy(), p["sigma2_2"].copy(), p["Xw1"].copy()
    p["sigma2_1"][j], p["sigma2_2"][j] = sig[1], sig[4]
    p["Xw1"][j, 0] = F(float(p["Xw1"][j, 0]) + 3.62 * float(p["Xw1"][j, 2]) / K_DEFAULT[0])
    first = _spread_triple(p, exclude=(j,))
    tr = drawn_triples(64, 8, 14)
    tr[tr == j] = (j + 1) % 64
    return p, np.concatenate([np.array([first], np.int32), tr])


def _pure_translation():
    """Exact pure translation: camera 1 at the origin, camera 2 a translation on the 1/8 grid, the same world points (on that grid) on both sides,
    and every hand-made triple (3m, 3m+1, 3m+2) with coordinate sums divisible by three grid units -- centroids, relative coordinates and
    M = Pr2 * Pr1.t() are exact, M is symmetric, N12 = N13 = N14 = 0, the eigenvector is (1, 0, 0, 0), vec / norm(vec) is 0 / 0: T12 is NaN."""
    rng = np.random.default_rng(5501)
    n = 21
    g = np.zeros((n, 3), np.int64)
    for m in range(n // 3):
        a = np.array([rng.integers(-12, 13), rng.integers(-10, 11), rng.integers(16, 49)])
        b = np.array([rng.integers(-12, 13), rng.integers(-10, 11), rng.integers(16, 49)])
        c = np.array([rng.integers(-12, 13), rng.integers(-10, 11), rng.integers(16, 49)])
        c = c - (a + b + c) % 3
        g[3 * m:3 * m + 3] = (a, b, c)
    Xw = (g / 8.0).astype(F)
    T1w, T2w = np.eye(4, dtype=F), np.eye(4, dtype=F)
    T2w[:3, 3] = (0.25, -0.125, 0.5)
    sig = level_sigma2()
    o = rng.integers(0, 8, n)
    p = dict(T1w=T1w, T2w=T2w, Xw1=Xw, Xw2=Xw.copy(), sigma2_1=sig[o], sigma2_2=sig[o], K1=K_DEFAULT, K2=K_DEFAULT, fix_scale=True)
    return p, np.arange(n, dtype=np.int32).reshape(-1, 3)


def _degenerate_triples():
    """a friendly scene under repeated-index triples -- (a, a, a), (a, b, b), the (a, N-1, N-1) the sampling loop can draw -- and exactly collinear ones
    (correspondence 1 moved to the midpoint of 0 and 2 in both camera frames)"""
    p = scene(n=64, seed=5601, fix_scale=False, identity_cam1=True, outlier_frac=0.0, noise_px=0.0)
    for k in ("Xw1", "Xw2"):
        p[k] = p[k].copy()
        p[k][1] = ((p[k][0].astype(np.float64) + p[k][2].astype(np.float64)) / 2).astype(F)
    tr = np.array([[3, 3, 3], [4, 9, 9], [7, 63, 63], [63, 63, 63], [0, 1, 2], [2, 1, 0], [0, 2, 1]], np.int32)
    return p, np.concatenate([tr, drawn_triples(64, 5, 16)])


def _scaled(s):
    def make():
        p = scene(n=65, seed=5701 + int(s > 1), fix_scale=False, scale=s)
        return p, drawn_triples(65, 12, 17)
    return make


IRREGULAR = [("n0", _small(0)), ("n3", _small(3)), ("n19", _small(19)), ("n_equals_min", _n_equals_min), ("depth_edge", _depth_edge),
             ("truncation", _truncation), ("pure_translation", _pure_translation), ("degenerate_triples", _degenerate_triples),
             ("scale_1e-3", _scaled(1e-3)), ("scale_1e3", _scaled(1e3))]


def irregular(name):
    return dict(IRREGULAR)[name]()


def all_families():
    return [(name, lambda name=name: friendly(name)) for name, _ in FRIENDLY] + list(IRREGULAR)


def problem_arrays(prob):
    """the keys the library reads"""
    return {k: prob[k] for k in ("T1w", "T2w", "Xw1", "Xw2", "sigma2_1", "sigma2_2", "K1", "K2", "fix_scale")}
