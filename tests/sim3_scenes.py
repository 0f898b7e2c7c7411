"""Seeded OptimizeSim3 problems (the eao_sim3_problem fields as numpy arrays) for the Sim3 tests, the golden generator and the
benchmark: two keyframes looking at the same points, S12 planted between their camera frames, pixel noise, optional outliers."""
import math

import numpy as np

from sim3_reference import Sim3, camera_points, qmul, quat_from_R, quat_to_R

K_TUM1 = (517.306408, 516.469215, 318.643040, 255.313989)


def axis_angle_q(axis, ang):
    axis = np.asarray(axis, np.float64)
    axis = axis / np.linalg.norm(axis)
    h = 0.5 * ang
    return np.array([axis[0] * math.sin(h), axis[1] * math.sin(h), axis[2] * math.sin(h), math.cos(h)])


def random_pose(rng, rot_deg=30.0, trans=2.0):
    q = axis_angle_q(rng.normal(size=3), math.radians(rng.uniform(-rot_deg, rot_deg)))
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = quat_to_R(q)
    T[:3, 3] = rng.uniform(-trans, trans, 3)
    return T


def scene(n, seed, fix_scale=True, outlier_frac=0.0, off_deg=1.0, off_m=0.02, noise_px=1.0, th2=10.0, scale=None, n_levels=8):
    """n correspondences; S12 maps camera-2 points into camera 1.  The start is the planted S12 rotated by off_deg about a random
    axis and moved by off_m (and, without fix_scale, scaled by up to 5 %)."""
    rng = np.random.default_rng(seed)
    s_true = 1.0 if fix_scale else (scale if scale is not None else float(rng.uniform(0.6, 1.6)))
    q_true = axis_angle_q(rng.normal(size=3), math.radians(rng.uniform(2, 15)))
    S12 = Sim3(q_true, rng.uniform(-0.3, 0.3, 3), s_true)
    # points in front of camera 1, inside the image; camera 2 sees them through S21
    X1 = np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-1.1, 1.1, n), np.ones(n)], axis=1) * rng.uniform(2.0, 6.0, (n, 1))
    X2 = S12.inverse().map(X1)
    T1w, T2w = random_pose(rng), random_pose(rng)

    def to_world(T, Xc):
        R, t = T[:3, :3].astype(np.float64), T[:3, 3].astype(np.float64)
        return ((Xc - t) @ R).astype(np.float32)

    Xw1, Xw2 = to_world(T1w, X1), to_world(T2w, X2)
    K1 = K_TUM1
    K2 = (K_TUM1[0] * 1.01, K_TUM1[1] * 0.99, K_TUM1[2] + 2.0, K_TUM1[3] - 1.5)

    def project(K, X):
        return np.stack([X[:, 0] / X[:, 2] * K[0] + K[2], X[:, 1] / X[:, 2] * K[1] + K[3]], axis=1)

    oct1, oct2 = rng.integers(0, n_levels, n), rng.integers(0, n_levels, n)
    sig1, sig2 = 1.2 ** oct1, 1.2 ** oct2
    obs1 = project(K1, X1) + rng.normal(size=(n, 2)) * noise_px * sig1[:, None]
    obs2 = project(K2, X2) + rng.normal(size=(n, 2)) * noise_px * sig2[:, None]
    if outlier_frac > 0:
        bad = rng.random(n) < outlier_frac
        obs1[bad] += rng.uniform(-60, 60, (int(bad.sum()), 2))
        bad2 = rng.random(n) < outlier_frac * 0.5
        obs2[bad2] += rng.uniform(-60, 60, (int(bad2.sum()), 2))
    dq = axis_angle_q(rng.normal(size=3), math.radians(off_deg))
    d = rng.normal(size=3)
    q0 = qmul(dq, q_true)
    t0 = S12.t + off_m * d / np.linalg.norm(d)
    s0 = s_true if fix_scale else s_true * float(rng.uniform(0.95, 1.05))
    inv_levels = (1.0 / (1.2 ** (2 * np.arange(n_levels)))).astype(np.float32)
    return dict(T1w=T1w, T2w=T2w, Xw1=Xw1, Xw2=Xw2, obs1=obs1.astype(np.float32), obs2=obs2.astype(np.float32),
                inv_sigma2_1=inv_levels[oct1], inv_sigma2_2=inv_levels[oct2], K1=np.array(K1, np.float32), K2=np.array(K2, np.float32),
                q=q0, t=t0, s=s0, th2=np.float32(th2), fix_scale=bool(fix_scale), planted=dict(q=q_true, t=S12.t.copy(), s=s_true))


def ulp_perturbed(prob, seed=0):
    """The same problem with every observation moved by one float32 ulp (the chaos probe of the parity tests)."""
    rng = np.random.default_rng(seed)
    p = dict(prob)
    for k in ("obs1", "obs2"):
        a = np.asarray(prob[k], np.float32)
        direction = np.where(rng.random(a.shape) < 0.5, np.float32(-np.inf), np.float32(np.inf))
        p[k] = np.nextafter(a, direction).astype(np.float32)
    return p


def keyframe_scene(prob, seed=0, n_extra=None):
    """Embeds a flattened problem in two stand-in keyframes (tests/cpp/sim3/sim3_driver.cpp's input) among entries the walk must skip:
    no match, no KF1 map point, a bad point on either side, a match not observed in KF2 (GetIndexInKeyFrame < 0).  Returns
    (scene text, expected index of each correspondence in vpMatches1)."""
    rng = np.random.default_rng(seed)
    n = len(prob["Xw1"])
    n_extra = n // 3 + 6 if n_extra is None else n_extra
    kinds = np.array([0] * n + list(rng.integers(1, 6, n_extra)))
    rng.shuffle(kinds)
    N1 = len(kinds)
    inv = (1.0 / (1.2 ** (2 * np.arange(8)))).astype(np.float32)
    oct_of = {float(v): k for k, v in enumerate(inv)}
    pool, kf1, kf2, expected = [], [], [], []
    c = 0
    for i, kind in enumerate(kinds):
        if kind == 0:
            x1, x2 = prob["Xw1"][c], prob["Xw2"][c]
            o1, o2 = prob["obs1"][c], prob["obs2"][c]
            oc1, oc2 = oct_of[float(prob["inv_sigma2_1"][c])], oct_of[float(prob["inv_sigma2_2"][c])]
            j = len(kf2)
            kf2.append((o2[0], o2[1], oc2))
            pool.append((x1, 0, -1))
            pool.append((x2, 0, j))
            kf1.append((o1[0], o1[1], oc1, len(pool) - 2, len(pool) - 1))
            expected.append(i)
            c += 1
            continue
        xr = rng.normal(size=3).astype(np.float32)
        j = len(kf2)
        kf2.append((float(rng.uniform(0, 640)), float(rng.uniform(0, 480)), 0))
        bad1, bad2, i2, has1, has_match = 0, 0, j, True, True
        if kind == 1:
            has_match = False
        elif kind == 2:
            has1 = False
        elif kind == 3:
            bad1 = 1
        elif kind == 4:
            bad2 = 1
        else:
            i2 = -1
        pool.append((xr, bad1, -1))
        pool.append((xr * 2, bad2, i2))
        kf1.append((float(rng.uniform(0, 640)), float(rng.uniform(0, 480)), 0, len(pool) - 2 if has1 else -1, len(pool) - 1 if has_match else -1))
    f = lambda v: repr(float(v))
    lines = ["%d %d" % (N1, len(kf2)), " ".join(f(v) for v in prob["K1"]), " ".join(f(v) for v in prob["K2"]),
             " ".join(f(v) for v in np.asarray(prob["T1w"], np.float32).ravel()), " ".join(f(v) for v in np.asarray(prob["T2w"], np.float32).ravel()),
             " ".join(f(v) for v in prob["q"]) + " " + " ".join(f(v) for v in prob["t"]) + " %s %s %d" % (f(prob["s"]), f(prob["th2"]), int(prob["fix_scale"])),
             str(len(pool))]
    lines += ["%s %s %s %d %d" % (f(x[0]), f(x[1]), f(x[2]), b, i2) for x, b, i2 in pool]
    lines += ["%s %s %d %d %d" % (f(x), f(y), o, m1, mt) for x, y, o, m1, mt in kf1]
    lines += ["%s %s %d" % (f(x), f(y), o) for x, y, o in kf2]
    lines.append(" ".join(f(v) for v in inv))
    return "\n".join(lines) + "\n", expected


# The seeded families of the parity tests: (family, scene() arguments).
FAMILIES = (
    [("rgbd", dict(n=n, seed=s, fix_scale=True)) for n in (20, 300, 2000) for s in (11, 12)]
    + [("mono", dict(n=n, seed=s, fix_scale=False)) for n in (20, 300, 2000) for s in (21, 22)]
    + [("outliers", dict(n=300, seed=s, fix_scale=fs, outlier_frac=0.2)) for s, fs in ((31, True), (32, False), (33, True))]
    + [("far_off", dict(n=300, seed=s, fix_scale=fs, off_deg=10.0, off_m=0.3)) for s, fs in ((41, True), (42, False))]
    + [("early_exit", dict(n=14, seed=s, fix_scale=True, outlier_frac=0.6)) for s in (51, 52)]
    + [("empty", dict(n=0, seed=61, fix_scale=True))]
)

# Families on which the reference's own ITERATION COUNTS change when every observation moves by one float32 ulp (ulp_perturbed): the
# problem has converged before the last optimize() ends, and whether the rho == 0 / "3 bad iterations" stop comes one iteration earlier
# or later is rounding.  Only the iteration counts move; removed, n_inliers, early_exit stay, and the estimate moves by at most 1.5e-5
# of the update (profiles/r07_sim3_chaotic_seeds.txt, written by tools/sim3_chaotic_seeds.py).  (family, n, seed).
ITERS_UNSTABLE = {("rgbd", 20, 11), ("rgbd", 20, 12), ("rgbd", 300, 12)}


def family_key(name, kw):
    return (name, kw["n"], kw["seed"])


# ---------------------------------------------------------------------- irregular correspondence sets
# Small edits of a scene() problem, each returning a new problem.  What an edit planted is recorded under prob["planted_rows"][label], so
# that the CPU tests can hold a family to what it claims (tests/test_sim3_reference_cpu.py).
def _edited(prob, label, idx, **arrays):
    p = dict(prob)
    p.update(arrays)
    rows = dict(prob.get("planted_rows", {}))
    rows[label] = np.union1d(rows.get(label, np.zeros(0, np.int64)), np.asarray(idx, np.int64))
    p["planted_rows"] = rows
    return p


def _camera_frame(prob, which):
    T = np.asarray(prob["T%dw" % which], np.float32)
    return T, camera_points(T, prob["Xw%d" % which])


def _world_from_camera(T, Xc):
    R, t = T[:3, :3].astype(np.float64), T[:3, 3].astype(np.float64)
    return ((Xc - t) @ R).astype(np.float32)


def mirror_behind(prob, which, idx):
    """The map points idx of keyframe `which` (1 or 2) reflected through that camera's z = 0 plane: z < 0 in its own frame, and -- S12
    being a few degrees and decimetres -- behind the other camera as well, where the edge divides by that z."""
    T, Xc = _camera_frame(prob, which)
    Xc[idx, 2] = -Xc[idx, 2]
    Xw = np.array(prob["Xw%d" % which], np.float32)
    Xw[idx] = _world_from_camera(T, Xc[idx])
    return _edited(prob, "behind%d" % which, idx, **{"Xw%d" % which: Xw})


def set_depth(prob, which, idx, z):
    """The map points idx of keyframe `which` given depth z in that camera, x and y kept: far off its own viewing ray."""
    T, Xc = _camera_frame(prob, which)
    Xc[idx, 2] = z
    Xw = np.array(prob["Xw%d" % which], np.float32)
    Xw[idx] = _world_from_camera(T, Xc[idx])
    return _edited(prob, "depth%d" % which, idx, **{"Xw%d" % which: Xw})


def gross(prob, idx, px):
    """obs1 of rows idx moved by px pixels in x and y."""
    obs1 = np.array(prob["obs1"], np.float32)
    obs1[idx] += np.float32(px)
    return _edited(prob, "gross", idx, obs1=obs1)


def zero_information(prob, idx1, idx2):
    """inv_sigma2_1 = 0 on rows idx1 and inv_sigma2_2 = 0 on rows idx2: chi2 = 0, rho' = 1, no contribution, never an outlier.  The rows in
    both sets are recorded as "zero_info": nothing can remove them."""
    i1, i2 = np.array(prob["inv_sigma2_1"], np.float32), np.array(prob["inv_sigma2_2"], np.float32)
    i1[idx1] = 0
    i2[idx2] = 0
    return _edited(prob, "zero_info", np.intersect1d(idx1, idx2), inv_sigma2_1=i1, inv_sigma2_2=i2)


def duplicate_rows(prob, src, idx):
    """Rows idx become copies of row src."""
    out = {}
    for k in ("Xw1", "Xw2", "obs1", "obs2", "inv_sigma2_1", "inv_sigma2_2"):
        a = np.array(prob[k])
        a[idx] = a[src]
        out[k] = a
    return _edited(prob, "duplicates", idx, **out)


def non_unit_q(prob, factor):
    """The start quaternion scaled: g2o never renormalises, so S.map scales by |q|^2 on top of s."""
    return _edited(prob, "non_unit_q", [], q=np.asarray(prob["q"], np.float64) * factor)


def _ten_survivors(n_clean, n_gross):
    n = n_clean + n_gross
    return lambda p: gross(p, np.arange(n)[::2][:n_gross], 80.0)


def _strided_rows(n):
    m = np.arange(n)
    return m[(m % 256 == 7) | ((m >= 64) & (m < 128))]


def _zero_info_edit(p):
    n = len(p["Xw1"])
    both = np.arange(5, n, 13)                      # zero on both edges: cannot be removed, whatever their observations
    p = gross(p, both[::3], 80.0)
    return zero_information(p, np.union1d(both, np.arange(0, n, 5)), np.union1d(both, np.arange(2, n, 5)))


# (name, scene() arguments, edit or None); family_key() is unique.  irregular_scene() builds one.
IRREGULAR = (
    [("ten_survive", dict(n=15, seed=311, fix_scale=True, noise_px=0.3), _ten_survivors(10, 5)),
     ("nine_survive", dict(n=15, seed=312, fix_scale=True, noise_px=0.3), _ten_survivors(9, 6)),
     ("ten_clean", dict(n=10, seed=315, fix_scale=True, noise_px=0.3), None),
     ("nine_clean", dict(n=9, seed=314, fix_scale=True, noise_px=0.3), None),
     ("behind_cam2", dict(n=200, seed=321, fix_scale=False), lambda p: mirror_behind(p, 2, np.arange(3, 200, 17))),
     ("behind_cam1", dict(n=200, seed=322, fix_scale=True), lambda p: mirror_behind(p, 1, np.arange(5, 200, 17))),
     ("depth_collapse", dict(n=200, seed=330, fix_scale=True), lambda p: set_depth(p, 1, np.arange(10, 200, 50), 1e-4)),
     ("depth_near", dict(n=200, seed=341, fix_scale=True), lambda p: set_depth(p, 1, np.arange(10, 200, 50), 0.1)),
     ("zero_info", dict(n=200, seed=341, fix_scale=True, outlier_frac=0.2), _zero_info_edit),
     ("scale_small", dict(n=300, seed=351, fix_scale=False, scale=0.05), None),
     ("scale_large", dict(n=300, seed=352, fix_scale=False, scale=20.0), None),
     ("scale_large_banded", dict(n=300, seed=376, fix_scale=False, scale=20.0), None),
     ("all_outliers", dict(n=300, seed=361, fix_scale=True, outlier_frac=1.0), None),
     ("far_start", dict(n=200, seed=402, fix_scale=True, off_deg=25.0, off_m=0.8), None),
     ("far_start_lost", dict(n=200, seed=404, fix_scale=True, off_deg=25.0, off_m=0.8), None),
     ("far_start_lost", dict(n=200, seed=461, fix_scale=False, off_deg=25.0, off_m=0.8), None),
     ("th2_narrow", dict(n=300, seed=371, fix_scale=True, outlier_frac=0.1, th2=2.0), None),
     ("th2_wide", dict(n=300, seed=372, fix_scale=False, outlier_frac=0.1, th2=40.0), None),
     ("budget_five", dict(n=200, seed=382, fix_scale=True, off_deg=25.0, off_m=2.0, th2=1e6, noise_px=0.3), None),
     ("non_unit_q", dict(n=300, seed=391, fix_scale=True, outlier_frac=0.1), lambda p: non_unit_q(p, 1.003)),
     ("duplicates", dict(n=300, seed=392, fix_scale=True, outlier_frac=0.1), lambda p: duplicate_rows(p, 7, np.arange(100, 150))),
     ("strided", dict(n=1500, seed=396, fix_scale=True, noise_px=0.3), lambda p: gross(p, _strided_rows(1500), 80.0))]
    + [("edge_n", dict(n=n, seed=500 + k, fix_scale=(k % 2 == 0), outlier_frac=0.1), None)
       for k, n in enumerate((63, 64, 65, 255, 256, 257, 513, 1025))]
    + [("large", dict(n=20000, seed=395, fix_scale=False, outlier_frac=0.05), None)]
)


# The problems of the call-order test, in their first order: sizes that grow, shrink to nothing and grow again on one thread's staging
# buffers.  (scene() arguments, edit) as in IRREGULAR; tests/sim3_child.py runs one of them in a process of its own.
CALL_ORDER = [
    (dict(n=20000, seed=395, fix_scale=False, outlier_frac=0.05), None),
    (dict(n=0, seed=61, fix_scale=True), None),
    (dict(n=11, seed=601, fix_scale=True, noise_px=0.3), None),
    (dict(n=2000, seed=602, fix_scale=False, outlier_frac=0.1), None),
    (dict(n=20000, seed=603, fix_scale=True, outlier_frac=0.05), None),
    (dict(n=14, seed=51, fix_scale=True, outlier_frac=0.6), None),
]


def irregular_scene(kw, edit):
    p = scene(**kw)
    return edit(p) if edit is not None else p


def irregular_ids():
    return ["%s-%d-%d" % (name, kw["n"], kw["seed"]) for name, kw, _ in IRREGULAR]


# The two tables below are written from profiles/sim3_irregular_bands.txt (tools/sim3_chaotic_seeds.py --irregular: every family as
# generated and under ulp_perturbed seeds 0..3); a CPU test keeps them equal to that probe.  Keys as family_key().
# Families whose reference iteration counts move under one ulp (the rule of ITERS_UNSTABLE); at most three that do not exit early.
IRREGULAR_ITERS_UNSTABLE = {("ten_clean", 10, 315), ("nine_clean", 9, 314)}
# Families on which the reference's own one-ulp displacement exceeds lm_tolerances.UPDATE_REL of its update; at most one.
IRREGULAR_BANDED = {("scale_large_banded", 300, 376)}
# Caps, not measurements: a family that breaks one gets another seed or a milder parameter, never a wider table.  (And no family's removed,
# n_inliers or early_exit may move under one ulp at all.)
IRREGULAR_BANDED_MAX, IRREGULAR_ITERS_UNSTABLE_MAX = 1, 3


__all__ = ["scene", "ulp_perturbed", "axis_angle_q", "quat_from_R", "K_TUM1", "FAMILIES", "ITERS_UNSTABLE", "family_key", "IRREGULAR", "CALL_ORDER",
           "irregular_scene", "irregular_ids", "IRREGULAR_ITERS_UNSTABLE", "IRREGULAR_BANDED", "IRREGULAR_BANDED_MAX",
           "IRREGULAR_ITERS_UNSTABLE_MAX", "mirror_behind", "set_depth", "gross",
           "zero_information", "duplicate_rows", "non_unit_q"]
