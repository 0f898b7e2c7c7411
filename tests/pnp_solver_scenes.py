"""Seeded PnPsolver problems (the eao_pnp_solver_problem fields as numpy arrays, the sets in draw order, the parameters SetRansacParameters leaves) for the
PnPsolver tests, the bands tool, the golden generator and the benchmark.

A case is dict(prob, sets (n_hyp, min_set), min_inliers, max_its, min_set, true_inlier, R_true, t_true, kind) and, for the sequencing cases, `chunks` (the
sizes of consecutive iterate calls) or `state` (what the first call starts from).
kind: "parity"   min_set >= 6: per-hypothesis parity with the yardstick is asked (tests/test_pnp_solver_reference_cpu.py holds the conditions it rests on)
      "min4"     min_set = 4 with upstream's parameters: M^T M has a four-dimensional null space, the pose depends on the eigen-solver's basis -- no per-hypothesis
                 parity; replay, the sequential rule, Refine parity and (exact inliers) the outcome are held
      "degenerate" / "sequence"   replay and the sequential rule."""
import numpy as np

import pnp_solver_reference as Y

K = (525.0, 525.0, 319.5, 239.5)
RELOCALIZATION = (0.99, 10, 300, 4, 0.5, 5.991)       # Tracking::Relocalization's SetRansacParameters (src/Tracking.cc:2831)
TH2 = 5.991


def draw_sets(rng, n, min_set, n_hyp):
    """The sampling loop of iterate (:188-201) WITH ITS QUIRK: the drawn VALUE idx, not the position randi, is overwritten by the back element, so an index can be
    drawn again inside a set.  (Where idx is past the live range upstream's write lands in the vector's spare capacity and is never read: skipped here.)"""
    sets = np.zeros((n_hyp, min_set), np.int32)
    for h in range(n_hyp):
        avail = list(range(n))
        for i in range(min_set):
            randi = int(rng.integers(0, len(avail)))      # DUtils::Random::RandomInt(0, size - 1)
            idx = avail[randi]
            sets[h, i] = idx
            if idx < len(avail):
                avail[idx] = avail[-1]
            avail.pop()
    return sets


def random_pose(rng, identity=False):
    if identity:
        return np.eye(3), np.zeros(3)
    a = rng.normal(size=3)
    a /= np.linalg.norm(a)
    th = rng.uniform(0.1, 0.8)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx, rng.uniform(-1, 1, 3)


def project(Xc):
    return np.stack([K[0] * Xc[:, 0] / Xc[:, 2] + K[2], K[1] * Xc[:, 1] / Xc[:, 2] + K[3]], axis=1)


def world(n, rng, R, t, noise_px, outlier_frac, planar=False):
    """n points 2 .. 8 m in front of the camera (R, t), their observations with noise_px * level scale of noise, a share of gross outliers (50 .. 150 px off)."""
    Xc = np.stack([rng.uniform(-1.2, 1.2, n), rng.uniform(-0.9, 0.9, n), np.ones(n)], axis=1) * rng.uniform(2.0, 8.0, (n, 1))
    if planar:
        Xc[:, 2] = 4.0 + 0.3 * Xc[:, 0] - 0.2 * Xc[:, 1]
    Xw = ((Xc - t) @ R).astype(np.float32)      # Xc = R Xw + t
    Xc = Xw.astype(np.float64) @ R.T + t
    octave = rng.integers(0, 8, n)
    sigma2 = (1.2 ** (2 * octave)).astype(np.float32)
    uv = project(Xc) + noise_px * rng.normal(size=(n, 2)) * (1.2 ** octave)[:, None]
    bad = rng.random(n) < outlier_frac
    uv[bad] += rng.uniform(50, 150, (int(bad.sum()), 2)) * rng.choice([-1.0, 1.0], (int(bad.sum()), 2))
    return Xw, uv.astype(np.float32), sigma2, ~bad


def case(n, seed, min_set, n_hyp, noise_px=0.0, outlier_frac=0.3, kind="parity", params=None, planar=False, identity=False):
    rng = np.random.default_rng(seed)
    R, t = random_pose(rng, identity)
    Xw, uv, sigma2, good = world(n, rng, R, t, noise_px, outlier_frac, planar)
    p = params or (0.99, 10, 300, min_set, 0.5, TH2)
    min_inliers, max_its = Y.ransac_parameters(n, *p)
    sets = draw_sets(rng, n, min_set, n_hyp if n_hyp else max_its)
    return dict(prob=dict(p3d_w=Xw, p2d=uv, sigma2=sigma2, K=np.array(K, np.float32), th2=np.float32(p[5])), sets=sets, min_inliers=min_inliers, max_its=max_its,
                min_set=min_set, true_inlier=good, R_true=R, t_true=t, kind=kind)


def two_worlds(seed, n_a, n_b, n_out, min_set=6):
    """Group A (exactly min_inliers = n_a points) agrees with one pose, the larger group B with another, the rest with neither.  A set drawn inside A passes the
    >= gate with n_a inliers and its Refine ends with n_a again: not MORE than min_inliers, so it fails; a set inside B is a later record whose Refine succeeds."""
    rng = np.random.default_rng(seed)
    Ra, ta = random_pose(rng)
    Rb, tb = random_pose(rng)
    Xa, ua, sa, _ = world(n_a, rng, Ra, ta, 0.0, 0.0)
    Xb, ub, sb, _ = world(n_b, rng, Rb, tb, 0.0, 0.0)
    Xo, uo, so, _ = world(n_out, rng, Ra, ta, 0.0, 0.0)
    uo = (uo + rng.uniform(50, 150, uo.shape) * rng.choice([-1.0, 1.0], uo.shape)).astype(np.float32)
    perm = rng.permutation(n_a + n_b + n_out)
    Xw, uv, s2 = np.concatenate([Xa, Xb, Xo])[perm], np.concatenate([ua, ub, uo])[perm], np.concatenate([sa, sb, so])[perm]
    group = np.concatenate([np.zeros(n_a, int), np.ones(n_b, int), np.full(n_out, 2)])[perm]
    prob = dict(p3d_w=Xw, p2d=uv, sigma2=s2, K=np.array(K, np.float32), th2=np.float32(TH2))
    ia, ib = np.flatnonzero(group == 0), np.flatnonzero(group == 1)
    pick = lambda pool: rng.choice(pool, min_set, replace=False)
    return prob, ia, ib, pick, rng, (Rb, tb), group == 1


def fail_then_succeed(seed=40):
    prob, ia, ib, pick, rng, (Rb, tb), good = two_worlds(seed, 12, 30, 23)
    n = len(good)
    mixed = lambda: rng.choice(n, 6, replace=False)
    sets = np.array([mixed(), pick(ia), mixed(), pick(ia), pick(ib), pick(ib), mixed()], np.int32)
    return dict(prob=prob, sets=sets, min_inliers=12, max_its=20, min_set=6, true_inlier=good, R_true=Rb, t_true=tb, kind="sequence")


def carried(seed=41):
    """Two consecutive calls (4 + 5 hypotheses): the first leaves a best set whose Refine fails; in the second a gate-passing NON-record meets that carried set
    before the record that succeeds."""
    prob, ia, ib, pick, rng, (Rb, tb), good = two_worlds(seed, 12, 30, 23)
    n = len(good)
    mixed = lambda: rng.choice(n, 6, replace=False)
    sets = np.array([mixed(), pick(ia), mixed(), mixed(), pick(ia), mixed(), pick(ib), mixed(), pick(ib)], np.int32)
    return dict(prob=prob, sets=sets, min_inliers=12, max_its=20, min_set=6, true_inlier=good, R_true=Rb, t_true=tb, kind="sequence", chunks=(4, 5))


def carried_success(seed=42):
    """Relocalization calls iterate again on a solver that has returned: the state carries a best set whose Refine succeeds, so the first hypothesis that passes the
    >= gate -- record or not -- returns the refined pose of the CARRIED set.  chunks: the first call ends at its record, the second starts from its state."""
    c = case(64, seed, 6, 8, noise_px=0.0, outlier_frac=0.25, kind="sequence")
    good = np.flatnonzero(c["true_inlier"])
    bad = np.flatnonzero(~c["true_inlier"])
    rng = np.random.default_rng(seed + 1000)
    inl = lambda: rng.choice(good, 6, replace=False)
    out = lambda: np.concatenate([rng.choice(good, 3, replace=False), rng.choice(bad, 3, replace=False)])
    c["sets"] = np.array([out(), inl(), out(), out(), inl(), out()], np.int32)
    c["chunks"] = (2, 4)
    return c


def degenerate_repeat(seed=31):
    c = case(65, seed, 6, 6, outlier_frac=0.2, kind="degenerate")
    c["sets"][0, 1] = c["sets"][0, 0]      # a repeated index inside a set: the quirk of the sampling loop makes it legal
    c["sets"][3, 5] = c["sets"][3, 2]
    return c


def degenerate_zero_depth(seed=32):
    """Camera at the identity pose; correspondence 0 lies in the camera's plane z = 0 (its observation is arbitrary) and is drawn into two sets."""
    c = case(64, seed, 6, 6, outlier_frac=0.2, kind="degenerate", identity=True)
    c["prob"]["p3d_w"][0] = (0.5, -0.25, 0.0)
    c["true_inlier"][0] = False
    c["sets"][1, 0] = 0
    c["sets"][4, 3] = 0
    return c


def all_outliers(seed=33):
    c = case(64, seed, 6, 8, outlier_frac=1.0, kind="sequence")
    c["max_its"] = 8      # the chunk exhausts the iterations: no_more with nothing returned
    return c


def all_families():
    """[(name, builder)] -- small on purpose: nothing above N = 257 and 35 hypotheses."""
    reloc = RELOCALIZATION
    return [
        # min_set >= 6: exact inliers + gross outliers (x), 1 px noise (n); wave-edge sizes
        ("x6_n63", lambda: case(63, 1, 6, 20)),
        ("n6_n64", lambda: case(64, 2, 6, 20, noise_px=1.0, outlier_frac=0.2)),
        ("x8_n65", lambda: case(65, 3, 8, 20, outlier_frac=0.12)),
        ("n8_n257", lambda: case(257, 4, 8, 20, noise_px=1.0, outlier_frac=0.2)),
        # N = min_set (nIterations = 1 path: min_inliers = N), N at min_inliers, N just below it
        ("x6_n6", lambda: case(6, 5, 6, 3, outlier_frac=0.0, params=(0.99, 6, 300, 6, 0.5, TH2))),
        ("n8_n10_at_min", lambda: case(10, 6, 8, 6, noise_px=1.0, outlier_frac=0.0)),
        ("n8_n9_below_min", lambda: dict(case(9, 7, 8, 4, noise_px=1.0, outlier_frac=0.0), kind="sequence")),
        # min_set = 4, upstream's parameters, all max_its hypotheses as the first iterate(5) of Relocalization evaluates them
        ("x4_n100", lambda: case(100, 11, 4, 0, kind="min4", params=reloc)),
        ("n4_n100", lambda: case(100, 12, 4, 0, noise_px=1.0, outlier_frac=0.2, kind="min4", params=reloc)),
        ("x4_n257", lambda: case(257, 13, 4, 0, kind="min4", params=reloc)),
        ("n4_n63", lambda: case(63, 14, 4, 0, noise_px=1.0, outlier_frac=0.2, kind="min4", params=reloc)),
        # degenerate
        ("coplanar_n65", lambda: case(65, 30, 6, 8, outlier_frac=0.2, kind="degenerate", planar=True)),
        ("repeat_n65", degenerate_repeat),
        ("zero_depth_n64", degenerate_zero_depth),
        # sequencing
        ("all_outliers_n64", all_outliers),
        ("fail_then_succeed", fail_then_succeed),
        ("carried", carried),
        ("carried_success", carried_success),
    ]


FAMILIES = dict(all_families())
PARITY = [name for name, f in all_families() if f()["kind"] == "parity"]
MIN4 = [name for name, f in all_families() if f()["kind"] == "min4"]


def ulp_perturbed(prob, seed=0):
    """The same problem with every float input (points, observations) moved one float32 ulp up or down."""
    rng = np.random.default_rng(seed)
    p = dict(prob)
    for k in ("p3d_w", "p2d"):
        a = np.asarray(prob[k], np.float32)
        direction = np.where(rng.random(a.shape) < 0.5, np.float32(-np.inf), np.float32(np.inf))
        p[k] = np.nextafter(a, direction).astype(np.float32)
    return p


ULP_SEEDS = (0, 1, 2, 3)


def yardstick_runs(case, ulp_seeds=None):
    """[base (eigh), svd, jacobi, ulp 0..3 (eigh)]: hypotheses() of each, with error2 per (hypothesis, correspondence)"""
    prob, sets = case["prob"], case["sets"]
    out = [Y.hypotheses(prob, sets, "eigh"), Y.hypotheses(prob, sets, "svd"), Y.hypotheses(prob, sets, "jacobi")]
    out += [Y.hypotheses(ulp_perturbed(prob, s), sets, "eigh") for s in (ULP_SEEDS if ulp_seeds is None else ulp_seeds)]
    for h in out:
        h["err"] = np.stack([Y.check_inliers(h["R"][k], h["t"][k], prob, return_error=True)[1] for k in range(len(sets))]).astype(np.float64)
    return out


def pose_spread(rs, alts=None):
    """per hypothesis: the largest |dR|, |dt| between the base run and the others (inf where a NaN pattern differs)"""
    base = rs[0]
    sp = np.zeros(len(base["R"]))
    for a in (rs[1:] if alts is None else alts):
        with np.errstate(all="ignore"):
            d = np.maximum(np.abs(a["R"] - base["R"]).reshape(len(sp), -1).max(axis=1), np.abs(a["t"] - base["t"]).max(axis=1))
        sp = np.maximum(sp, np.where(np.isnan(d), np.inf, d))
    return sp
