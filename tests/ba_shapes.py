"""Bundle-adjustment problems with an IRREGULAR degree structure (a helper module like tests/contention.py, not a conftest).

synth.synth_ba draws one kind of graph: landmark i has 2 + (i mod 7) observers, every camera gets about the same share of the edges, every free camera is well
constrained and nothing is emptied by the outlier pass.  The code under test branches on exactly those counts (the active structure and its -1 entries, the m (m + 1) / 2
pair visits of a landmark with m free observers, long and short pair lists, the chunked validation pass that steps over landmarks without edges, the per-window bounds of
the batched entry point).  The shapes below are synth_ba problems with edges dropped and added: landmarks of degree 0 and 1, landmarks nobody free observes, tracks over
every camera, one camera that sees everything beside one that sees nothing, cameras and landmarks whose every edge is rejected after the first pass.

Every shape returns (problem, facts); `facts` are the properties the shape exists for, as CLAIMS with literal numbers -- tests/test_ba_shapes_cpu.py holds them against a
census of the problem, so that a later edit of synth_ba cannot quietly turn a shape back into an ordinary window."""
import numpy as np

from eao_fusion_amd import synth

EDGE_KEYS = ("edge_cam", "edge_point", "obs", "inv_sigma2")
MIN_UR = 0.5      # an ADDED observation whose right coordinate is not comfortably positive is made monocular (see rebuild)


def project(p, pt, cam):
    """ground-truth projection (u, v, ur, depth) of points `pt` into cameras `cam` (index arrays of equal length), float64"""
    T = p["poses_gt"].astype(np.float64)[cam]
    X = p["points_gt"].astype(np.float64)[pt]
    Xc = np.einsum("eij,ej->ei", T[:, :3, :3], X) + T[:, :3, 3]
    z = Xc[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        u = float(p["fx"]) * Xc[:, 0] / z + float(p["cx"])
        v = float(p["fy"]) * Xc[:, 1] / z + float(p["cy"])
        ur = u - float(p["bf"]) / z
    return u, v, ur, z


def visible(p, pt, cam):
    """the camera has the point in its image: depth > 0.5 m, inside 640 x 480"""
    u, v, _, z = project(p, pt, cam)
    return (z > 0.5) & (u >= 0) & (u < 640) & (v >= 0) & (v < 480)


def rebuild(p, keep=None, extra=None, seed=0):
    """The synth_ba problem `p` with the edges outside the mask `keep` dropped and the edges `extra` = [(point, camera), ...] added (a pair that is already there is not
    added twice).  An added observation is the projection of points_gt through poses_gt with 1 px of noise and inv_sigma2 = 1.  Its right coordinate: obs[:, 2] == 0.0
    is a STEREO edge (the reference tests !(ur < 0)) and one float32 ulp below it is a monocular one, so a value that is not comfortably positive (> MIN_UR px) becomes
    the monocular marker -1 -- a one-ulp probe of such a problem would otherwise change the problem, not its rounding.
    The edge list comes back grouped landmark by landmark, ascending camera inside a landmark (what both adapters produce)."""
    q = dict(p)
    E = len(p["edge_cam"])
    keep = np.ones(E, bool) if keep is None else np.asarray(keep, bool)
    ec, ep = p["edge_cam"][keep].astype(np.int64), p["edge_point"][keep].astype(np.int64)
    obs, inv = p["obs"][keep], p["inv_sigma2"][keep]
    if extra is not None and len(extra):
        extra = np.unique(np.asarray(extra, np.int64).reshape(-1, 2), axis=0)
        nc = len(p["poses"])
        have = set((ep * nc + ec).tolist())
        new = np.array([k not in have for k in (extra[:, 0] * nc + extra[:, 1]).tolist()], bool)
        xp, xc = extra[new, 0], extra[new, 1]
        rng = np.random.default_rng(seed)
        u, v, ur, z = project(p, xp, xc)
        assert np.all(z > 0.1), "an added edge looks at a point behind its camera"
        noise = rng.normal(0.0, 1.0, size=(len(xp), 3))
        xo = np.stack([u + noise[:, 0], v + noise[:, 1], ur + noise[:, 0] + 0.3 * noise[:, 2]], axis=1)
        xo[:, 2] = np.where(xo[:, 2] > MIN_UR, xo[:, 2], -1.0)
        ec, ep = np.concatenate([ec, xc]), np.concatenate([ep, xp])
        obs = np.concatenate([obs, xo.astype(np.float32)])
        inv = np.concatenate([inv, np.ones(len(xp), np.float32)])
    order = np.lexsort((ec, ep))
    q["edge_cam"] = np.ascontiguousarray(ec[order].astype(np.int32))
    q["edge_point"] = np.ascontiguousarray(ep[order].astype(np.int32))
    q["obs"] = np.ascontiguousarray(obs[order].astype(np.float32))
    q["inv_sigma2"] = np.ascontiguousarray(inv[order].astype(np.float32))
    return q


def census(p):
    """degree structure of a problem: edges per landmark, edges per camera, FREE observers per landmark"""
    nc, npt = len(p["poses"]), len(p["points"])
    free = p["fixed"][p["edge_cam"]] == 0
    return dict(lm_deg=np.bincount(p["edge_point"], minlength=npt), cam_deg=np.bincount(p["edge_cam"], minlength=nc),
                lm_free=np.bincount(p["edge_point"][free], minlength=npt), mono=p["obs"][:, 2] < 0)


def first_edge_of(p, mask=None):
    """mask of the first edge (in list order) of every landmark, among the edges of `mask`"""
    E = len(p["edge_cam"])
    mask = np.ones(E, bool) if mask is None else mask
    idx = np.flatnonzero(mask)
    _, first = np.unique(p["edge_point"][idx], return_index=True)
    out = np.zeros(E, bool)
    out[idx[first]] = True
    return out


# ---------------------------------------------------------------------------------------------------------------- window scale
def window_base(n_points=900):
    return synth.synth_ba(n_free=12, n_fixed=3, n_points=n_points, seed=8800)


def _single_observer(n_points, mono):
    p = window_base(n_points)
    thin = p["edge_point"] % 5 == 0
    free = p["fixed"][p["edge_cam"]] == 0
    one = first_edge_of(p, thin & free)                                    # a free camera's edge where the landmark has one ...
    has = np.zeros(len(p["points"]), bool); has[p["edge_point"][one]] = True
    one |= first_edge_of(p, thin & ~has[p["edge_point"]])                  # ... its first edge otherwise
    q = rebuild(p, keep=~thin | one)
    if mono:
        q["obs"][q["edge_point"] % 5 == 0, 2] = -1.0
    return q


def single_observer(n_points=900):
    n = (n_points + 4) // 5
    return _single_observer(n_points, False), dict(landmarks_of_degree={1: n}, degree_of_landmarks=(np.arange(0, n_points, 5), 1))


def single_observer_mono(n_points=900):
    n = (n_points + 4) // 5
    return _single_observer(n_points, True), dict(landmarks_of_degree={1: n}, degree_of_landmarks=(np.arange(0, n_points, 5), 1),
                                                  mono_landmarks=np.arange(0, n_points, 5))


def fixed_only(n_points=900):
    p = window_base(n_points)
    # (every 6th from landmark 1 on: drawn from 0 on, landmark 858 -- two inlier observations 4 cm apart that contradict each other -- wanders 4.6 m in depth and carries
    #  6e-4 of that when the ORACLE's inputs move by one ulp; the gate of tests/test_ba_shapes_cpu.py re-draws such a shape)
    lm = np.arange(1, n_points, 6)
    sel = p["edge_point"] % 6 == 1
    q = rebuild(p, keep=~sel | (p["edge_cam"] <= 1), extra=[(i, c) for i in lm for c in (0, 1)], seed=8810)
    return q, dict(landmarks_without_free_observer=lm, degree_of_landmarks=(lm, 2))


def long_tracks(n_points=900):
    p = window_base(n_points)
    lm = 3 + 22 * np.arange(40)
    q = rebuild(p, extra=[(i, c) for i in lm for c in range(15)], seed=8811)
    return q, dict(degree_of_landmarks=(lm, 15), free_observers_of_landmarks=(lm, 12), max_free_observers=12)


def skewed(n_points=900):
    p = window_base(n_points)
    ec = p["edge_cam"]
    keep = (ec != 6) & (ec != 7)
    keep[np.flatnonzero(ec == 6)[:4]] = True
    q = rebuild(p, keep=keep, extra=[(i, 5) for i in range(n_points)], seed=8812)
    return q, dict(camera_degree={5: n_points, 6: 4, 7: 0}, every_landmark_observed=True)


def _scatter(p, sel, du, dv, unit_weight=False):
    """the observations `sel` moved by (du, dv) pixels; the right coordinate moves with u (the disparity, hence the depth the edge asks for, stays).  unit_weight: those
    edges get inv_sigma2 = 1 (with weights as unequal as 1 : 0.08 -- octave 0 beside octave 7 -- a landmark simply follows its heaviest observation, which then is an inlier)"""
    q = dict(p)
    obs = p["obs"].copy()
    stereo = obs[sel, 2] >= 0
    obs[sel, 0] += du.astype(np.float32); obs[sel, 1] += dv.astype(np.float32)
    ur = obs[sel, 2] + np.where(stereo, du, 0.0).astype(np.float32)
    obs[sel, 2] = np.where(stereo & (ur <= MIN_UR), -1.0, ur)
    q["obs"] = obs
    if unit_weight:
        q["inv_sigma2"] = np.where(sel, np.float32(1.0), p["inv_sigma2"]).astype(np.float32)
    return q


def camera_all_outliers(n_points=900):
    """80 px in u and in v, each observation with signs of its own: no pose of camera 9 explains them"""
    p = window_base(n_points)
    sel = p["edge_cam"] == 9
    rng = np.random.default_rng(8813)
    n = int(sel.sum())
    return _scatter(p, sel, 80.0 * rng.choice([-1.0, 1.0], n), 80.0 * rng.choice([-1.0, 1.0], n)), dict(rejected_edges=sel, rejected_camera=9)


def landmarks_all_outliers(n_points=900):
    """70 px, the k-th of a landmark's m observations in the direction 2 pi k / m (+ a phase per landmark): the shifts of one landmark add up to nothing, and no two of
    them are closer than 53 px (m = 8) -- no position of the landmark explains two of them at once"""
    p = window_base(n_points)
    sel = p["edge_point"] % 9 == 0
    deg = np.bincount(p["edge_point"], minlength=n_points)
    start = np.concatenate([[0], np.cumsum(deg)[:-1]])
    k = np.arange(len(p["edge_point"])) - start[p["edge_point"]]          # (the edge list is grouped by landmark)
    phase = np.random.default_rng(8814).uniform(0, 2 * np.pi, n_points)
    ang = (2 * np.pi * k / deg[p["edge_point"]] + phase[p["edge_point"]])[sel]
    return _scatter(p, sel, 70.0 * np.cos(ang), 70.0 * np.sin(ang), unit_weight=True), dict(rejected_edges=sel, rejected_landmarks=np.arange(0, n_points, 9))


def one_free():
    p = synth.synth_ba(n_free=1, n_fixed=2, n_points=150, seed=8801)
    return p, dict(free_cameras=1, fixed_cameras=2)


def all_mono():
    p = synth.synth_ba(n_free=6, n_fixed=2, n_points=300, seed=8802, mono_frac=1.0)
    return p, dict(stereo_edges=0)


def tile_limit_emptied():
    """30 free keyframes -- the register-tile solver's limit: 180 unknowns, the last tile rows padded -- of which one in the middle and the very last lose every edge:
    the solver's own identity padding and a camera block that is lambda * I meet in one factorisation."""
    p = synth.synth_ba(n_free=30, n_fixed=3, n_points=1500, seed=8803)
    q = rebuild(p, keep=(p["edge_cam"] != 17) & (p["edge_cam"] != 32))
    return q, dict(camera_degree={17: 0, 32: 0}, free_cameras=30)


# ---------------------------------------------------------------------------------------------------------------- map scale
def map_base():
    return synth.synth_ba(n_free=70, n_fixed=1, n_points=2800, seed=8900, band=7, outlier_frac=0.0)


def hub():
    p = map_base()
    lm = np.arange(len(p["points"]))
    see = lm[visible(p, lm, np.full(len(lm), 35))][::2]
    q = rebuild(p, extra=[(i, 35) for i in see], seed=8910)
    return q, dict(camera_degree_at_least={35: 1200}, covisible_cameras_at_least=(35, 60))


def long_tracks_map():
    p = map_base()
    nc = len(p["poses"])
    lm = np.arange(0, len(p["points"]), 93)
    pt, cam = np.repeat(lm, nc), np.tile(np.arange(nc), len(lm))
    ok = visible(p, pt, cam)
    q = rebuild(p, extra=np.stack([pt[ok], cam[ok]], axis=1), seed=8911)
    return q, dict(max_degree_at_least=40, landmarks_of_degree_at_least=(30, 20))


def thin_map():
    p = map_base()
    ec, ep = p["edge_cam"], p["edge_point"]
    keep = (ep % 5 != 0) | first_edge_of(p)
    keep &= ep % 50 != 2
    keep &= ec != 20
    k41 = np.flatnonzero(keep & (ec == 41))
    keep[k41[3:]] = False
    q = rebuild(p, keep=keep)
    gaps = np.arange(2, len(p["points"]), 50)
    return q, dict(camera_degree={20: 0, 41: 3}, degree_of_landmarks=(gaps, 0), landmarks_of_degree_at_least_count={1: 400})


def hub_last():
    """A hub that is also the LAST camera of the map: in every elimination order it is eliminated last (natural order) or sits behind the last separator -- its dense row is
    the bottom row of the factor, its diagonal pair the longest list, and the last panel is the one the identity padding joins."""
    p = map_base()
    lm = np.arange(len(p["points"]))
    see = lm[visible(p, lm, np.full(len(lm), 70))][::2]
    q = rebuild(p, extra=[(i, 70) for i in see], seed=8913)      # (seed 8912 fails the conditioning gate: one landmark at the edge of the outlier test)
    return q, dict(camera_degree_at_least={70: 700}, covisible_cameras_at_least=(70, 40))


WINDOW_SHAPES = dict(single_observer=single_observer, single_observer_mono=single_observer_mono, fixed_only=fixed_only, long_tracks=long_tracks, skewed=skewed,
                     camera_all_outliers=camera_all_outliers, landmarks_all_outliers=landmarks_all_outliers, one_free=one_free, all_mono=all_mono,
                     tile_limit_emptied=tile_limit_emptied)
MAP_SHAPES = dict(hub=hub, long_tracks_map=long_tracks_map, thin_map=thin_map, hub_last=hub_last)
SHAPES = dict(WINDOW_SHAPES, **MAP_SHAPES)
# the entry points a shape is used with: (name, oracle call, library call).  Window shapes go through all three; the map shapes too (LocalBundleAdjustment on an
# oversized window runs both passes on the map-scale path).
ENTRY_POINTS = ("local_ba", "ba_robust", "ba_plain")


def ba_iterations(p):
    """BundleAdjustment iterations: 8 on the map shapes (as every map-scale test of tests/test_gpu_lm.py), the entry point's default of 5 on the windows.  The windows carry
    synth_ba's 5 % of gross outliers; WITHOUT robust kernels a two-observer landmark with one of them wanders for metres from the sixth iteration on (8 - 10 m on
    single_observer, where the oracle's own one-ulp band then is 1.3e-4 - 3.4e-4 of the update; 1.5e-5 at five iterations) -- no implementation can be compared there."""
    return 8 if int((p["fixed"] == 0).sum()) > 64 else 5

_cache = {}


def shape(name):
    """(problem, facts) of a named shape, built once per process (callers must not write into the arrays)"""
    if name not in _cache:
        _cache[name] = SHAPES[name]()
    return _cache[name]


def run_oracle(O, entry, p):
    if entry == "local_ba":
        return O.local_ba(p)
    return O.bundle_adjustment(p, ba_iterations(p), entry == "ba_robust")


def run_library(E, entry, p):
    if entry == "local_ba":
        return E.Optimizer.LocalBundleAdjustment(p)
    return E.Optimizer.BundleAdjustment(p, ba_iterations(p), bRobust=entry == "ba_robust")


def check_facts(p, facts):
    """every claim of `facts` against the census of `p`; returns the list of claims that do not hold (empty: all hold)"""
    c = census(p)
    nc = len(p["poses"])
    bad = []

    def claim(ok, text):
        if not ok:
            bad.append(text)
    for key, val in facts.items():
        if key == "landmarks_of_degree":
            for d, n in val.items():
                claim(int((c["lm_deg"] == d).sum()) == n, "%d landmarks of degree %d (found %d)" % (n, d, int((c["lm_deg"] == d).sum())))
        elif key == "landmarks_of_degree_at_least_count":
            for d, n in val.items():
                claim(int((c["lm_deg"] == d).sum()) >= n, "at least %d landmarks of degree %d (found %d)" % (n, d, int((c["lm_deg"] == d).sum())))
        elif key == "degree_of_landmarks":
            claim(np.all(c["lm_deg"][val[0]] == val[1]), "the chosen landmarks have degree %d" % val[1])
        elif key == "free_observers_of_landmarks":
            claim(np.all(c["lm_free"][val[0]] == val[1]), "the chosen landmarks have %d free observers" % val[1])
        elif key == "max_free_observers":
            claim(int(c["lm_free"].max()) == val, "most free observers of a landmark: %d (found %d)" % (val, int(c["lm_free"].max())))
        elif key == "landmarks_without_free_observer":
            claim(np.all(c["lm_free"][val] == 0) and np.all(c["lm_deg"][val] > 0), "the chosen landmarks have edges, none to a free camera")
        elif key == "mono_landmarks":
            claim(np.all(c["mono"][np.isin(p["edge_point"], val)]), "every edge of the chosen landmarks is monocular")
        elif key == "camera_degree":
            for cam, d in val.items():
                claim(int(c["cam_deg"][cam]) == d and not p["fixed"][cam], "free camera %d has %d edges (found %d)" % (cam, d, int(c["cam_deg"][cam])))
        elif key == "camera_degree_at_least":
            for cam, d in val.items():
                claim(int(c["cam_deg"][cam]) >= d and not p["fixed"][cam], "free camera %d has at least %d edges (found %d)" % (cam, d, int(c["cam_deg"][cam])))
        elif key == "covisible_cameras_at_least":
            cam, n = val
            mine = np.zeros(len(p["points"]), bool); mine[p["edge_point"][p["edge_cam"] == cam]] = True
            others = np.unique(p["edge_cam"][mine[p["edge_point"]]])
            claim(len(others) - 1 >= n, "camera %d shares a landmark with at least %d others (found %d)" % (cam, n, len(others) - 1))
        elif key == "every_landmark_observed":
            claim(int(c["lm_deg"].min()) >= 1, "no landmark without edges")
        elif key == "max_degree_at_least":
            claim(int(c["lm_deg"].max()) >= val, "a landmark with at least %d observers (most: %d)" % (val, int(c["lm_deg"].max())))
        elif key == "landmarks_of_degree_at_least":
            d, n = val
            claim(int((c["lm_deg"] >= d).sum()) >= n, "at least %d landmarks with %d observers or more (found %d)" % (n, d, int((c["lm_deg"] >= d).sum())))
        elif key == "free_cameras":
            claim(int((p["fixed"] == 0).sum()) == val, "%d free cameras" % val)
        elif key == "fixed_cameras":
            claim(int((p["fixed"] != 0).sum()) == val, "%d fixed cameras" % val)
        elif key == "stereo_edges":
            claim(int((~c["mono"]).sum()) == val, "%d stereo edges (found %d)" % (val, int((~c["mono"]).sum())))
        elif key in ("rejected_edges", "rejected_camera", "rejected_landmarks"):
            pass      # (held against the ORACLE's outlier table by the CPU test: a property of the solution, not of the graph)
        else:
            bad.append("unknown claim %s" % key)
    # what every shape promises: a well-formed list in adapter order, one edge per (camera, point), no right coordinate that a one-ulp probe could carry across zero
    key = p["edge_point"].astype(np.int64) * nc + p["edge_cam"]
    claim(np.all(np.diff(key) > 0), "edges grouped by landmark, ascending camera, no pair twice")
    claim(not np.any(p["obs"][:, 2] == 0.0), "no right coordinate is exactly zero")
    claim(not np.any((p["obs"][:, 2] > 0) & (p["obs"][:, 2] < 1e-3)), "no right coordinate within a rounding error of zero")
    return bad


def one_ulp(p, seed):
    """`p` with every float32 entry of points / obs / poses moved ONE ulp up or down at random (the probe of tests/test_gpu_lm_conditioning.py).  The monocular markers
    (ur < 0) and the bottom row of the poses stay as they are, and no value moves across (or off) zero."""
    rs = np.random.default_rng(9000 + seed)
    q = dict(p)
    for k in ("points", "obs", "poses"):
        a = p[k]
        up = rs.integers(0, 2, size=a.shape).astype(bool)
        b = np.where(up, np.nextafter(a, np.float32(np.inf)), np.nextafter(a, np.float32(-np.inf))).astype(np.float32)
        q[k] = np.where((a == 0) | (np.sign(b) != np.sign(a)), a, b)
    q["obs"][:, 2] = np.where(p["obs"][:, 2] < 0, p["obs"][:, 2], q["obs"][:, 2])
    q["poses"][:, 3, :] = p["poses"][:, 3, :]
    return q


def displacement(a, b, old):
    """largest |a - b| relative to the largest update |b - old|, and its flat index"""
    upd = max(np.abs(b.astype(np.float64) - old.astype(np.float64)).max(), 1e-6)
    d = np.abs(a.astype(np.float64) - b.astype(np.float64))
    return float(d.max() / upd), int(d.argmax())


def oracle_band(O, entry, p, runs=6):
    """The conditioning gate of one (shape, entry point): `runs` one-ulp perturbed oracle runs against the unperturbed one.  Returns dict(schedule_stable, poses, points):
    whether iters (and the outlier table) stayed the same in every run, and the largest displacement of poses / points relative to the largest update."""
    o = run_oracle(O, entry, p)
    out = dict(schedule_stable=True, poses=0.0, points=0.0)
    for s in range(runs):
        o2 = run_oracle(O, entry, one_ulp(p, s))
        same = list(o2["iters"]) == list(o["iters"])
        if entry == "local_ba":
            same = same and np.array_equal(o2["edge_outlier"], o["edge_outlier"])
        out["schedule_stable"] = out["schedule_stable"] and same
        for k in ("poses", "points"):
            out[k] = max(out[k], displacement(o2[k], o[k], p[k])[0])
    return out
