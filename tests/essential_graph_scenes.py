"""Seeded OptimizeEssentialGraph problems (the eao_essential_graph_problem fields as numpy arrays; tests/essential_graph_reference.py says
what they mean) for the pose-graph tests, the golden generator and the benchmark helper.

The base scene: n keyframes on a circle looking inwards; the estimated trajectory is the true one composed with a drift that grows from
keyframe to keyframe (rotation, translation and -- optionally -- scale).  Keyframe 0 plays pLoopKF, keyframe n - 1 pCurKF: it and a few
keyframes before it carry a CorrectedSim3 (the loop's Sim3 propagated as LoopClosing::CorrectLoop does: S_ic * S_cw) and keep their drifted
pose as NonCorrectedSim3.  Every keyframe has a spanning-tree edge to its predecessor (kind 1), there are random covisibility chords
(kind 1) and one loop-connection edge from the current keyframe to the loop keyframe (kind 0)."""
import math

import numpy as np

from sim3_reference import Sim3, sim3_exp


def _rows(S):
    return np.concatenate([S.q, S.t, [S.s]])


def _sim3_of_row(r):
    return Sim3(r[0:4], r[4:7], r[7])


def ring(n=40, seed=0, fix_scale=False, rot_drift=2e-3, trans_drift=5e-3, scale_drift=0.0, loop_scale=None, n_corrected=3, n_chords=None,
         chord_span=6, fixed=0, n_points=24, radius=4.0):
    """rot_drift / trans_drift: standard deviation of the drift added per keyframe (radians, metres); scale_drift: relative scale change
    per keyframe; loop_scale: scale of the current keyframe's CorrectedSim3 (default: the accumulated scale drift, exactly 1 without)."""
    rng = np.random.default_rng(seed)
    true = []
    for k in range(n):
        a = 2 * math.pi * k / n
        w = np.array([0.05 * math.sin(3 * a), 0.05 * math.cos(2 * a), a])
        Rk = sim3_exp(np.concatenate([w, np.zeros(4)]))
        c = np.array([radius * math.cos(a), radius * math.sin(a), 0.2 * math.sin(2 * a)])
        Rk.t = -Sim3(Rk.q, np.zeros(3), 1.0).map(c)
        true.append(Rk)
    # drifted estimate: relative motions with noise, translation scaled by the running scale
    est = [true[0].copy()]
    sc = 1.0
    for k in range(1, n):
        rel = true[k] * true[k - 1].inverse()
        sc *= 1.0 + scale_drift
        rel.t = rel.t * sc
        d = sim3_exp(np.concatenate([rng.normal(size=3) * rot_drift, rng.normal(size=3) * trans_drift, [0.0]]))
        est.append(d * rel * est[k - 1])
    for S in est:
        S.s = 1.0
    Scw = np.stack([_rows(S) for S in est])
    Snc = Scw.copy()
    has_nc = np.zeros(n, np.uint8)
    cur = n - 1
    s_c = sc if loop_scale is None else loop_scale
    # the loop's verdict on the current keyframe: the true pose (in the units of the drifted map at that point), a little noise
    noise = sim3_exp(np.concatenate([rng.normal(size=3) * 1e-3, rng.normal(size=3) * 1e-3, [0.0]]))
    corrected_cur = noise * Sim3(true[cur].q, s_c * true[cur].t, s_c)
    for k in range(max(cur - n_corrected + 1, 1), cur + 1):
        has_nc[k] = 1
        Sic = est[k] * est[cur].inverse()
        Scw[k] = _rows(Sic * corrected_cur)
    edges = [(k, k - 1, 1) for k in range(1, n)]
    n_chords = n // 2 if n_chords is None else n_chords
    for _ in range(n_chords):
        i = int(rng.integers(2, n))
        j = max(i - int(rng.integers(2, chord_span + 1)), 0)
        edges.append((i, j, 1))
    if n > 1:
        edges.append((cur, 0, 0))
    prob = dict(n=n, fixed=fixed, fix_scale=bool(fix_scale), Scw=Scw, has_nc=has_nc, Snc=Snc, edges=np.array(edges, np.int32).reshape(-1, 3))
    return with_points(prob, n_points, seed)


def with_points(prob, n_points, seed=0):
    """n_points map points around the ring; the first references nothing (ref = -1), the second the fixed keyframe, the others any keyframe."""
    rng = np.random.default_rng(seed + 7919)
    p = dict(prob)
    p["Xw"] = rng.uniform(-5, 5, (n_points, 3)).astype(np.float32)
    ref = rng.integers(0, prob["n"], n_points).astype(np.int32)
    if n_points > 0:
        ref[0] = -1
    if n_points > 1:
        ref[1] = prob["fixed"]
    if n_points > 8:
        ref[5::8] = -1
    p["ref"] = ref
    return p


def with_edges(prob, edges):
    p = dict(prob)
    p["edges"] = np.array(edges, np.int32).reshape(-1, 3)
    return p


def reversed_edges(prob):
    """Every edge (i, j) given as (j, i): the measurement becomes its inverse, the fixed vertex is vertex 0 of its edges."""
    e = prob["edges"]
    return with_edges(prob, np.stack([e[:, 1], e[:, 0], e[:, 2]], axis=1))


def hub(prob, centre, n_extra, seed=0):
    """n_extra more normal edges between keyframe `centre` and other keyframes."""
    rng = np.random.default_rng(seed + 31)
    others = [k for k in range(prob["n"]) if k != centre]
    pick = rng.choice(others, size=n_extra, replace=n_extra > len(others))
    extra = [(max(centre, int(k)), min(centre, int(k)), 1) for k in pick]
    return with_edges(prob, list(map(tuple, prob["edges"])) + extra)


def edge_count(prob, m, seed=0):
    """Exactly m edges: random chords added (or the last chords dropped, never the loop edge)."""
    rng = np.random.default_rng(seed + 57)
    e = list(map(tuple, prob["edges"]))
    loop = e.pop()
    while len(e) + 1 < m:
        i = int(rng.integers(2, prob["n"]))
        j = int(rng.integers(0, i - 1))
        e.append((i, j, 1))
    e = e[:m - 1] + [loop]
    assert len(e) == m
    return with_edges(prob, e)


def isolate(prob, v):
    """Keyframe v loses every edge (its successor's spanning-tree edge goes to its predecessor); the third map point references it."""
    e = []
    for i, j, k in map(tuple, prob["edges"]):
        if i == v:
            continue
        if j == v:
            if i == v + 1 and k == 1:
                e.append((i, v - 1, 1))
            continue
        e.append((i, j, k))
    p = with_edges(prob, e)
    ref = p["ref"].copy()
    ref[2] = v
    p["ref"] = ref
    p["isolated"] = v
    return p


def star(prob):
    """Every other keyframe linked to the fixed one, by a normal and a loop-connection edge, and to nothing else: no pair of free vertices has an edge, so nothing but a vertex's own block keeps the
    tiles it lies in alive -- and the 10th free vertex's seven rows (63 .. 69) lie across the first 64-row tile boundary."""
    f = prob["fixed"]
    e = [(k, f, kind) for k in range(prob["n"]) if k != f for kind in (1, 0)]      # (both kinds: where a NonCorrectedSim3 exists they disagree, so chi2 does not end at zero)
    return with_edges(prob, e)


def straddle_far(prob, v=10, far=(25, 30)):
    """Keyframe v (with keyframe 0 fixed the 10th free vertex, rows 63 .. 69 of the natural order) keeps no edge but two to keyframes whose rows lie two and
    three tiles further down; its neighbours on the line are linked past it."""
    e = [(i, j, k) for i, j, k in map(tuple, prob["edges"]) if i != v and j != v]
    e += [(v + 1, v - 1, 1)] + [(w, v, 1) for w in far]
    return with_edges(prob, e)


def ulp_perturbed(prob, seed=0):
    """The same problem with every entry of Scw and Snc moved to a neighbouring double (the chaos probe of the parity tests)."""
    rng = np.random.default_rng(seed)
    p = dict(prob)
    for k in ("Scw", "Snc"):
        a = np.asarray(prob[k], np.float64)
        direction = np.where(rng.random(a.shape) < 0.5, -np.inf, np.inf)
        p[k] = np.nextafter(a, direction)
    return p


def permutation(prob, seed=0):
    """A random elimination order of the active free vertices (the `perm` argument of the yardstick)."""
    from essential_graph_reference import Graph
    return np.random.default_rng(seed + 99).permutation(len(Graph(prob).free))


def planted(n=12, seed=0):
    """A consistent graph: every measurement equals the relative pose of the estimates it links (no drift to distribute)."""
    p = ring(n=n, seed=seed, rot_drift=1e-2, trans_drift=2e-2, n_corrected=0)
    p["has_nc"] = np.zeros(n, np.uint8)
    return p


# ---------------------------------------------------------------------- the families of the parity tests: name -> builder(fix_scale)
FAMILIES = {
    "dup2": lambda fs: with_edges(ring(n=2, seed=101, fix_scale=fs, n_corrected=1, n_chords=0, rot_drift=2e-2, trans_drift=5e-2), [(1, 0, 1), (1, 0, 0)]),
    "ring9": lambda fs: ring(n=9, seed=102, fix_scale=fs),
    "ring10": lambda fs: ring(n=10, seed=103, fix_scale=fs),
    "ring65": lambda fs: ring(n=65, seed=104, fix_scale=fs),            # 64 free vertices: 448 rows, exactly seven 64-row tiles
    "ring66": lambda fs: ring(n=66, seed=105, fix_scale=fs),            # one vertex past that boundary
    "ring40": lambda fs: ring(n=40, seed=106, fix_scale=fs),
    "reversed": lambda fs: reversed_edges(ring(n=40, seed=106, fix_scale=fs)),
    "fixed_middle": lambda fs: ring(n=40, seed=107, fix_scale=fs, fixed=20),
    "fixed_last": lambda fs: ring(n=40, seed=108, fix_scale=fs, fixed=39),
    "hub": lambda fs: hub(ring(n=40, seed=109, fix_scale=fs), 11, 35, seed=109),
    "edges63": lambda fs: edge_count(ring(n=40, seed=110, fix_scale=fs), 63, seed=110),
    "edges64": lambda fs: edge_count(ring(n=40, seed=111, fix_scale=fs), 64, seed=111),
    "edges65": lambda fs: edge_count(ring(n=40, seed=112, fix_scale=fs), 65, seed=112),
    "edges257": lambda fs: edge_count(ring(n=40, seed=113, fix_scale=fs), 257, seed=113),
    "isolated": lambda fs: isolate(ring(n=40, seed=114, fix_scale=fs), 17),
    "drift_small": lambda fs: ring(n=40, seed=115, fix_scale=fs, rot_drift=2e-5, trans_drift=1e-3),        # every edge error in the d > 1 - eps branch
    "drift_large": lambda fs: ring(n=40, seed=116, fix_scale=fs, rot_drift=1.5e-2, trans_drift=2e-2),      # loop-side edges leave it
    "unit_scale": lambda fs: ring(n=40, seed=117, fix_scale=fs, loop_scale=1.0),                           # sigma = 0 everywhere at the start
    "scale_drift": lambda fs: ring(n=40, seed=118, fix_scale=fs, scale_drift=-0.004),                      # about 0.4 % per keyframe
    "star": lambda fs: star(ring(n=12, seed=120, fix_scale=fs)),
    "straddle_far": lambda fs: straddle_far(ring(n=40, seed=121, fix_scale=fs)),
    "ring300": lambda fs: ring(n=300, seed=119, fix_scale=fs, rot_drift=1e-3, trans_drift=3e-3, n_chords=120, chord_span=10),
}
CASES = [(name, fs) for name in FAMILIES for fs in (False, True)]
POINT_COUNTS = (0, 1, 63, 65, 5000)


def case(name, fix_scale):
    return FAMILIES[name](bool(fix_scale))


def case_ids():
    return ["%s-fs%d" % (name, int(fs)) for name, fs in CASES]


# The tables below are written from profiles/essential_graph_bands.txt (tools/essential_graph_bands.py: every case as generated, under
# ulp_perturbed seeds 0..3 and under a permuted elimination order); tests/test_essential_graph_reference_cpu.py keeps them equal to that probe.
# Cases whose yardstick iteration or trial counts move under those perturbations.
ITERS_UNSTABLE = {
    "dup2-fs0", "dup2-fs1", "ring9-fs1", "ring10-fs1", "ring65-fs1", "ring66-fs1",
    "ring40-fs1", "reversed-fs1", "fixed_middle-fs1", "fixed_last-fs1", "hub-fs1", "edges63-fs1",
    "edges64-fs1", "edges65-fs1", "edges257-fs1", "isolated-fs1", "drift_small-fs1", "unit_scale-fs1",
    "scale_drift-fs1", "star-fs0", "star-fs1", "straddle_far-fs1", "ring300-fs1",
}
# Cases on which the yardstick's own displacement exceeds lm_tolerances.UPDATE_REL of its update; at most two.
BANDED = set()
BANDED_MAX = 2


# ---------------------------------------------------------------------- a hand-built map for the class surface (tests/cpp/essential_graph/essential_graph_driver.cpp)
def _pose_matrix(row):
    from sim3_reference import quat_to_R
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = quat_to_R(row[0:4])
    T[:3, 3] = row[4:7]
    return T


def map_text(m):
    f = lambda v: repr(float(v))
    out = ["%d %d %d %d" % (len(m["kfs"]), int(m["fix_scale"]), m["loop"], m["cur"])]
    for kf in m["kfs"]:
        out.append("%d %d %d %s" % (kf["id"], int(kf["bad"]), kf["parent"], " ".join(f(v) for v in np.asarray(kf["T"], np.float32).ravel())))
        out.append("%d %s" % (len(kf["loop_edges"]), " ".join(str(k) for k in kf["loop_edges"])))
        out.append("%d %s" % (len(kf["covisible"]), " ".join("%d %d" % kw for kw in kf["covisible"])))
        out.append("%d %s" % (len(kf["children"]), " ".join(str(k) for k in kf["children"])))
    for key in ("corrected", "non_corrected"):
        out.append(str(len(m[key])))
        out += ["%d %s" % (k, " ".join(f(v) for v in row)) for k, row in m[key]]
    out.append(str(len(m["loop_connections"])))
    out += ["%d %d %s" % (k, len(js), " ".join(str(j) for j in js)) for k, js in m["loop_connections"]]
    out.append(str(len(m["points"])))
    out += ["%s %s %s %d %d %d %d" % (f(x[0]), f(x[1]), f(x[2]), bad, by, cref, ref) for x, bad, by, cref, ref in m["points"]]
    out.append(str(len(m["planes"])))
    out += ["%s %s %s %s %d %d %d %d" % (f(x[0]), f(x[1]), f(x[2]), f(x[3]), bad, by, cref, ref) for x, bad, by, cref, ref in m["planes"]]
    return "\n".join(out) + "\n"


def hand_built_map(fix_scale=False):
    """Eight keyframes with gaps in their mnIds, one of them bad, and one case of every filter of the walk (src/Optimizer.cc:1157-1344).  Returns (the map, the
    scene text, what WalkEssentialGraph must make of it: ids, fixed, the edges in upstream's order with the filter each one passed, has_nc, the points' references)."""
    base = ring(n=8, seed=77, fix_scale=fix_scale, n_corrected=2, n_chords=0)
    ids = [0, 2, 3, 5, 6, 8, 9, 11]
    kf = lambda k, parent, bad=False, loop_edges=(), covisible=(), children=(): dict(
        id=ids[k], bad=bad, parent=parent, T=_pose_matrix(base["Snc"][k]), loop_edges=list(loop_edges), covisible=list(covisible), children=list(children))
    kfs = [
        kf(0, -1, covisible=[(1, 200)], children=[1]),
        kf(1, 0, covisible=[(0, 200), (2, 150), (7, 120), (4, 90)], children=[2]),
        kf(2, 1, covisible=[(1, 150), (4, 130), (0, 110)], children=[3, 4]),
        kf(3, 2, bad=True),
        kf(4, 2, loop_edges=[1, 6], covisible=[(1, 140), (2, 130), (3, 125), (5, 105)], children=[5]),
        kf(5, 4, covisible=[(4, 250), (2, 101), (1, 99)], children=[6]),
        kf(6, 5, loop_edges=[4], covisible=[(4, 300), (3, 200), (1, 40)], children=[7]),
        kf(7, 6, covisible=[(6, 180), (3, 150), (1, 120), (2, 100)]),
    ]
    m = dict(kfs=kfs, fix_scale=fix_scale, loop=0, cur=7,
             corrected=[(6, base["Scw"][6]), (7, base["Scw"][7])], non_corrected=[(6, base["Snc"][6]), (7, base["Snc"][7])],
             loop_connections=[(6, [1]), (7, [0, 1, 3, 6])],
             points=[((1.0, 0.5, -0.25), 0, 0, 0, 1), ((9.0, 9.0, 9.0), 1, 0, 0, 1), ((-2.0, 1.5, 0.75), 0, 11, 8, 0), ((0.5, 0.5, 0.5), 0, 0, 0, 3),
                     ((3.0, -1.0, 0.125), 0, 0, 0, 0), ((-1.0, -2.0, 0.375), 0, 9, 2, 7)],
             planes=[((0.0, 0.6, 0.8, 1.5), 0, 0, 0, 2), ((1.0, 0.0, 0.0, 2.0), 1, 0, 0, 2), ((0.6, 0.0, 0.8, 0.5), 0, 11, 3, 6)])
    expected = dict(
        ids=[0, 2, 3, 6, 8, 9, 11], fixed=0, has_nc=[0, 0, 0, 0, 0, 1, 1],
        edges=[((5, 1, 0), None),                         # (dropped) loop connection 9 -> 2 of weight 40: below minFeat
               ((6, 0, 0), "the (current, loop) pair of weight 0: minFeat's exception"),
               ((6, 1, 0), "loop connection of weight 120"),
               ((6, -1, 0), None),                        # (dropped) loop connection to the bad keyframe 5
               ((6, 5, 0), "loop connection to the current keyframe's parent: the spanning-tree edge below exists as well"),
               ((1, 0, 1), "parent"), ((2, 1, 1), "parent"),
               ((2, 0, 1), "covisibility 110 with a smaller mnId (the parent, the child and the larger mnIds of the same list are not)"),
               ((3, 2, 1), "parent"), ((3, 1, 1), "loop edge with a smaller mnId (the one with the larger mnId 9 is not)"),
               ((4, 3, 1), "parent"), ((4, 2, 1), "covisibility 101 (99 is below minFeat)"),
               ((5, 4, 1), "parent"), ((5, 3, 1), "loop edge; the same keyframe in the covisibility list is skipped by sLoopEdges.count, the bad one by isBad"),
               ((6, 5, 1), "parent"), ((6, 2, 1), "covisibility of exactly 100; keyframe 2 is in sInsertedEdges, keyframe 5 is bad")],
        refs=[1, 4, -1, 0, 6, 2, 2], n_points=5, n_planes=2)
    expected["edges"] = [e for e, why in expected["edges"] if why is not None]
    return m, map_text(m), expected


def problem_of_walk(text):
    """The problem dict of the driver's `walk` output."""
    lines = text.strip().split("\n")
    head = lines[0].split()
    n, fixed, fs = int(head[1]), int(head[3]), int(head[5])
    edges = np.array([[int(v) for v in e.split(",")] for e in lines[2].split()[1:]], np.int32).reshape(-1, 3)
    has = np.array([int(v) for v in lines[3].split()[1:]], np.uint8)
    S = np.array([[float(v) for v in ln.split()[1:]] for ln in lines[4:4 + n]]).reshape(n, 16)
    cnt = lines[4 + n].split()
    ref = np.array([int(v) for v in lines[5 + n].split()[1:]], np.int32)
    X = np.array([float(v) for v in lines[6 + n].split()[1:]], np.float32).reshape(-1, 3)
    return dict(n=n, fixed=fixed, fix_scale=bool(fs), Scw=S[:, :8].copy(), Snc=S[:, 8:].copy(), has_nc=has, edges=edges, Xw=X, ref=ref,
                ids=[int(v) for v in lines[1].split()[1:]], n_map_points=int(cnt[1]), n_planes=int(cnt[3]))
