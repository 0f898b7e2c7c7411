"""Seeded scenes of the plane association (tests/plane_association_reference.py is the yardstick).  A scene is
  planes     [(id, world_pos (4,), xyz (n, 3), Tcw (4, 4) or None)] in add order -- xyz in the camera frame of Tcw, or in the world frame
  M          (n_sets, 4, 4) float32: mTcw of AssociatePlanesByBoundary, Scw of SearchMatchedPlanes
  set_start  CSR over coef;  coef (rows, 4) float32, camera frame
  cand_id    the candidates in the caller's order, or None (every plane in add order)
  dis_th, angle_th
  expect     what the scene claims: match (rows) always; dis / gated as {(row, candidate): value} where the branch is about them
tests/test_plane_association_reference_cpu.py holds the yardstick to every claim; the GPU test holds the library to the yardstick."""
import numpy as np

import plane_association_reference as Y

F = np.float32
I4 = np.eye(4, dtype=np.float32)
UP = np.array([0, 0, 1, 0], np.float32)      # the plane z = 0 seen with the identity pose: d = |z|


def _scene(planes, coef, expect, M=I4, set_start=None, cand_id=None, dis_th=Y.DIS_TH, angle_th=Y.ANGLE_TH):
    coef = np.asarray(coef, np.float32).reshape(-1, 4)
    M = np.asarray(M, np.float32).reshape(-1, 4, 4)
    return dict(planes=[(int(i), np.asarray(w, np.float32), np.asarray(p, np.float32).reshape(-1, 3), None if T is None else np.asarray(T, np.float32))
                        for i, w, p, T in planes],
                M=M, set_start=np.asarray([0, len(coef)] if set_start is None else set_start, np.int32), coef=coef,
                cand_id=None if cand_id is None else [int(c) for c in cand_id], dis_th=F(dis_th), angle_th=F(angle_th), expect=expect)


def at_height(zs, seed=0):
    """points with the given z (their distance from z = 0) and seeded x, y"""
    zs = np.asarray(zs, np.float32).reshape(-1)
    rs = np.random.RandomState(seed)
    return np.stack([rs.uniform(-2, 2, len(zs)).astype(np.float32), rs.uniform(-2, 2, len(zs)).astype(np.float32), zs], 1)


def rot(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def pose(rs, angle=0.4, trans=1.0):
    T = np.eye(4)
    T[:3, :3] = rot(rs.normal(size=3), rs.uniform(-angle, angle))
    T[:3, 3] = rs.uniform(-trans, trans, 3)
    return T


def room(seed):
    """6-10 map planes (walls, floor, ceiling of a box and a few tables), each with a voxel-like boundary cloud seen from its own reference keyframe; the
    frame sees 3-6 of them from a noisy pose"""
    rs = np.random.RandomState(seed)
    n_map, n_frame = int(rs.randint(6, 11)), int(rs.randint(3, 7))
    base = [(1, 0, 0, 3.0), (-1, 0, 0, 3.0), (0, 1, 0, 2.5), (0, -1, 0, 2.5), (0, 0, 1, 1.2), (0, 0, -1, 1.4), (0, 0, 1, 0.5), (0, 0, 1, 0.1), (1, 0, 0, 1.0),
            (0, 1, 0, 0.7)]
    planes, world = [], []
    for k in range(n_map):
        n = np.array(base[k][:3], np.float64)
        d = base[k][3]
        # a frame on the plane n.X + d = 0
        a = np.cross(n, [0.3, 0.5, 0.8]); a /= np.linalg.norm(a)
        b = np.cross(n, a)
        m = int(rs.randint(150, 900))
        uv = rs.uniform(-1.5, 1.5, (m, 2))
        Xw = -d * n + uv[:, :1] * a + uv[:, 1:] * b + rs.normal(0, 0.004, (m, 1)) * n
        Tkf = pose(rs)
        Xc = Xw @ Tkf[:3, :3].T + Tkf[:3, 3]
        w = np.array([n[0], n[1], n[2], d], np.float32)
        planes.append((20 + k, w, Xc.astype(np.float32), Tkf.astype(np.float32)))
        world.append(np.array([n[0], n[1], n[2], d]))
    Tcw = pose(rs)
    seen = [int(s) for s in rs.choice(n_map, n_frame, replace=False)]
    Tn = Tcw.copy()
    Tn[:3, :3] = Tn[:3, :3] @ rot(rs.normal(size=3), 0.01)
    Tn[:3, 3] += rs.normal(0, 0.01, 3)
    coef = [np.linalg.inv(Tn).T @ world[s] for s in seen]      # pi_c = Tcw^-T pi_w, with the noisy pose
    return _scene(planes, coef, dict(match=seen), M=Tcw.astype(np.float32))


def _below(x):
    return np.nextafter(F(x), F(0))


def _above(x):
    return np.nextafter(F(x), F(10))


def tie(order):
    cloud = at_height([0.15, 0.0625, 0.11], 3)
    return _scene([(1, UP, cloud, None), (2, UP, cloud[::-1].copy(), None)], [UP], dict(match=[0], dis={(0, 0): F(0.0625), (0, 1): F(0.0625)}), cand_id=order)


def threshold_distance():
    th = F(0.2)
    return _scene([(1, UP, at_height([th, 0.5]), None), (2, UP, at_height([_below(th), 0.5]), None)], [UP, UP],
                  dict(match=[1, 1], dis={(0, 0): th, (0, 1): _below(th)}))


def threshold_distance_alone():
    th = F(0.2)
    return _scene([(1, UP, at_height([th, 0.5]), None)], [UP], dict(match=[-1], dis={(0, 0): th}, gated={(0, 0): 1}))


def threshold_angle():
    th = F(0.8)
    ws = [(0, 0, th, 0), (0, 0, _above(th), 0), (0, 0, -th, 0), (0, 0, -_above(th), 0)]
    cloud = at_height([0.01])
    # the two at the threshold are gated out although their clouds are at 0.01; candidate 1 is the first to pass
    return _scene([(k + 1, np.array(w, np.float32), cloud, None) for k, w in enumerate(ws)], [UP],
                  dict(match=[1], gated={(0, 0): 0, (0, 1): 1, (0, 2): 0, (0, 3): 1}, dis={(0, 0): F(100), (0, 2): F(100)}))


def from_behind():
    return _scene([(1, -UP, at_height([0.03, 0.4]), None)], [UP], dict(match=[0], gated={(0, 0): 1}, dis={(0, 0): F(0.03)}))


def later_closer():
    return _scene([(1, UP, at_height([0.1]), None), (2, UP, at_height([0.05]), None), (3, UP, at_height([0.07]), None)], [UP],
                  dict(match=[1], dis={(0, 0): F(0.1), (0, 1): F(0.05), (0, 2): F(0.07)}))


def gated_out_closer():
    side = np.array([1, 0, 0, 0], np.float32)
    return _scene([(1, side, at_height([0.01]), None), (2, UP, at_height([0.1]), None)], [UP], dict(match=[1], gated={(0, 0): 0, (0, 1): 1}, dis={(0, 0): F(100)}))


def empty_cloud():
    return _scene([(1, UP, np.zeros((0, 3)), None), (2, UP, at_height([0.15]), None)], [UP], dict(match=[1], gated={(0, 0): 1}, dis={(0, 0): F(100)}))


def only_empty_clouds():
    return _scene([(1, UP, np.zeros((0, 3)), None)], [UP], dict(match=[-1], gated={(0, 0): 1}, dis={(0, 0): F(100)}))


def far_cloud():
    return _scene([(1, UP, at_height([150, 100, 1e30, np.inf]), None)], [UP], dict(match=[-1], gated={(0, 0): 1}, dis={(0, 0): F(100)}))


def nan_point():
    return _scene([(1, UP, at_height([0.15, np.nan, 0.12, np.nan]), None)], [UP], dict(match=[0], dis={(0, 0): F(0.12)}))


def nan_row():
    return _scene([(1, UP, at_height([0.05]), None)], [[0, 0, np.nan, 0], UP, [0, 0, 1, np.nan]],
                  dict(match=[-1, 0, -1], gated={(0, 0): 0, (1, 0): 1, (2, 0): 0}, dis={(0, 0): F(100), (2, 0): F(100)}))      # (0 * NaN: the whole of pM)


def nan_cloud():
    return _scene([(1, UP, at_height([np.nan] * 70), None), (2, UP, at_height([0.19]), None)], [UP], dict(match=[1], gated={(0, 0): 1}, dis={(0, 0): F(100)}))


def permuted_subset():
    planes = [(k + 1, UP, at_height([0.02 * (k + 1)], k), None) for k in range(6)]
    return _scene(planes, [UP], dict(match=[2], dis={(0, 0): F(0.02 * 5), (0, 1): F(0.02 * 3), (0, 2): F(0.02 * 2)}), cand_id=[5, 3, 2, 6])


def same_id_twice():
    planes = [(7, UP, at_height([0.05]), None), (9, UP, at_height([0.1]), None)]
    return _scene(planes, [UP], dict(match=[1], dis={(0, 0): F(0.1), (0, 1): F(0.05), (0, 2): F(0.05)}), cand_id=[9, 7, 7])


def scaled_sim3():
    """SearchMatchedPlanes with Scw = [sR | t]: the normal of pM has length s, so the gate and the distances scale with it"""
    rs = np.random.RandomState(11)
    s = 1.7
    T = pose(rs)
    S = T.copy()
    S[:3, :3] *= s
    world = np.array([0, 0, 1, -0.5])      # the plane z = 0.5
    c = np.linalg.inv(S).T @ world         # so that S^T c is the world plane again
    c2 = c * 0.4                           # |normal| = 0.4 after the product: below the gate although the planes coincide
    cloud = at_height([0.5, 0.53, 0.6], 5)
    return _scene([(1, world.astype(np.float32), cloud, None)], [c, c2], dict(match=[0, -1], gated={(0, 0): 1, (1, 0): 0}), M=S.astype(np.float32))


def three_sets():
    """n_sets = 3 with an empty set in the middle: LoopClosing::SearchAndFuse's connected keyframes against one candidate list"""
    rs = np.random.RandomState(5)
    worlds = [np.array([0, 0, 1, -0.5]), np.array([1, 0, 0, -1.0]), np.array([0, 1, 0, 0.8])]
    planes = []
    for k, w in enumerate(worlds):
        n = w[:3]
        a = np.cross(n, [0.3, 0.5, 0.8]); a /= np.linalg.norm(a)
        b = np.cross(n, a)
        uv = rs.uniform(-1, 1, (40 + 30 * k, 2))
        planes.append((k + 1, w.astype(np.float32), (-w[3] * n + uv[:, :1] * a + uv[:, 1:] * b).astype(np.float32), None))
    Ms = [pose(rs), pose(rs), pose(rs)]
    coef, match = [], []
    for s, rows in ((0, [2, 0]), (2, [1, 0, 2])):
        for r in rows:
            coef.append(np.linalg.inv(Ms[s]).T @ worlds[r])
            match.append(r)
    return _scene(planes, coef, dict(match=match), M=np.array(Ms, np.float32), set_start=[0, 2, 2, 5])


SIZES = [1, 63, 64, 65, 255, 256, 257, Y.CHUNK - 1, Y.CHUNK, Y.CHUNK + 1, 2 * Y.CHUNK + 1]


def sizes():
    """clouds either side of the wavefront, the workgroup and the kernel's chunk, the minimum planted at the LAST point"""
    planes, dis = [], {}
    for k, n in enumerate(SIZES):
        z = np.full(n, 0.19, np.float32)
        z[-1] = F(0.01) * F(k + 2)
        planes.append((k + 1, UP, at_height(z, k), None))
        dis[(0, k)] = z[-1]
    return _scene(planes, [UP], dict(match=[0], dis=dis))


SCENES = {
    "room_0": lambda: room(0), "room_1": lambda: room(1), "room_2": lambda: room(2),
    "tie_ab": lambda: tie([1, 2]), "tie_ba": lambda: tie([2, 1]),
    "threshold_distance": threshold_distance, "threshold_distance_alone": threshold_distance_alone, "threshold_angle": threshold_angle,
    "from_behind": from_behind, "later_closer": later_closer, "gated_out_closer": gated_out_closer,
    "empty_cloud": empty_cloud, "only_empty_clouds": only_empty_clouds, "far_cloud": far_cloud,
    "nan_point": nan_point, "nan_row": nan_row, "nan_cloud": nan_cloud,
    "permuted_subset": permuted_subset, "same_id_twice": same_id_twice, "scaled_sim3": scaled_sim3, "three_sets": three_sets, "sizes": sizes,
}
_cache = {}


def get(name):
    if name not in _cache:
        _cache[name] = SCENES[name]()
    return _cache[name]


def model(sc):
    m = Y.Model()
    for pid, w, xyz, T in sc["planes"]:
        m.add(pid, w, xyz, T)
    return m


_ref = {}


def reference(name, vectorised=False):
    """the yardstick's result on the scene (computed once, shared, never changed)"""
    key = (name, vectorised)
    if key not in _ref:
        sc = get(name)
        r = Y.associate(sc["M"], sc["set_start"], sc["coef"], model(sc).candidates(sc["cand_id"]), sc["dis_th"], sc["angle_th"], vectorised=vectorised)
        for a in r.values():
            a.setflags(write=False)
        _ref[key] = r
    return _ref[key]


def scale_scene(n_planes=300, n_points=2000, rows=12, seed=7):
    """the scale case: world-frame clouds of n_points around n_planes random planes, rows of which the frame sees"""
    rs = np.random.RandomState(seed)
    planes, worlds = [], []
    for k in range(n_planes):
        n = rs.normal(size=3); n /= np.linalg.norm(n)
        d = rs.uniform(0.5, 4.0)
        a = np.cross(n, [0.3, 0.5, 0.8]); a /= np.linalg.norm(a)
        b = np.cross(n, a)
        uv = rs.uniform(-1.5, 1.5, (n_points, 2))
        X = -d * n + uv[:, :1] * a + uv[:, 1:] * b + rs.normal(0, 0.004, (n_points, 1)) * n
        planes.append((k, np.array([n[0], n[1], n[2], d], np.float32), X.astype(np.float32), None))
        worlds.append(np.array([n[0], n[1], n[2], d]))
    Tcw = pose(rs)
    seen = [int(s) for s in rs.choice(n_planes, rows, replace=False)]
    coef = [np.linalg.inv(Tcw).T @ worlds[s] for s in seen]
    return _scene(planes, coef, dict(), M=Tcw.astype(np.float32))      # (no claim: random planes cross, and a crossing cloud may be the nearer one)
