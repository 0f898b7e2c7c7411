"""Seeded scenes for the object layer's data association: Object_2D::NoParaDataAssociation (reference src/Object.cc:728-962) and
Object_Map::ComputeProjectRectFrame (:1606-1651).  Each scene is the smallest at which the branch it is named for can still go wrong;
tools/gen_golden_object_association.py runs the yardstick (tests/object_association_reference.py) on them and records tests/golden/object_association/*.npz.

np_scenes():   name -> dict(det (m, 3), map (nGood, 3), S, branch): the good points of a detection and of a map object, mvpMapObjectMappoints.size(), and what the
               scene must reach (tests/test_object_association_reference_cpu.py checks it): verdict, and optionally step, n, and the axes that fail
rect_scenes(): name -> dict(points, Tcw, fx, fy, cx, cy, cols, rows, status)"""
import numpy as np

MIN_POINTS, SAMPLE_RATIO = 20, 3      # src/Object.cc:760 / :764, :776 (held to the reference text by tests/golden/object_association_constants.json)
# the kernel's shapes (csrc/object_assoc.hip; the CPU test holds them to the source): workgroup size, detection points per thread and pass, map points per tile
BLOCK, OWNED, TILE = 256, 2, 1024
INT32_MAX = 2 ** 31 - 1


def _gauss(n, seed, centre=(0.5, -0.3, 2.0), sigma=0.2):
    rs = np.random.RandomState(seed)
    return np.ascontiguousarray(np.asarray(centre) + rs.normal(0.0, sigma, (n, 3)), np.float32)


def _pair(det, mp, S=None, **branch):
    mp = np.ascontiguousarray(mp, np.float32).reshape(-1, 3)
    return dict(det=np.ascontiguousarray(det, np.float32).reshape(-1, 3), map=mp, S=len(mp) if S is None else S, branch=branch)


def largest_m_under_the_bound(n):
    """the largest m with m * n * (m + n + 1) <= INT32_MAX"""
    m = 1
    while (m + 1) * n * (m + 1 + n + 1) <= INT32_MAX:
        m += 1
    return m


def np_scenes():
    sc = {}
    # the early returns (:760, :764): m is looked at first
    sc["m19"] = _pair(_gauss(19, 1), _gauss(60, 2), verdict=0)
    sc["m20"] = _pair(_gauss(20, 3), _gauss(60, 4), step=1, n=60)
    sc["ngood19"] = _pair(_gauss(30, 5), _gauss(19, 6), verdict=2, early=True)
    sc["ngood20"] = _pair(_gauss(30, 7), _gauss(20, 8), step=1, n=20)
    sc["m19_ngood19"] = _pair(_gauss(19, 9), _gauss(19, 10), verdict=0)
    sc["no_good_map_points"] = _pair(_gauss(30, 11), np.zeros((0, 3), np.float32), S=5, verdict=2, early=True)
    # the sampling threshold (:776) and the step taken from S with the bad points (:779)
    sc["ngood_3m"] = _pair(_gauss(30, 12), _gauss(90, 13), step=1, n=90, sampled=False)
    sc["ngood_3m_plus_1"] = _pair(_gauss(30, 14), _gauss(91, 15), step=1, n=91, sampled=True)
    sc["bad_points_step_2"] = _pair(_gauss(30, 16), _gauss(91, 17), S=210, step=2, n=46, sampled=True)        # 91 is no multiple of 2
    sc["bad_points_even"] = _pair(_gauss(30, 18), _gauss(92, 19), S=210, step=2, n=46, sampled=True)
    sc["step_3_remainder"] = _pair(_gauss(20, 20), _gauss(100, 21), S=185, step=3, n=34, sampled=True)        # 100 = 3 * 33 + 1
    # ties on every axis: the detection's points ARE map points (the normal case upstream), and a lattice
    mp = _gauss(120, 22)
    sc["det_points_are_map_points"] = _pair(mp[::3], mp, ties=True, sampled=False)
    mp = _gauss(250, 23)
    sc["det_points_are_map_points_sampled"] = _pair(mp[:40], mp, ties=True, step=2, n=125, sampled=True)
    sc["lattice"] = _pair(np.round(_gauss(40, 24) * 8) / 8, np.round(_gauss(130, 25) * 8) / 8, ties=True, sampled=True)
    # -0.0f against +0.0f: equal in every compare, in either order inside std::sort
    rs = np.random.RandomState(26)
    d, mp = _gauss(24, 27, (0, 0, 0)), _gauss(80, 28, (0, 0, 0))
    d[rs.rand(24, 3) < 0.4] = 0.0
    d[rs.rand(24, 3) < 0.2] = -0.0
    mp[rs.rand(80, 3) < 0.3] = -0.0
    mp[rs.rand(80, 3) < 0.2] = 0.0
    sc["signed_zeros"] = _pair(d, mp, ties=True, sampled=True)
    # infinities compare normally
    d, mp = _gauss(25, 29), _gauss(90, 30)
    d[0, 0], d[1, 1], d[2, 2], d[3, 0] = np.inf, -np.inf, np.inf, -np.inf
    mp[0, 0], mp[1, 0], mp[2, 1], mp[3, 2], mp[4, 2] = np.inf, -np.inf, -np.inf, np.inf, np.inf
    sc["infinities"] = _pair(d, mp, ties=True, sampled=True)
    # the verdicts: one distribution (1), and one axis shifted (2 through that axis alone)
    mp = _gauss(300, 31)
    sc["same_distribution"] = _pair(mp[1::3], mp, verdict=1)
    for a, name in enumerate("xyz"):
        shift = np.zeros(3, np.float32)
        shift[a] = 0.25
        sc["shifted_" + name] = _pair(mp[1::3] + shift, mp, verdict=2, fails=(a,))
    # detection sizes around the wavefront, the workgroup (a thread's second point) and a second pass
    for m in (63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, BLOCK * OWNED - 1, BLOCK * OWNED, BLOCK * OWNED + 1):
        sc["m%d" % m] = _pair(_gauss(m, 100 + m), _gauss(45, 200 + m))
    # map sizes around the LDS tile: sampled (cheap for the literal form) and once unsampled
    for k in (TILE - 1, TILE, TILE + 1, 2 * TILE + 1):
        sc["ngood%d" % k] = _pair(_gauss(24, 300 + k), _gauss(k, 400 + k), sampled=True)
    sc["ngood%d_unsampled" % (TILE + 1)] = _pair(_gauss((TILE + 1 + 2) // 3, 41), _gauss(TILE + 1, 42), step=1, n=TILE + 1, sampled=False)
    # the overflow bound of m * n * (m + n + 1): the largest m under it for n = 20, and the first above
    mb = largest_m_under_the_bound(20)
    sc["bound_under"] = _pair(_gauss(mb, 43), _gauss(20, 44), n=20, defined=True)
    sc["bound_over"] = _pair(_gauss(mb + 1, 45), _gauss(20, 46), verdict=3, n=20, step=1)
    return sc


def _pose(seed):
    """a small rotation and translation: no entry of Rcw is 0 or 1"""
    rs = np.random.RandomState(seed)
    ax = rs.normal(0, 1, 3)
    ax /= np.linalg.norm(ax)
    th = 0.2
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    T[:3, 3] = rs.uniform(-0.2, 0.2, 3)
    return np.ascontiguousarray(T, np.float32)


IDENTITY = np.eye(4, dtype=np.float32)
CAM = dict(fx=517.3, fy=516.5, cx=318.6, cy=255.3, cols=640, rows=480)


def _rect(points, Tcw, status, **kw):
    cam = dict(CAM)
    cam.update(kw)
    return dict(points=np.ascontiguousarray(points, np.float32).reshape(-1, 3), Tcw=np.ascontiguousarray(Tcw, np.float32), status=status, **cam)


def rect_scenes():
    sc = {}
    sc["in_view"] = _rect(_gauss(50, 50, (0.1, -0.1, 3.0), 0.15), _pose(1), 1, clamps=())
    sc["left_and_above"] = _rect(_gauss(40, 51, (-1.9, -1.4, 3.0), 0.3), _pose(2), 1, clamps=("x_min", "y_min"))
    sc["right_and_below"] = _rect(_gauss(40, 52, (1.9, 1.4, 3.0), 0.3), _pose(3), 1, clamps=("x_max", "y_max"))
    sc["all_four_clamps"] = _rect(_gauss(70, 53, (0.0, 0.0, 2.0), 1.2), _pose(4), 1, clamps=("x_min", "y_min", "x_max", "y_max"))
    p = _gauss(30, 54, (0.1, 0.1, 3.0), 0.15)
    p[7] = (0.4, -0.3, -2.0)
    sc["point_behind_the_camera"] = _rect(p, IDENTITY, 1)
    p = _gauss(30, 55, (0.1, 0.1, 3.0), 0.15)
    p[3] = (1.0, -1.0, 0.0)          # z = 0, xc and yc not 0: u = +inf, v = -inf, both defined and clamped
    sc["z0_infinite"] = _rect(p, IDENTITY, 1)
    p = _gauss(30, 56, (0.1, 0.1, 3.0), 0.15)
    p[29] = (0.0, 0.5, 0.0)          # z = 0 and xc = 0: fx * 0 * inf is a NaN
    sc["z0_nan"] = _rect(p, IDENTITY, 2)
    sc["box_right_of_int"] = _rect(np.array([[1.0, 1.0, 1e-8], [1.5, 1.2, 1e-8]], np.float32), IDENTITY, 2)      # x_min about 5e10: only x_max is clamped
    sc["width_minus_infinity"] = _rect(np.array([[-1.0, 1.0, 0.0]], np.float32), IDENTITY, 2)                  # x_min -> 0, x_max = -inf
    sc["no_points"] = _rect(np.zeros((0, 3), np.float32), _pose(5), 0)
    sc["one_point"] = _rect(np.array([[0.2, 0.1, 2.5]], np.float32), _pose(6), 1)
    for n in (63, 64, 65, 129):      # around the wavefront's lanes
        sc["points_%d" % n] = _rect(_gauss(n, 60 + n, (0.0, 0.0, 3.0), 0.4), _pose(7 + n), 1)
    return sc
