"""Seeded scenes of a map object's cuboid (tests/object_cuboid_reference.py is their yardstick).  An object is a dict: points (n, 3) float32 = GetWorldPos() of
mvpMapObjectMappoints after the erase of the bad ones, centroids (m, 3) float32 = mObjectFrame[i]->_Pos, Ryaw (9,) float32, prev_cuboid_center (3,) float64.
Every scene names the branch it claims (`claims`); tests/test_object_cuboid_reference_cpu.py holds it to that."""
import numpy as np

import object_cuboid_reference as Y

f32, f64 = np.float32, np.float64
STAGE = 1024      # kChunk of csrc/object_cuboid.hip: the staging edge
IDENTITY = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], f32)


def obj(points, centroids, Ryaw=IDENTITY, prev=(0.0, 0.0, 0.0), **claims):
    return dict(points=np.ascontiguousarray(points, f32).reshape(-1, 3), centroids=np.ascontiguousarray(centroids, f32).reshape(-1, 3),
                Ryaw=np.ascontiguousarray(Ryaw, f32).reshape(9), prev_cuboid_center=np.ascontiguousarray(prev, f64).reshape(3), claims=claims)


def cloud(rng, n, centre=(0.5, -0.3, 2.0), spread=(0.3, 0.2, 0.4)):
    return (np.asarray(centre) + rng.standard_normal((n, 3)) * np.asarray(spread)).astype(f32)


def w_negative_angles():
    """the first (rotP, rotR, rotY) of a short list whose Quaterniond(R) has w < 0 before normalizeRotation"""
    for rotR in (3.3, 3.5, 2.9):
        for rotP in (0.1, -0.2):
            for rotY in (0.2, -0.4):
                R = Y.ryaw(rotP, rotR, rotY)
                if Y.quat_branch(R) >= 0 and Y.quat_from_R(R)[3] < 0:
                    return rotP, rotR, rotY
    raise AssertionError("no candidate has w < 0")


def scenes():
    out = {}
    rng = np.random.default_rng(20240613)
    # point counts, with m on both sides of :1071 in turn
    ms = [0, 1, 4, 5, 64, 65]
    for k, n in enumerate([0, 1, 2, 63, 64, 65, 255, 256, 257, STAGE - 1, STAGE, STAGE + 1, 5000]):
        m = ms[k % len(ms)]
        out["n%d_m%d" % (n, m)] = obj(cloud(rng, n), cloud(rng, m, spread=(0.05, 0.05, 0.05)), Y.ryaw(0, 0, 0.1 * k), prev=(0.4, -0.2, 2.1),
                                     n=n, m=m, status=Y.EMPTY if n == 0 else Y.DONE, bounds_written=int(n > 0 and m < 5))
    for m in ms:      # every centroid count beside the same 300 points
        out["m%d" % m] = obj(cloud(rng, 300), cloud(rng, m, spread=(0.05, 0.05, 0.05)), Y.ryaw(0, 0, -0.7), prev=(0.45, -0.35, 2.05), n=300, m=m, status=Y.DONE,
                             bounds_written=int(m < 5))
    out["empty_with_centroids"] = obj(np.zeros((0, 3)), cloud(rng, 7), n=0, m=7, status=Y.EMPTY, bounds_written=0)
    out["all_points_equal"] = obj(np.tile(f32([0.25, -1.5, 3.0]), (40, 1)), cloud(rng, 3), n=40, m=3, status=Y.DONE, bounds_written=1, zero_scale=True)
    p = cloud(rng, 50)
    p[[3, 17, 41]] = p.max(axis=0)      # the maxima three times, the minima twice
    p[[8, 30]] = p.min(axis=0)
    out["repeated_extrema"] = obj(p, cloud(rng, 2), Y.ryaw(0, 0, 0.3), n=50, m=2, status=Y.DONE, bounds_written=1)
    p = np.abs(cloud(rng, 20, centre=(1, 1, 1), spread=(0.2, 0.2, 0.2)))
    p[4] = [0.0, 0.0, 0.0]
    p[9] = [-0.0, -0.0, -0.0]
    out["zero_signs_at_the_minimum"] = obj(p, cloud(rng, 1), n=20, m=1, status=Y.DONE, bounds_written=1, zero_sign=True)
    p = -np.abs(cloud(rng, 20, centre=(1, 1, 1), spread=(0.2, 0.2, 0.2)))
    p[2] = [-0.0, -0.0, -0.0]
    p[11] = [0.0, 0.0, 0.0]
    out["zero_signs_at_the_maximum"] = obj(p, cloud(rng, 4), n=20, m=4, status=Y.DONE, bounds_written=1, zero_sign=True)
    out["cancellation"] = obj(cloud(rng, 200, centre=(1000.0, -1000.0, 1000.0), spread=(1e-3, 1e-3, 1e-3)), cloud(rng, 6, centre=(1000.0, -1000.0, 1000.0), spread=(1e-3,) * 3),
                              prev=(1000.0, -1000.0, 1000.0), n=200, m=6, status=Y.DONE, bounds_written=0)
    out["squares_overflow"] = obj(cloud(rng, 30, centre=(0, 0, 0), spread=(1e20, 1e20, 1e20)), cloud(rng, 3, centre=(0, 0, 0), spread=(1e20,) * 3), n=30, m=3, status=Y.DONE,
                                  bounds_written=1, overflow=True)
    # the quaternion's branches
    out["ryaw_identity"] = obj(cloud(rng, 80), cloud(rng, 2), IDENTITY, n=80, m=2, status=Y.DONE, bounds_written=1, branch=-1)
    out["yaw_only"] = obj(cloud(rng, 80), cloud(rng, 2), Y.ryaw(0, 0, 0.9), n=80, m=2, status=Y.DONE, bounds_written=1, branch=-1)
    out["yaw_third_quadrant"] = obj(cloud(rng, 80), cloud(rng, 2), Y.ryaw(0, 0, -2.4), n=80, m=2, status=Y.DONE, bounds_written=1, branch=2)
    out["roll_near_pi"] = obj(cloud(rng, 80), cloud(rng, 9), Y.ryaw(0.1, 3.0, 0.2), prev=(0.5, -0.3, 2.0), n=80, m=9, status=Y.DONE, bounds_written=0, branch=0)
    out["pitch_near_pi"] = obj(cloud(rng, 80), cloud(rng, 2), Y.ryaw(3.0, 0.1, 0.2), n=80, m=2, status=Y.DONE, bounds_written=1, branch=1)
    out["yaw_near_pi"] = obj(cloud(rng, 80), cloud(rng, 2), Y.ryaw(0.1, 0.2, 3.0), n=80, m=2, status=Y.DONE, bounds_written=1, branch=2)
    out["w_negative"] = obj(cloud(rng, 80), cloud(rng, 2), Y.ryaw(*w_negative_angles()), n=80, m=2, status=Y.DONE, bounds_written=1, w_negative=True)
    out["prev_center_far_away"] = obj(cloud(rng, 120), cloud(rng, 8), Y.ryaw(0, 0, 0.5), prev=(250.0, -400.0, 90.0), n=120, m=8, status=Y.DONE, bounds_written=0, far=True)
    return out


def overlap_scenes():
    out = {}
    rng = np.random.default_rng(977)
    # two unit boxes exactly one length apart on x: dis == sum_half, `<` is strict; the third one overlaps both
    out["touching"] = (Y.make_rows([[0, 0, 0], [1, 0, 0], [0.5, 0.25, 0]], [[1, 1, 1]] * 3), np.array([1, 1, 1], np.uint8))
    out["inside"] = (Y.make_rows([[0, 0, 0], [0.1, -0.1, 0.05]], [[4, 4, 4], [0.5, 0.5, 0.5]]), np.array([1, 1], np.uint8))
    out["ineligible_row"] = (Y.make_rows([[0, 0, 0], [0.2, 0, 0], [0.1, 0.1, 0.1]], [[1, 1, 1]] * 3), np.array([1, 0, 1], np.uint8))
    for m in (1, 2, 64, 65):
        centers = rng.uniform(-2, 2, (m, 3))
        scales = rng.uniform(0.2, 1.5, (m, 3))
        out["m%d" % m] = (Y.make_rows(centers, scales), (rng.uniform(0, 1, m) < 0.85).astype(np.uint8))
    return out


def overlap_large(m=300):
    rng = np.random.default_rng(4242)
    return Y.make_rows(rng.uniform(-6, 6, (m, 3)), rng.uniform(0.2, 2.5, (m, 3))), (rng.uniform(0, 1, m) < 0.9).astype(np.uint8)


def large_object(n=1 << 20):
    rng = np.random.default_rng(31337)
    return obj(cloud(rng, n), cloud(rng, 3), Y.ryaw(0, 0, 0.35), n=n, m=3)
