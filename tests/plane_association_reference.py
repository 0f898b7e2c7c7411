"""The yardstick of the plane association: the reference's loops literally, in numpy float32 / float64 scalars, one operation per line.

  Map::AssociatePlanesByBoundary   reference src/Map.cc:155-215
  Map::PointDistanceFromPlane      src/Map.cc:217-236
  Map::SearchMatchedPlanes         src/Map.cc:245-292
  Frame::ComputePlaneWorldCoeff    src/Frame.cc:373-379
  MapPlane::MapPlane / UpdateBoundary, the transform of the boundary cloud   src/MapPlane.cc:34-37, :150-153

Readings that the reference text does not pin: a cv::Mat product accumulates in double and rounds once to float;
pcl::transformPointCloud with a double matrix computes each coordinate in double, left to right, and rounds once to float; the isometry is
Converter::toSE3Quat's unit quaternion turned back into a rotation matrix (Eigen's formulas), inverted as R^T, -(R^T t).

Model is the handle's bookkeeping (add order, offsets, counts, compaction) as include/eao_fusion.h states it."""
import math

import numpy as np

F = np.float32
DIS_TH = F(0.2)        # mfDisTh = 0.2 into a float member, src/Map.cc:22
ANGLE_TH = F(0.8)      # mfAngleTh = 0.8, src/Map.cc:23
NO_DISTANCE = F(100)   # double res = 100, src/Map.cc:219
CHUNK = 512            # the distance kernel's points per workgroup (sizes either side of it are scenes)
INITIAL_POINTS = 1 << 13


# ------------------------------------------------------------------------------------------------ the transform
def quat_from_matrix(m):
    """Eigen::Quaterniond(Matrix3d) as Converter::toSE3Quat -> g2o::SE3Quat(R, t) runs it; m row-major, python floats (IEEE double)"""
    t = m[0] + m[4] + m[8]
    if t > 0:
        t = math.sqrt(t + 1.0)
        w = 0.5 * t
        t = 0.5 * (1.0 / t)
        x = (m[7] - m[5]) * t
        y = (m[2] - m[6]) * t
        z = (m[3] - m[1]) * t
    elif m[0] >= m[4] and m[0] >= m[8]:
        t = math.sqrt(m[0] - m[4] - m[8] + 1.0)
        x = 0.5 * t
        t = 0.5 * (1.0 / t)
        w = (m[7] - m[5]) * t
        y = (m[3] + m[1]) * t
        z = (m[6] + m[2]) * t
    elif m[4] > m[0] and m[4] >= m[8]:
        t = math.sqrt(m[4] - m[8] - m[0] + 1.0)
        y = 0.5 * t
        t = 0.5 * (1.0 / t)
        w = (m[2] - m[6]) * t
        z = (m[7] + m[5]) * t
        x = (m[1] + m[3]) * t
    else:
        t = math.sqrt(m[8] - m[0] - m[4] + 1.0)
        z = 0.5 * t
        t = 0.5 * (1.0 / t)
        w = (m[3] - m[1]) * t
        x = (m[2] + m[6]) * t
        y = (m[5] + m[7]) * t
    if w < 0:      # SE3Quat's constructor: positive w, then normalised
        x, y, z, w = -x, -y, -z, -w
    inv = 1.0 / math.sqrt(x * x + y * y + z * z + w * w)
    return x * inv, y * inv, z * inv, w * inv


def quat_to_matrix(q):
    """Eigen's toRotationMatrix"""
    x, y, z, w = q
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return [1 - (tyy + tzz), txy - twz, txz + twy,
            txy + twz, 1 - (txx + tzz), tyz - twx,
            txz - twy, tyz + twx, 1 - (txx + tyy)]


def inverse_isometry(Tcw):
    """rows 0..2 of T.inverse().matrix(), 12 python floats; Tcw: 4x4 float32"""
    T = np.asarray(Tcw, np.float32).reshape(4, 4)
    R = [float(T[i, j]) for i in range(3) for j in range(3)]
    t = [float(T[0, 3]), float(T[1, 3]), float(T[2, 3])]
    R = quat_to_matrix(quat_from_matrix(R))
    m = []
    for i in range(3):
        m += [R[0 * 3 + i], R[1 * 3 + i], R[2 * 3 + i]]
        m.append(-(R[0 * 3 + i] * t[0] + R[1 * 3 + i] * t[1] + R[2 * 3 + i] * t[2]))
    return m


def transform_cloud(xyz, Tcw):
    """pcl::transformPointCloud(cloud, out, T.inverse().matrix()), literally; Tcw None: the cloud as it is"""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    if Tcw is None:
        return xyz.copy()
    m = inverse_isometry(Tcw)
    out = np.zeros_like(xyz)
    with np.errstate(all="ignore"):
        for i in range(len(xyz)):
            x, y, z = np.float64(xyz[i, 0]), np.float64(xyz[i, 1]), np.float64(xyz[i, 2])
            for k in range(3):
                s = np.float64(m[4 * k]) * x
                s = s + np.float64(m[4 * k + 1]) * y
                s = s + np.float64(m[4 * k + 2]) * z
                s = s + np.float64(m[4 * k + 3])
                out[i, k] = F(s)
    return out


def transform_cloud_vectorised(xyz, Tcw):
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    if Tcw is None:
        return xyz.copy()
    m = np.array(inverse_isometry(Tcw), np.float64).reshape(3, 4)
    p = xyz.astype(np.float64)
    with np.errstate(all="ignore"):
        out = [((m[k, 0] * p[:, 0] + m[k, 1] * p[:, 1]) + m[k, 2] * p[:, 2]) + m[k, 3] for k in range(3)]
        return np.stack(out, 1).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the query
def world_coefficients(M, c):
    """pM = M^T c, a cv::Mat product: double accumulation, one rounding"""
    M = np.asarray(M, np.float32).reshape(4, 4)
    c = np.asarray(c, np.float32).reshape(4)
    pM = np.zeros(4, np.float32)
    with np.errstate(all="ignore"):
        for k in range(4):
            s = np.float64(0)
            for j in range(4):
                s = s + np.float64(M[j, k]) * np.float64(c[j])
            pM[k] = F(s)
    return pM


def gate(pM, pW, angle_th):
    with np.errstate(all="ignore"):
        angle = F(pM[0]) * F(pW[0])
        angle = angle + F(pM[1]) * F(pW[1])
        angle = angle + F(pM[2]) * F(pW[2])
        return bool(angle > F(angle_th) or angle < -F(angle_th))


def point_distance(pM, cloud):
    """Map::PointDistanceFromPlane"""
    res = NO_DISTANCE
    with np.errstate(all="ignore"):
        for p in cloud:
            d = F(pM[0]) * F(p[0])
            d = d + F(pM[1]) * F(p[1])
            d = d + F(pM[2]) * F(p[2])
            d = d + F(pM[3])
            d = np.abs(d)
            if d < res:
                res = d
    return res


def point_distance_vectorised(pM, cloud):
    cloud = np.asarray(cloud, np.float32).reshape(-1, 3)
    if len(cloud) == 0:
        return NO_DISTANCE
    with np.errstate(all="ignore"):
        d = np.abs(((F(pM[0]) * cloud[:, 0] + F(pM[1]) * cloud[:, 1]) + F(pM[2]) * cloud[:, 2]) + F(pM[3]))
        d = np.where(d < NO_DISTANCE, d, NO_DISTANCE)      # a NaN, an infinity and anything from 100 up never win
    return F(d.min())


def associate(M, set_start, coef, cands, dis_th=DIS_TH, angle_th=ANGLE_TH, vectorised=False):
    """cands: [(world_pos (4,), cloud (n, 3))] in the caller's iteration order.  dict(world_coef, gated, dis, match, match_dis)"""
    M = np.asarray(M, np.float32).reshape(-1, 4, 4)
    coef = np.asarray(coef, np.float32).reshape(-1, 4)
    set_start = [0, len(coef)] if set_start is None else [int(s) for s in set_start]
    rows, nc = len(coef), len(cands)
    out = dict(world_coef=np.zeros((rows, 4), np.float32), gated=np.zeros((rows, nc), np.uint8), dis=np.full((rows, nc), NO_DISTANCE, np.float32),
               match=np.full(rows, -1, np.int32), match_dis=np.zeros(rows, np.float32))
    pd = point_distance_vectorised if vectorised else point_distance
    for s in range(len(M)):
        for i in range(set_start[s], set_start[s + 1]):
            pM = world_coefficients(M[s], coef[i])
            out["world_coef"][i] = pM
            ldTh = F(dis_th)
            for j, (pW, cloud) in enumerate(cands):
                if gate(pM, pW, angle_th):
                    out["gated"][i, j] = 1
                    dis = pd(pM, cloud)
                    out["dis"][i, j] = dis
                    if dis < ldTh:
                        ldTh = dis
                        out["match"][i] = j
            out["match_dis"][i] = ldTh
    return out


# ------------------------------------------------------------------------------------------------ the handle's bookkeeping
class Model:
    """ids in add order, (begin, count) per plane, points in use, dead points, compaction when the dead exceed half"""

    def __init__(self):
        self.compactions = 0
        self.clear()

    def clear(self):
        self.entries = []      # [id, begin, count, world, cloud, live]
        self.used = self.dead = 0

    def _find(self, pid):
        for e in self.entries:
            if e[5] and e[0] == pid:
                return e
        return None

    def add(self, pid, world, xyz, Tcw=None):
        if self._find(pid) is not None:
            raise ValueError("live id")
        cloud = transform_cloud_vectorised(xyz, Tcw)
        self.entries.append([pid, self.used, len(cloud), np.asarray(world, np.float32).reshape(4).copy(), cloud, True])
        self.used += len(cloud)

    def update_boundary(self, pid, xyz, Tcw=None):
        e = self._find(pid)
        if e is None:
            raise ValueError("unknown id")
        cloud = transform_cloud_vectorised(xyz, Tcw)
        self.dead += e[2]
        e[1], e[2], e[4] = self.used, len(cloud), cloud
        self.used += len(cloud)
        self._maybe_compact()

    def set_world_pos(self, pid, world):
        e = self._find(pid)
        if e is None:
            raise ValueError("unknown id")
        e[3] = np.asarray(world, np.float32).reshape(4).copy()

    def erase(self, pid):
        e = self._find(pid)
        if e is None:
            return
        e[5] = False
        self.dead += e[2]
        self._maybe_compact()

    def _maybe_compact(self):
        n_live = sum(e[5] for e in self.entries)
        if self.dead * 2 > self.used or (n_live == 0 and self.entries):
            self.entries = [e for e in self.entries if e[5]]
            at = 0
            for e in self.entries:
                e[1] = at
                at += e[2]
            self.used, self.dead = at, 0
            self.compactions += 1

    def live(self):
        return [e for e in self.entries if e[5]]

    def candidates(self, cand_id=None):
        if cand_id is None:
            return [(e[3], e[4]) for e in self.live()]
        out = []
        for pid in cand_id:
            e = self._find(int(pid))
            if e is None:
                raise ValueError("unknown id")
            out.append((e[3], e[4]))
        return out
