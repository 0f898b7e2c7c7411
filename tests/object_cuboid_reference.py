"""The yardstick of a map object's cuboid: Object_Map::ComputeMeanAndStandard (reference src/Object.cc:999-1235) with Object_Map::UpdateObjPose (:2243-2303),
and the pairwise overlap test (Object_Map::WhetherOverlap, :1954-1970; src/LocalMapping.cc:858-877), in numpy, every float operation rounded on its own.

Two forms, held equal on every scene (tests/test_object_cuboid_reference_cpu.py):
  literal(obj)      upstream's loops in numpy scalars, one operation per line: push_back, sort, the early returns
  device(obj)       what the device runs: extrema instead of sorts (of equal values the one at the smallest list position), whole-list passes; the ordered sums
                    are np.add.accumulate over the list behind a leading +0.0f, which IS the dependent chain.  Vectorised, so that 2^20 points take under a second.
They can differ in one thing only: where -0.0f and +0.0f tie at an extremum, the sort decides which sign is taken.  zero_sign_fields(obj) runs device() under
all four tie rules (first / last position for minima and for maxima), shows that the records differ in the sign of zeros only, and names the fields that do:
same_records(a, b, drop) compares with exactly those zeros' signs dropped.

Readings that OpenCV, Eigen and g2o leave open on a machine without them.  The main reading, and with alt=True the plain alternative:
  mSumPointsPos / n           convertTo with alpha = 1.0 / n: sum * (float)alpha + 0.0f         | IEEE sum / (float)n
  Rcw * Ryaw, Rcw = identity  double accumulation from +0.0, rounded once (-0.0f never survives) | the unrolled float form a0 b0 + a1 b1 + a2 b2 without a start value
  Quaterniond(R)              t = 0.5 / t                                                        | t = 0.5 * (1.0 / t)
  normalizeRotation           coeffs / sqrt(((x x + y y) + z z) + w w)                           | coeffs * (1.0 / norm)
Every scene carries `variant`: whether the alternative gives other bits anywhere in its record."""
import numpy as np

f32, f64 = np.float32, np.float64

FEW_FRAMES = 5
CORNER_MAX_X, CORNER_MAX_Y, CORNER_MAX_Z = 0x66, 0xCC, 0xF0
CORNER_FAR = (2, 8)
EMPTY, DONE = 0, 1

RECORD_DTYPE = np.dtype([("status", np.int32), ("bounds_written", np.int32), ("sum_pos", np.float32, 3), ("center", np.float32, 3), ("standar", np.float32, 3),
                         ("center_standar", np.float32, 3), ("center_standar_dis", np.float32), ("bounds", np.float32, 6),
                         ("lenth", np.float32), ("width", np.float32), ("height", np.float32), ("rmax", np.float32), ("reserved", np.int32),
                         ("Twobj", np.float32, 16), ("Twobj_without_yaw", np.float32, 16), ("cuboid_center", np.float64, 3),
                         ("corners", np.float64, (8, 3)), ("corners_w", np.float64, (8, 3)), ("pose_q", np.float64, 4), ("pose_t", np.float64, 3),
                         ("pose_without_yaw_q", np.float64, 4), ("pose_without_yaw_t", np.float64, 3)])
ROW_DTYPE = np.dtype([("cuboid_center", np.float64, 3), ("lenth", np.float32), ("width", np.float32), ("height", np.float32), ("reserved", np.int32)])
FLOAT_FIELDS = [n for n in RECORD_DTYPE.names if RECORD_DTYPE[n].base.kind == "f"]


def arrays(obj):
    return (np.ascontiguousarray(obj["points"], f32).reshape(-1, 3), np.ascontiguousarray(obj["centroids"], f32).reshape(-1, 3),
            np.ascontiguousarray(obj["Ryaw"], f32).reshape(9), np.ascontiguousarray(obj["prev_cuboid_center"], f64).reshape(3))


def ryaw(rotP, rotR, rotY):
    """upstream's expression (:2250-2260) in float; cos / sin are the caller's"""
    cp, sp, sr, cr, sy, cy = f32(np.cos(f32(rotP))), f32(np.sin(f32(rotP))), f32(np.sin(f32(rotR))), f32(np.cos(f32(rotR))), f32(np.sin(f32(rotY))), f32(np.cos(f32(rotY)))
    return np.array([cp * cy, (sr * sp * cy) - (cr * sy), (cr * sp * cy) + (sr * sy),
                     cp * sy, (sr * sp * sy) + (cr * cy), (cr * sp * sy) - (sr * cy),
                     -sp, sr * cp, cr * cp], f32)


def mat_div(s, n, alt=False):
    if alt:
        return f32(f32(s) / f32(n))
    alpha = f32(f64(1.0) / f64(n))
    return f32(f32(f32(s) * alpha) + f32(0.0))


def quat_branch(m):
    """which branch of Eigen's Quaterniond(Matrix3d) a row-major R takes: -1 (trace > 0), 0, 1, 2"""
    if f64(m[0]) + f64(m[4]) + f64(m[8]) > 0:
        return -1
    i = 0
    if m[4] > m[0]:
        i = 1
    if m[8] > (m[4] if i == 1 else m[0]):
        i = 2
    return i


def quat_from_R(m, alt=False):
    m = [f64(v) for v in m]
    half = (lambda t: f64(0.5) * (f64(1.0) / t)) if alt else (lambda t: f64(0.5) / t)
    t = m[0] + m[4] + m[8]
    if t > 0:
        t = np.sqrt(t + f64(1.0))
        w = f64(0.5) * t
        t = half(t)
        return [(m[7] - m[5]) * t, (m[2] - m[6]) * t, (m[3] - m[1]) * t, w]
    i = quat_branch(m)
    if i == 0:
        t = np.sqrt(m[0] - m[4] - m[8] + f64(1.0))
        x = f64(0.5) * t
        t = half(t)
        return [x, (m[3] + m[1]) * t, (m[6] + m[2]) * t, (m[7] - m[5]) * t]
    if i == 1:
        t = np.sqrt(m[4] - m[8] - m[0] + f64(1.0))
        y = f64(0.5) * t
        t = half(t)
        return [(m[1] + m[3]) * t, y, (m[7] + m[5]) * t, (m[2] - m[6]) * t]
    t = np.sqrt(m[8] - m[0] - m[4] + f64(1.0))
    z = f64(0.5) * t
    t = half(t)
    return [(m[2] + m[6]) * t, (m[5] + m[7]) * t, z, (m[3] - m[1]) * t]


def se3_from_T(T, alt=False, info=None):
    """Converter::toSE3Quat -> g2o::SE3Quat(R, t): (q = x y z w, t), all f64"""
    R = [f64(T[4 * i + j]) for i in range(3) for j in range(3)]
    t = [f64(T[4 * i + 3]) for i in range(3)]
    q = quat_from_R(R, alt)
    if info is not None:
        info.append((quat_branch(R), bool(q[3] < 0)))
    if q[3] < 0:
        q = [v * f64(-1.0) for v in q]
    n2 = ((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]
    n = np.sqrt(n2)
    if alt:
        inv = f64(1.0) / n
        q = [v * inv for v in q]
    else:
        q = [v / n for v in q]
    return q, t


def quat_rotate(q, v):
    """Eigen's Quaterniond * Vector3d; v's components may be f64 scalars or f64 arrays"""
    uv = [q[1] * v[2] - q[2] * v[1], q[2] * v[0] - q[0] * v[2], q[0] * v[1] - q[1] * v[0]]
    uv = [u + u for u in uv]
    c = [q[1] * uv[2] - q[2] * uv[1], q[2] * uv[0] - q[0] * uv[2], q[0] * uv[1] - q[1] * uv[0]]
    return [(v[k] + q[3] * uv[k]) + c[k] for k in range(3)]


def pose_inverse(pose):
    q, t = pose
    qi = [-q[0], -q[1], -q[2], q[3]]
    return qi, quat_rotate(qi, [t[k] * f64(-1.0) for k in range(3)])


def pose_apply(pose, v):
    r = quat_rotate(pose[0], v)
    return [pose[1][k] + r[k] for k in range(3)]


def update_obj_pose(Ryaw, rec, alt=False, info=None):
    T = [f32(1.0) if k % 5 == 0 else f32(0.0) for k in range(16)]
    W = list(T)
    res = [None] * 9
    for i in range(3):
        for j in range(3):
            if alt:
                res[3 * i + j] = f32(f32(f32(T[4 * i] * Ryaw[j]) + f32(T[4 * i + 1] * Ryaw[3 + j])) + f32(T[4 * i + 2] * Ryaw[6 + j]))
            else:
                acc = f64(0.0)
                for k in range(3):
                    acc = acc + f64(T[4 * i + k]) * f64(Ryaw[3 * k + j])
                res[3 * i + j] = f32(acc)
    for i in range(3):
        for j in range(3):
            T[4 * i + j] = res[3 * i + j]
        T[4 * i + 3] = f32(rec["cuboid_center"][i])
    W[3] = f32(rec["center"][0])
    W[7] = f32(rec["cuboid_center"][1])
    W[11] = f32(rec["center"][2])
    pose, pose_wy = se3_from_T(T, alt, info), se3_from_T(W, alt)
    rec["Twobj"], rec["Twobj_without_yaw"] = T, W
    rec["pose_q"], rec["pose_t"], rec["pose_without_yaw_q"], rec["pose_without_yaw_t"] = pose[0], pose[1], pose_wy[0], pose_wy[1]
    return pose, pose_wy


def _corner(ext, c):
    return [f64(ext[(CORNER_MAX_X >> c) & 1]), f64(ext[2 + ((CORNER_MAX_Y >> c) & 1)]), f64(ext[4 + ((CORNER_MAX_Z >> c) & 1)])]


def world_box(ext, rec):
    rec["cuboid_center"] = [f64(f32(f32(ext[2 * a + 1] + ext[2 * a]) / f32(2))) for a in range(3)]
    rec["bounds"] = [f32(v) for v in ext]
    rec["lenth"], rec["width"], rec["height"] = f32(ext[1] - ext[0]), f32(ext[3] - ext[2]), f32(ext[5] - ext[4])
    rec["corners"] = [_corner(ext, c) for c in range(8)]
    rec["corners_w"] = [_corner(ext, c) for c in range(8)]
    rec["bounds_written"] = 1


def object_box(Ryaw, ext, pose, pose_wy, rec, alt=False):
    rec["corners"] = [pose_apply(pose, _corner(ext, c)) for c in range(8)]
    rec["corners_w"] = [pose_apply(pose_wy, _corner(ext, c)) for c in range(8)]
    rec["lenth"], rec["width"], rec["height"] = f32(ext[1] - ext[0]), f32(ext[3] - ext[2]), f32(ext[5] - ext[4])
    a, b = rec["corners"][CORNER_FAR[0] - 1], rec["corners"][CORNER_FAR[1] - 1]
    rec["cuboid_center"] = [(a[k] + b[k]) / f64(2.0) for k in range(3)]
    update_obj_pose(Ryaw, rec, alt)
    rmax = f32(0.0)
    for c in range(8):
        d = [f32(f32(rec["center"][k]) - f32(rec["corners"][c][k])) for k in range(3)]
        tmp = np.sqrt(f32(f32(f32(d[0] * d[0]) + f32(d[1] * d[1])) + f32(d[2] * d[2])))
        rmax = tmp if rmax < tmp else rmax
    rec["rmax"] = rmax


def _new():
    return dict(status=EMPTY, bounds_written=0, sum_pos=[f32(0)] * 3, center=[f32(0)] * 3, standar=[f32(0)] * 3, center_standar=[f32(0)] * 3,
                center_standar_dis=f32(0), bounds=[f32(0)] * 6, lenth=f32(0), width=f32(0), height=f32(0), rmax=f32(0), reserved=0, Twobj=[f32(0)] * 16,
                Twobj_without_yaw=[f32(0)] * 16, cuboid_center=[f64(0)] * 3, corners=[[f64(0)] * 3] * 8, corners_w=[[f64(0)] * 3] * 8, pose_q=[f64(0)] * 4,
                pose_t=[f64(0)] * 3, pose_without_yaw_q=[f64(0)] * 4, pose_without_yaw_t=[f64(0)] * 3)


def pack(rec):
    out = np.zeros(1, RECORD_DTYPE)
    for k in RECORD_DTYPE.names:
        out[k][0] = np.asarray(rec[k], RECORD_DTYPE[k].base).reshape(RECORD_DTYPE[k].shape)
    return out[0]


def literal(obj, alt=False, info=None):
    """upstream's loops; returns one RECORD_DTYPE record"""
    P, Cn, R, prev = arrays(obj)
    n, m = len(P), len(Cn)
    rec = _new()
    with np.errstate(all="ignore"):
        s = [f32(0), f32(0), f32(0)]
        for i in range(n):
            for a in range(3):
                s[a] = f32(s[a] + P[i, a])
        rec["sum_pos"] = s
        center = [mat_div(s[a], n, alt) for a in range(3)]
        rec["center"] = center
        sum2 = [f32(0), f32(0), f32(0)]
        pt = [[], [], []]
        for i in range(n):
            for a in range(3):
                d = f32(P[i, a] - center[a])
                sum2[a] = f32(sum2[a] + f32(d * d))
                pt[a].append(P[i, a])
        rec["standar"] = [np.sqrt(f32(sum2[a] / f32(n))) for a in range(3)]
        if len(pt[0]) == 0:
            return pack(rec)
        rec["status"] = DONE
        sum2c = [f32(0), f32(0), f32(0)]
        for i in range(m):
            for a in range(3):
                d = f32(Cn[i, a] - center[a])
                sum2c[a] = f32(sum2c[a] + f32(d * d))
        rec["center_standar"] = [np.sqrt(f32(sum2c[a] / f32(m))) for a in range(3)]
        rec["cuboid_center"] = [f64(v) for v in prev]
        if m < FEW_FRAMES:
            ext = []
            for a in range(3):
                srt = np.sort(np.array(pt[a], f32))
                ext += [srt[0], srt[-1]]
            world_box(ext, rec)
        pose, pose_wy = update_obj_pose(R, rec, alt, info)
        obj_pt = [[], [], []]
        for i in range(n):
            o = pose_apply(pose_inverse(pose), [f64(P[i, 0]), f64(P[i, 1]), f64(P[i, 2])])
            for a in range(3):
                obj_pt[a].append(f32(o[a]))
        ext = []
        for a in range(3):
            srt = np.sort(np.array(obj_pt[a], f32))
            ext += [srt[0], srt[n - 1]]
        object_box(R, ext, pose, pose_wy, rec, alt)
        dis = f32(0)
        for i in range(m):
            sq = [f32(f32(Cn[i, a] - center[a]) * f32(Cn[i, a] - center[a])) for a in range(3)]
            dis = f32(dis + np.sqrt(f32(f32(sq[0] + sq[1]) + sq[2])))
        rec["center_standar_dis"] = np.sqrt(f32(dis / f32(m)))
    return pack(rec)


def chain(v):
    """acc = 0.0f; for x in v: acc = acc + x -- per column of a float32 array"""
    v = np.asarray(v, f32)
    return np.add.accumulate(np.concatenate([np.zeros((1,) + v.shape[1:], f32), v]), axis=0, dtype=f32)[-1]


def extremum(v, is_max, pick):
    """the value at the first / last list position among the entries equal to the extremum (keeps the sign of a zero)"""
    best = v.max() if is_max else v.min()
    at = np.flatnonzero(v == best)
    return v[at[0] if pick == "first" else at[-1]]


def extrema(A, picks):
    return [extremum(A[:, a], k == 1, picks[k]) for a in range(3) for k in range(2)]


def device(obj, alt=False, picks=("first", "first")):
    """the device's form, vectorised; returns one RECORD_DTYPE record"""
    P, Cn, R, prev = arrays(obj)
    n, m = len(P), len(Cn)
    rec = _new()
    with np.errstate(all="ignore"):
        s = chain(P)
        rec["sum_pos"] = list(s)
        center = np.array([mat_div(s[a], n, alt) for a in range(3)], f32)
        rec["center"] = list(center)
        if n == 0:
            rec["standar"] = [np.sqrt(f32(f32(0) / f32(0)))] * 3
            return pack(rec)
        d = P - center
        rec["standar"] = list(np.sqrt(chain(d * d) / f32(n)))
        rec["status"] = DONE
        dc = Cn - center
        sq = dc * dc
        rec["center_standar"] = list(np.sqrt(chain(sq) / f32(m)))
        dis = np.sqrt((sq[:, 0] + sq[:, 1]) + sq[:, 2])
        rec["center_standar_dis"] = np.sqrt(chain(dis) / f32(m))
        rec["cuboid_center"] = [f64(v) for v in prev]
        if m < FEW_FRAMES:
            world_box(extrema(P, picks), rec)
        pose, pose_wy = update_obj_pose(R, rec, alt)
        inv = pose_inverse(pose)
        Pd = P.astype(f64)
        o = pose_apply(inv, [Pd[:, 0], Pd[:, 1], Pd[:, 2]])
        O = np.stack([c.astype(f32) for c in o], axis=1)
        object_box(R, extrema(O, picks), pose, pose_wy, rec, alt)
    return pack(rec)


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32 if x.dtype == np.float32 else np.uint64)


def _drop_zero_signs(x):
    x = np.array(x, copy=True)
    x[x == 0] = 0
    return x


def same_field(x, y, drop=False):
    x, y = np.atleast_1d(np.asarray(x)), np.atleast_1d(np.asarray(y))
    if x.dtype.kind != "f":
        return bool(np.array_equal(x, y))
    if drop:
        x, y = _drop_zero_signs(x), _drop_zero_signs(y)
    nan = np.isnan(x)
    return bool(np.array_equal(nan, np.isnan(y)) and np.array_equal(_bits(x)[nan == 0], _bits(y)[nan == 0]))


def differing_fields(a, b):
    """field by field: integers as they are, floats as bit patterns, a NaN by isnan (its sign and payload are nobody's contract)"""
    return [k for k in RECORD_DTYPE.names if not same_field(a[k], b[k])]


def same_records(a, b, drop=()):
    return all(same_field(a[k], b[k], k in drop) for k in RECORD_DTYPE.names)


def zero_sign_fields(obj):
    """the fields that change between the tie rules; asserts that they change in the sign of zeros only"""
    base, names = device(obj), set()
    for picks in (("first", "last"), ("last", "first"), ("last", "last")):
        other = device(obj, picks=picks)
        diff = differing_fields(base, other)
        assert same_records(base, other, drop=diff), "a tie between equal extrema changed more than the sign of a zero"
        names |= set(diff)
    return sorted(names)


def variant(obj):
    return len(differing_fields(device(obj), device(obj, alt=True))) > 0


# ---- the overlap matrix
def overlap_pair(a, b):
    """(verdict, extents) of WhetherOverlap(a, b) in numpy scalars"""
    dis = [f32(np.abs(f64(a["cuboid_center"][k]) - f64(b["cuboid_center"][k]))) for k in range(3)]
    half = [f32(f32(f32(a[k]) / f32(2)) + f32(f32(b[k]) / f32(2))) for k in ("lenth", "width", "height")]
    return bool(dis[0] < half[0] and dis[1] < half[1] and dis[2] < half[2]), [f32(half[k] - dis[k]) for k in range(3)]


def overlaps_literal(rows, eligible):
    m = len(rows)
    verdict, extents = np.zeros((m, m), np.uint8), np.zeros((m, m, 3), f32)
    for i in range(m):
        for j in range(m):
            v, e = overlap_pair(rows[i], rows[j])
            if i != j and eligible[i] and eligible[j] and v:
                verdict[i, j], extents[i, j] = 1, e
    return verdict, extents


def overlaps_vectorised(rows, eligible):
    """the same, whole-matrix operations; extents are zero where the verdict is 0"""
    c = rows["cuboid_center"]
    dis = np.abs(c[:, None, :] - c[None, :, :]).astype(f32)
    s = np.stack([rows["lenth"], rows["width"], rows["height"]], axis=1) / f32(2)
    half = s[:, None, :] + s[None, :, :]
    el = np.asarray(eligible) != 0
    verdict = (dis < half).all(axis=2) & el[:, None] & el[None, :] & ~np.eye(len(rows), dtype=bool)
    return verdict.astype(np.uint8), np.where(verdict[:, :, None], half - dis, f32(0)).astype(f32)


def make_rows(centers, scales):
    rows = np.zeros(len(centers), ROW_DTYPE)
    rows["cuboid_center"] = np.asarray(centers, f64).reshape(-1, 3)
    s = np.asarray(scales, f32).reshape(-1, 3)
    rows["lenth"], rows["width"], rows["height"] = s[:, 0], s[:, 1], s[:, 2]
    return rows


# ---- tools/object_cuboid_walk.cpp's script and output
def _h32(v):
    return "%08x" % np.float32(v).view(np.uint32)


def _h64(v):
    return "%016x" % np.float64(v).view(np.uint64)


def walk_script(obj, verb="object"):
    P, Cn, R, prev = arrays(obj)
    return "%s %d %d %s %s %s %s\n" % (verb, len(P), len(Cn), " ".join(_h32(v) for v in R), " ".join(_h64(v) for v in prev),
                                       " ".join(_h32(v) for v in P.reshape(-1)), " ".join(_h32(v) for v in Cn.reshape(-1)))


def walk_line(rec, drop=()):
    """a record as the program prints it (a NaN as `nan`), the zeros of the fields in `drop` without their signs"""
    out = ["rec", str(int(rec["status"])), str(int(rec["bounds_written"]))]
    for k in FLOAT_FIELDS:
        v = np.atleast_1d(rec[k]).reshape(-1)
        if k in drop:
            v = _drop_zero_signs(v)
        out += ["nan" if np.isnan(x) else (_h32(x) if v.dtype == np.float32 else _h64(x)) for x in v]
    return " ".join(out)


def drop_line(line, drop):
    """the same dropping applied to a printed line"""
    t = line.split()
    at = 3
    for k in FLOAT_FIELDS:
        cnt = int(np.prod(RECORD_DTYPE[k].shape, dtype=np.int64))
        if k in drop:
            for c in range(at, at + cnt):
                if t[c] in ("80000000", "8000000000000000"):
                    t[c] = "0" * len(t[c])
        at += cnt
    return " ".join(t)


def overlap_script(rows, eligible):
    return "overlaps %d %s\n" % (len(rows), " ".join("%s %s %s %s %s %s %d" % (_h64(r["cuboid_center"][0]), _h64(r["cuboid_center"][1]), _h64(r["cuboid_center"][2]),
                                                                                _h32(r["lenth"]), _h32(r["width"]), _h32(r["height"]), int(e))
                                                       for r, e in zip(rows, eligible)))


def overlap_lines(verdict, extents):
    m = len(verdict)
    out = ["ov " + "".join(str(int(v)) for v in verdict.reshape(-1))]
    for i in range(m):
        for j in range(m):
            if verdict[i, j]:
                out.append("ex %d %d %s" % (i, j, " ".join(_h32(v) for v in extents[i, j])))
    return out


# ---- tests/cpp/object_cuboid/object_cuboid_driver.cpp's script and output
def ryaw_libm(rotP, rotR, rotY):
    """upstream's expression with the C library's cosf / sinf, which is what std::cos(float) / std::sin(float) of the adapter's caller resolve to"""
    import ctypes
    libm = ctypes.CDLL("libm.so.6")
    for fn in (libm.cosf, libm.sinf):
        fn.restype, fn.argtypes = ctypes.c_float, [ctypes.c_float]
    cp, sp, sr, cr, sy, cy = (f32(fn(float(f32(a)))) for fn, a in ((libm.cosf, rotP), (libm.sinf, rotP), (libm.sinf, rotR), (libm.cosf, rotR), (libm.sinf, rotY),
                                                                   (libm.cosf, rotY)))
    return np.array([cp * cy, (sr * sp * cy) - (cr * sy), (cr * sp * cy) + (sr * sy),
                     cp * sy, (sr * sp * sy) + (cr * cy), (cr * sp * sy) - (sr * cy),
                     -sp, sr * cp, cr * cp], f32)


def driver_object(points, centroids, rot=(0.0, 0.0, 0.0), prev=(0.0, 0.0, 0.0), cls=0, bad=None):
    """an object as the driver reads it; rot = (rotP, rotR, rotY); bad: per point, isBad()"""
    P, Cn = np.ascontiguousarray(points, f32).reshape(-1, 3), np.ascontiguousarray(centroids, f32).reshape(-1, 3)
    bad = np.zeros(len(P), np.uint8) if bad is None else np.asarray(bad)
    return "%d %s %s %d %s %d %s" % (cls, " ".join(_h32(v) for v in rot), " ".join(_h64(v) for v in prev), len(P),
                                     " ".join("%d %s %s %s" % (b, _h32(p[0]), _h32(p[1]), _h32(p[2])) for b, p in zip(bad, P)), len(Cn),
                                     " ".join(_h32(v) for v in Cn.reshape(-1)))


SENTINEL32, SENTINEL64 = "44424000", "4088480000000000"      # 777, what every member of the driver's stand-in object starts as
MEMBER_FLOATS = ["sum_pos", "center", "standar", "center_standar", "center_standar_dis", "bounds", "lenth", "width", "height", "rmax", "Twobj", "Twobj_without_yaw"]
MEMBER_DOUBLES = ["cuboid_center", "corners", "corners_w"]


def members_line(rec, prev=None):
    """the driver's `members` line for an object whose members the adapter wrote from `rec`: on EMPTY nothing past the deviations, the bounds only when
    bounds_written; everything else keeps the sentinel (cuboidCenter: what the script set, `prev`)"""
    out = ["members"]
    empty = int(rec["status"]) == EMPTY
    for k in MEMBER_FLOATS + MEMBER_DOUBLES:
        v = np.atleast_1d(rec[k]).reshape(-1)
        h, sentinel = (_h32, SENTINEL32) if v.dtype == np.float32 else (_h64, SENTINEL64)
        written = k in ("sum_pos", "center", "standar") or (not empty and (k != "bounds" or int(rec["bounds_written"])))
        if written:
            out += ["nan" if np.isnan(x) else h(x) for x in v]
        elif k == "cuboid_center" and prev is not None:
            out += [_h64(x) for x in prev]
        else:
            out += [sentinel] * len(v)
    return " ".join(out)
