"""The yardstick of the object layer's data association: Object_2D::NoParaDataAssociation (reference src/Object.cc:728-962) and
Object_Map::ComputeProjectRectFrame (:1606-1651).

This is a TRANSCRIPTION, not a recording: src/Object.cc needs OpenCV to compile, so its two functions are restated here statement by statement in numpy scalars
of upstream's types -- it really sorts each axis and strides through it, counts in float32 counters incremented by one, forms the int32 products and takes the
square root in double.  The line numbers beside the statements are the reference's.  A second, sort-free and vectorised form of each function stands beside the
literal one (the form the device uses); tests/test_object_association_reference_cpu.py holds the two to each other.

Point lists hold the GOOD points only (not isBad() and not out_point) in vector order; S is mvpMapObjectMappoints.size() with the bad ones."""
import numpy as np

MIN_DET_POINTS = 20     # src/Object.cc:760   (tests/golden/object_association_constants.json holds these to the reference text)
MIN_MAP_POINTS = 20     # :764
SAMPLE_RATIO = 3        # :776
CRITICAL = 1.282        # :942
VARIANCE_DIVISOR = 12   # :942
HALF = 0.5              # :942
UNDEFINED = 3           # not upstream's: its int product m * n * (m + n + 1) overflows
INT32_MAX = 2 ** 31 - 1
RECT_EMPTY, RECT_OK, RECT_UNDEFINED = 0, 1, 2

f32, f64 = np.float32, np.float64


def plan(m, n_good, S):
    """(verdict or None, n, step) before a coordinate is compared; n and step as far as upstream got (step = 0: not declared yet)"""
    if m < MIN_DET_POINTS:
        return 0, n_good, 0
    if n_good < MIN_MAP_POINTS:
        return 2, n_good, 0
    n, step = n_good, 1
    if SAMPLE_RATIO * m > INT32_MAX:
        return UNDEFINED, n, step
    if n_good > SAMPLE_RATIO * m:
        step = S // (SAMPLE_RATIO * m)
        n = len(range(0, n_good, step))
    if m * n * (m + n + 1) > INT32_MAX:
        return UNDEFINED, n, step
    return None, n, step


def decide(m, n, counts):
    """:930-961 over float32 counters; returns (verdict, w (3,) float32, r (2,) float32)"""
    m32, n32 = np.int32(m), np.int32(n)
    tm, tn = np.int32(m32 * (m32 + np.int32(1)) // np.int32(2)), np.int32(n32 * (n32 + np.int32(1)) // np.int32(2))
    w = np.zeros(3, f32)
    for a in range(3):
        w12, w21, w00 = f32(counts[3 * a]), f32(counts[3 * a + 1]), f32(counts[3 * a + 2])
        p, q = f32(w12 + f32(tm)), f32(w21 + f32(tn))
        w[a] = f32(min(p, q) + f32(w00 / f32(2)))
    prod = np.int32(np.int32(m32 * n32) * np.int32(m32 + n32 + np.int32(1)))      # (below INT32_MAX: plan() saw to it)
    root = np.sqrt(f64(int(prod) // VARIANCE_DIVISOR))
    centre = f64(HALF) * f64(m) * f64(m + n + 1)
    r = np.array([f32(centre - f64(CRITICAL) * root), f32(centre + f64(CRITICAL) * root)], f32)
    add = sum(1 for a in range(3) if w[a] > r[0] and w[a] < r[1])
    return (1 if add == 3 else 2), w, r


def result(m, n, step, verdict, counts=None, w=None, r=None):
    return dict(m=int(m), n=int(n), step=int(step), verdict=int(verdict), counts=np.zeros(9, np.uint32) if counts is None else np.asarray(counts, np.uint32),
                w=np.zeros(3, f32) if w is None else w, r=np.zeros(2, f32) if r is None else r)


def np_literal(det, mp, S=None):
    """Object_2D::NoParaDataAssociation as written: sort, stride, float counters, three compares per pair"""
    det, mp = np.asarray(det, f32).reshape(-1, 3), np.asarray(mp, f32).reshape(-1, 3)
    S = len(mp) if S is None else S
    m, n_good = len(det), len(mp)
    v, n, step = plan(m, n_good, S)
    if v is not None:
        return result(m, n, step, v)
    if n_good > SAMPLE_RATIO * m:                                   # :776
        xs, ys, zs = np.sort(mp[:, 0]), np.sort(mp[:, 1]), np.sort(mp[:, 2])      # :798-800, each axis separately
        sample = [[float(xs[i]), float(ys[i]), float(zs[i])] for i in range(0, n_good, step)]      # :802-807
    else:
        sample = [[float(p[0]), float(p[1]), float(p[2])] for p in mp]                             # :812-824
    assert len(sample) == n
    wc = np.zeros(9, f32)                                           # w_x_12 w_x_21 w_x_00 w_y_.. w_z_.. (:830-838)
    one = f32(1)
    for p1 in det:                                                  # :843
        x1 = (float(p1[0]), float(p1[1]), float(p1[2]))             # promoted to double (:850-852)
        for s in sample:                                            # :894
            for a in range(3):
                if x1[a] > s[a]:
                    wc[3 * a] += one
                elif x1[a] < s[a]:
                    wc[3 * a + 1] += one
                elif x1[a] == s[a]:
                    wc[3 * a + 2] += one
    assert (wc < 2 ** 24).all()
    verdict, w, r = decide(m, n, wc)
    return result(m, n, step, verdict, wc.astype(np.uint32), w, r)


def counts_sort_free(det, mp, n, step):
    """per detection value lb = #(map < x) and ub = #(map <= x) over ALL good points; the strided sample holds ceil(lb / step) below x and ceil(ub / step) up to x"""
    c = np.zeros(9, np.int64)
    for a in range(3):
        col = np.sort(mp[:, a])
        lb, ub = np.searchsorted(col, det[:, a], "left"), np.searchsorted(col, det[:, a], "right")
        kl, ku = -(-lb // step), -(-ub // step)
        c[3 * a], c[3 * a + 1], c[3 * a + 2] = kl.sum(), (n - ku).sum(), (ku - kl).sum()
    return c.astype(np.uint32)


def np_sort_free(det, mp, S=None):
    det, mp = np.asarray(det, f32).reshape(-1, 3), np.asarray(mp, f32).reshape(-1, 3)
    S = len(mp) if S is None else S
    v, n, step = plan(len(det), len(mp), S)
    if v is not None:
        return result(len(det), n, step, v)
    c = counts_sort_free(det, mp, n, step)
    verdict, w, r = decide(len(det), n, c)
    return result(len(det), n, step, verdict, c, w, r)


# ---- Object_Map::ComputeProjectRectFrame

def project_literal(points, Tcw, fx, fy, cx, cy):
    """:1612-1629 point by point.  Rcw * X + tcw is a cv::Mat product: accumulated in double and rounded to float once."""
    T = np.asarray(Tcw, f32).reshape(4, 4)
    fx, fy, cx, cy = f32(fx), f32(fy), f32(cx), f32(cy)
    uv = np.zeros((len(points), 2), f32)
    with np.errstate(all="ignore"):
        for j, X in enumerate(np.asarray(points, f32).reshape(-1, 3)):
            Pc = [f32(f64(T[r, 0]) * f64(X[0]) + f64(T[r, 1]) * f64(X[1]) + f64(T[r, 2]) * f64(X[2]) + f64(T[r, 3])) for r in range(3)]
            invzc = f32(f64(1.0) / f64(Pc[2]))      # :1621
            uv[j, 0] = f32(f32(f32(fx * Pc[0]) * invzc) + cx)      # :1623
            uv[j, 1] = f32(f32(f32(fy * Pc[1]) * invzc) + cy)
    return uv


def _to_int(v):
    """float -> int as cv::Rect_<int>(float, ...) converts: truncation; None where it is undefined"""
    if not np.isfinite(v):
        return None
    t = int(v)
    return t if -2 ** 31 <= t <= INT32_MAX else None


def finish_rect(x_min, x_max, y_min, y_max, cols, rows):
    """:1641-1650 -> (status, rect or None)"""
    if x_min < 0:
        x_min = f32(0)
    if y_min < 0:
        y_min = f32(0)
    if x_max > f32(cols):
        x_max = f32(cols)
    if y_max > f32(rows):
        y_max = f32(rows)
    with np.errstate(all="ignore"):
        vals = [_to_int(x_min), _to_int(y_min), _to_int(f32(x_max - x_min)), _to_int(f32(y_max - y_min))]
    if any(v is None for v in vals):
        return RECT_UNDEFINED, None
    return RECT_OK, np.array(vals, np.int32)


def rect_literal(points, Tcw, fx, fy, cx, cy, cols, rows):
    """Object_Map::ComputeProjectRectFrame as written -> (status, rect or None, uv)"""
    uv = project_literal(points, Tcw, fx, fy, cx, cy)
    if len(uv) == 0:                                                # :1631
        return RECT_EMPTY, None, uv
    if np.isnan(uv).any():                                          # std::sort over a NaN (:1634): undefined
        return RECT_UNDEFINED, None, uv
    x_pt, y_pt = np.sort(uv[:, 0]), np.sort(uv[:, 1])               # :1634-1635
    st, rect = finish_rect(x_pt[0], x_pt[-1], y_pt[0], y_pt[-1], cols, rows)
    return st, rect, uv


def project_vectorised(points, Tcw, fx, fy, cx, cy):
    T = np.asarray(Tcw, f32).reshape(4, 4).astype(f64)
    X = np.asarray(points, f32).reshape(-1, 3).astype(f64)
    with np.errstate(all="ignore"):
        Pc = (((T[:3, 0] * X[:, 0:1] + T[:3, 1] * X[:, 1:2]) + T[:3, 2] * X[:, 2:3]) + T[:3, 3]).astype(f32)
        invzc = (f64(1.0) / Pc[:, 2].astype(f64)).astype(f32)
        u = (f32(fx) * Pc[:, 0]) * invzc + f32(cx)
        v = (f32(fy) * Pc[:, 1]) * invzc + f32(cy)
    return np.stack([u, v], 1).astype(f32)


def rect_vectorised(points, Tcw, fx, fy, cx, cy, cols, rows):
    uv = project_vectorised(points, Tcw, fx, fy, cx, cy)
    if len(uv) == 0:
        return RECT_EMPTY, None, uv
    if np.isnan(uv).any():
        return RECT_UNDEFINED, None, uv
    st, rect = finish_rect(uv[:, 0].min(), uv[:, 0].max(), uv[:, 1].min(), uv[:, 1].max(), cols, rows)
    return st, rect, uv
