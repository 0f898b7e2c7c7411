"""The yardstick of the object layer's point-list update (csrc/object_points.hip): the change gate, the append and the erase of Object_Map::DataAssociateUpdate
(reference src/Object.cc:1364-1436, :1460-1535, :1538-1589), the append of MergeTwoMapObjs (:1766-1821), the erases of BigToSmall (:2070-2087) and
DivideEquallyTwoObjs (:2096-2120), in numpy scalars, twice:

    literal(desc)   upstream's form: the list grows while the candidates walk it, the compare stops at the first equal entry (`break`), the erase runs while
                    iterating, the extrema are the ends of sorted vectors
    device(desc)    the device's form: first[j] = the first equal position among (list entries, earlier candidates) for all j at once, the new candidates by
                    a prefix sum, the extrema as min / max, the erase as a mask

tests/test_object_points_reference_cpu.py holds the two equal on every scene.  The arithmetic the project already has is imported, not written again: the
projection and the rectangle (object_association_reference), contains and the overlap ratios (frame_objects_reference), the pose (object_cuboid_reference).

Three readings OpenCV leaves open where no OpenCV is at hand are stated here and carried as `variant(desc)` (whether the other reading gives another result):
Rcw * X + tcw accumulates in double and rounds once (alt: float, operation by operation); Point2f -> Point inside contains() is cvRound (alt: truncation);
cv::Rect(float, ...) truncates (alt: rounds)."""
import numpy as np

import frame_objects_reference as FO
import object_association_reference as OA
import object_cuboid_reference as OC

f32, f64 = np.float32, np.float64

# the literals (tests/golden/object_points_constants.json holds them to the reference text)
TH_MANY_FRAMES = 0.9     # src/Object.cc:1470
MANY_FRAMES = 5          # :1469
KEEP_COUNT = 8           # :1555
EDGE_PIXELS = 25         # :1538-1541
CUBOID_SLACK = 1.1       # :1772-1774
MIN_IOU = 0.5            # :1434
MIN_IOU_FORMER = 0.8     # :1434

DONE, REJECTED, UNDEFINED = 1, 2, 3
GATE_NONE, GATE_RADIUS, GATE_CUBOID = 0, 1, 2
ERASE_NONE, ERASE_PROJECTION, ERASE_BOX, ERASE_SHRUNK = 0, 1, 2, 3

RECORD_DTYPE = np.dtype([("status", np.int32), ("n_gated", np.int32), ("n_appended", np.int32), ("n_list", np.int32), ("n_erased", np.int32), ("n_survivors", np.int32),
                         ("rect2", np.int32, 4), ("iou", np.float32), ("iou2", np.float32), ("sum_pos_appended", np.float32, 3), ("sum_pos", np.float32, 3),
                         ("reserved", np.int32, 2)])

INTS = ["change_gate", "gate", "erase", "box_off_edge", "cols", "rows", "n_frames_after_push"]
FLOATS = ["fx", "fy", "cx", "cy", "rmax", "lenth", "width", "height"]
VECTORS = [("Tcw", 16, f32), ("project_rect1", 4, np.int32), ("box_rect", 4, np.int32), ("center", 3, f32), ("pose_q", 4, f64), ("pose_t", 3, f64),
           ("cuboid_center", 3, f64), ("bounds", 6, f32), ("overlap", 3, f32), ("sum_pos", 3, f32)]
DEFAULTS = {"Tcw": np.eye(4, dtype=f32).reshape(16), "pose_q": np.array([0.0, 0.0, 0.0, 1.0])}


def full(desc):
    """every field of a desc, typed; what is missing is zero (Tcw the identity, pose_q the unit quaternion)"""
    d = {}
    for k in INTS:
        d[k] = int(desc.get(k, 0))
    for k in FLOATS:
        d[k] = f32(desc.get(k, 0.0))
    for k, n, dt in VECTORS:
        d[k] = np.asarray(desc.get(k, DEFAULTS.get(k, np.zeros(n))), dt).reshape(n).copy()
    d["map_points"] = np.ascontiguousarray(desc["map_points"], f32).reshape(-1, 3)
    d["cand_points"] = np.ascontiguousarray(desc["cand_points"], f32).reshape(-1, 3)
    mc, cc = desc.get("map_count"), desc.get("cand_count")
    d["map_count"] = np.zeros(len(d["map_points"]), np.int32) if mc is None else np.ascontiguousarray(mc, np.int32).reshape(-1)
    d["cand_count"] = np.zeros(len(d["cand_points"]), np.int32) if cc is None else np.ascontiguousarray(cc, np.int32).reshape(-1)
    assert len(d["map_count"]) == len(d["map_points"]) and len(d["cand_count"]) == len(d["cand_points"])
    return d


# ---- the scalar rules

def project(points, d, alt=False):
    """(n, 2) float32: u, v of :1382-1389"""
    if not alt:
        return OA.project_literal(points, d["Tcw"], d["fx"], d["fy"], d["cx"], d["cy"])
    T = d["Tcw"].reshape(4, 4)
    uv = np.zeros((len(points), 2), f32)
    with np.errstate(all="ignore"):
        for j, X in enumerate(np.asarray(points, f32).reshape(-1, 3)):
            Pc = [f32(f32(f32(f32(T[r, 0] * X[0]) + f32(T[r, 1] * X[1])) + f32(T[r, 2] * X[2])) + T[r, 3]) for r in range(3)]
            invzc = f32(f64(1.0) / f64(Pc[2]))
            uv[j, 0] = f32(f32(f32(d["fx"] * Pc[0]) * invzc) + d["cx"])
            uv[j, 1] = f32(f32(f32(d["fy"] * Pc[1]) * invzc) + d["cy"])
    return uv


def radius_th(n_frames_after_push):
    th = f32(1.0)
    if n_frames_after_push > MANY_FRAMES:
        th = f32(TH_MANY_FRAMES)
    return th


def radius_gate(d, p):
    """:1465-1473: whether the candidate stays"""
    with np.errstate(all="ignore"):
        d0, d1, d2 = f32(d["center"][0] - p[0]), f32(d["center"][1] - p[1]), f32(d["center"][2] - p[2])
        fDis = f32(np.sqrt(f32(f32(f32(d0 * d0) + f32(d1 * d1)) + f32(d2 * d2))))
        return not (fDis > f32(radius_th(d["n_frames_after_push"]) * d["rmax"]))


def cuboid_gate(d, p):
    """:1771-1777"""
    pose = ([f64(v) for v in d["pose_q"]], [f64(v) for v in d["pose_t"]])
    s = OC.pose_apply(OC.pose_inverse(pose), [f64(p[0]), f64(p[1]), f64(p[2])])
    return not ((abs(s[0]) > f64(CUBOID_SLACK) * f64(d["lenth"]) / f64(2)) or (abs(s[1]) > f64(CUBOID_SLACK) * f64(d["width"]) / f64(2)) or
                (abs(s[2]) > f64(CUBOID_SLACK) * f64(d["height"]) / f64(2)))


def gate_of(d, p):
    return radius_gate(d, p) if d["gate"] == GATE_RADIUS else cuboid_gate(d, p)


def finish_rect(x_min, x_max, y_min, y_max, cols, rows, alt=False):
    """:1419-1429 -> rect or None where a conversion is undefined"""
    if not alt:
        st, rect = OA.finish_rect(x_min, x_max, y_min, y_max, cols, rows)
        return rect if st == OA.RECT_OK else None
    x_min, y_min = (f32(0) if x_min < 0 else x_min), (f32(0) if y_min < 0 else y_min)
    x_max, y_max = (f32(cols) if x_max > f32(cols) else x_max), (f32(rows) if y_max > f32(rows) else y_max)
    with np.errstate(all="ignore"):
        vals = [x_min, y_min, f32(x_max - x_min), f32(y_max - y_min)]
    if not all(np.isfinite(v) and abs(v) < 2.0 ** 31 for v in vals):
        return None
    return np.array([int(np.rint(v)) for v in vals], np.int32)


def change_gate(d, rec, sort, alt=False):
    """stage 1 into rec: status, rect2, iou, iou2"""
    uv = project(np.concatenate([d["cand_points"], d["map_points"]]), d, alt)
    rec["status"] = UNDEFINED
    if len(uv) == 0 or np.isnan(uv).any():
        return
    if sort:
        x_pt, y_pt = np.sort(uv[:, 0]), np.sort(uv[:, 1])
        ext = x_pt[0], x_pt[-1], y_pt[0], y_pt[-1]
    else:
        ext = uv[:, 0].min(), uv[:, 0].max(), uv[:, 1].min(), uv[:, 1].max()
    rect2 = finish_rect(*ext, d["cols"], d["rows"], alt)
    if rect2 is None:
        return
    rec["rect2"] = rect2
    with np.errstate(all="ignore"):
        rec["iou"] = FO.ratio(d["project_rect1"], rect2)
        rec["iou2"] = FO.ratio_former(rect2, d["box_rect"])
    rejected = (f64(rec["iou"]) < f64(MIN_IOU)) and (f64(rec["iou2"]) < f64(MIN_IOU_FORMER))
    rec["status"] = REJECTED if rejected else DONE
    if rejected:
        rec["sum_pos_appended"] = rec["sum_pos"] = d["sum_pos"]


def contains(box, u, v, alt=False):
    if not alt:
        return FO.contains(box, u, v)
    x, y = int(u), int(v)
    return int(box[0]) <= x < int(box[0]) + int(box[2]) and int(box[1]) <= y < int(box[1]) + int(box[3])


def erase_entry(d, x, count, alt=False):
    if d["erase"] == ERASE_PROJECTION:
        if not d["box_off_edge"] or count > KEEP_COUNT:
            return False
        u, v = project(x.reshape(1, 3), d, alt)[0]
        if (u > 0 and u < f32(d["cols"])) and (v > 0 and v < f32(d["rows"])):
            return not contains(d["box_rect"], u, v, alt)
        return False
    if d["erase"] == ERASE_BOX:
        b = d["bounds"]
        return bool(x[0] > b[0] and x[0] < b[1] and x[1] > b[2] and x[1] < b[3] and x[2] > b[4] and x[2] < b[5])
    if d["erase"] == ERASE_SHRUNK:
        ext = (d["lenth"], d["width"], d["height"])
        for a in range(3):
            half = f32(f32(ext[a] / f32(2)) - f32(d["overlap"][a] / f32(2)))
            if not (f64(x[a]) > d["cuboid_center"][a] - f64(half) and f64(x[a]) < d["cuboid_center"][a] + f64(half)):
                return False
        return True
    return False


def _result(rec, gate, target, count, lst, erased, surv, pts):
    return dict(rec=rec, gate=np.array(gate, np.uint8), target=np.array(target, np.int32), count=np.array(count, np.int32),
                list=np.array(lst, np.int32).reshape(-1, 2), erased=np.array(erased, np.uint8), survivors=np.array(surv, np.int32).reshape(-1, 2),
                points=np.array(pts, f32).reshape(-1, 3))


# ---- upstream's form

def literal(desc, alt=False):
    d = full(desc)
    rec = np.zeros((), RECORD_DTYPE)
    if d["change_gate"]:
        change_gate(d, rec, sort=True, alt=alt)
        if rec["status"] != DONE:
            return dict(rec=rec)
    rec["status"] = DONE
    mp, cp = d["map_points"], d["cand_points"]
    lst = [(0, m, int(d["map_count"][m]), mp[m]) for m in range(len(mp))]      # (source, index, count, position)
    keys = [tuple(float(v) for v in e[3]) for e in lst]                        # the positions as Python floats: == is IEEE's
    s = d["sum_pos"].copy()
    gate, target, count = [0] * len(cp), [-1] * len(cp), [int(c) for c in d["cand_count"]]
    for j in range(len(cp) if d["gate"] != GATE_NONE else 0):
        p = cp[j]
        if not gate_of(d, p):
            continue
        gate[j] = 1
        count[j] += 1
        rec["n_gated"] += 1
        key = tuple(float(v) for v in p)
        new_point = True
        for m in range(len(keys)):
            if keys[m][0] == key[0] and keys[m][1] == key[1] and keys[m][2] == key[2]:
                target[j] = m
                new_point = False
                break
        if new_point:
            lst.append((1, j, count[j], p))
            keys.append(key)
            rec["n_appended"] += 1
            with np.errstate(all="ignore"):
                s = (s + p).astype(f32)
    rec["sum_pos_appended"] = s
    rec["n_list"] = len(lst)
    pairs = [(e[0], e[1]) for e in lst]
    erased = [0] * len(lst)
    at, k = 0, 0
    while at < len(lst):      # the erase while iterating
        if erase_entry(d, lst[at][3], lst[at][2], alt):
            if d["erase"] == ERASE_PROJECTION:
                with np.errstate(all="ignore"):
                    s = (s - lst[at][3]).astype(f32)
            erased[k] = 1
            del lst[at]
        else:
            at += 1
        k += 1
    rec["n_erased"] = sum(erased)
    rec["n_survivors"] = len(lst)
    rec["sum_pos"] = s
    return _result(rec, gate, target, count, pairs, erased, [(e[0], e[1]) for e in lst], [e[3] for e in lst])


# ---- the device's form

def chain(start, terms, sign):
    """start (+ or -) the terms' rows in order, float by float"""
    s = np.asarray(start, f32).copy()
    with np.errstate(all="ignore"):
        for t in terms:
            s = (s + t).astype(f32) if sign > 0 else (s - t).astype(f32)
    return s


def first_equal(mp, cp, gate):
    """first[j]: the smallest position of (list entries, candidates before j) that equals candidate j; None where there is none; -2 where j is gated out"""
    both = np.concatenate([mp, cp])
    first = []
    for j in range(len(cp)):
        if not gate[j]:
            first.append(-2)
            continue
        hit = np.flatnonzero((both[:len(mp) + j] == cp[j]).all(axis=1))
        first.append(int(hit[0]) if len(hit) else None)
    return first


def device(desc):
    d = full(desc)
    rec = np.zeros((), RECORD_DTYPE)
    if d["change_gate"]:
        change_gate(d, rec, sort=False)
        if rec["status"] != DONE:
            return dict(rec=rec)
    rec["status"] = DONE
    mp, cp = d["map_points"], d["cand_points"]
    M, C = len(mp), len(cp)
    gate = [1 if d["gate"] != GATE_NONE and gate_of(d, cp[j]) else 0 for j in range(C)]
    first = first_equal(mp, cp, gate)
    is_new = np.array([f is None for f in first], np.int64)
    rank = np.cumsum(is_new) - is_new      # the exclusive prefix sum
    app = [j for j in range(C) if is_new[j]]
    target = [-1 if f is None or f == -2 else (f if f < M else M + int(rank[f - M])) for f in first]
    for f in first:
        assert f is None or f == -2 or f < M or is_new[f - M], "the first equal candidate is itself new"
    count = [int(d["cand_count"][j]) + gate[j] for j in range(C)]
    pairs = [(0, m) for m in range(M)] + [(1, j) for j in app]
    pos = [mp[m] for m in range(M)] + [cp[j] for j in app]
    cnt = [int(c) for c in d["map_count"]] + [count[j] for j in app]
    s = chain(d["sum_pos"], [cp[j] for j in app], +1)
    rec["n_gated"], rec["n_appended"], rec["n_list"] = sum(gate), len(app), len(pairs)
    rec["sum_pos_appended"] = s
    erased = [1 if erase_entry(d, pos[k], cnt[k]) else 0 for k in range(len(pairs))]
    if d["erase"] == ERASE_PROJECTION:
        s = chain(s, [pos[k] if erased[k] else np.zeros(3, f32) for k in range(len(pairs))], -1)      # a kept entry subtracts a zero
    rec["sum_pos"] = s
    keep = [k for k in range(len(pairs)) if not erased[k]]
    rec["n_erased"], rec["n_survivors"] = sum(erased), len(keep)
    return _result(rec, gate, target, count, pairs, erased, [pairs[k] for k in keep], [pos[k] for k in keep])


# ---- comparing

def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32 if x.dtype == f32 else np.uint64)


def same_float(a, b):
    """bit for bit, a NaN as a NaN (its sign and payload are nobody's contract)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(_bits(a)[~na], _bits(b)[~nb]))


def same_record(a, b):
    for k in RECORD_DTYPE.names:
        if RECORD_DTYPE[k].base.kind == "f":
            if not same_float(a[k], b[k]):
                return False
        elif not np.array_equal(a[k], b[k]):
            return False
    return True


def differences(a, b):
    """the names of the outputs in which two results differ"""
    bad = [] if same_record(a["rec"], b["rec"]) else ["rec"]
    if set(a) != set(b):
        return bad + ["keys"]
    for k in a:
        if k == "rec":
            continue
        ok = same_float(a[k], b[k]) if k == "points" else (np.asarray(a[k]).shape == np.asarray(b[k]).shape and np.array_equal(a[k], b[k]))
        if not ok:
            bad.append(k)
    return bad


def variant(desc):
    """whether the alternative readings give another result"""
    return bool(differences(literal(desc), literal(desc, alt=True)))


# ---- tools/object_points_walk.cpp: its script and the line it prints

def _h32(v):
    return " ".join("%08x" % b for b in _bits(np.asarray(v, f32).reshape(-1)))


def _h64(v):
    return " ".join("%016x" % b for b in _bits(np.asarray(v, f64).reshape(-1)))


def _ints(v):
    return " ".join(str(int(x)) for x in np.asarray(v).reshape(-1))


def walk_script(desc, verb="update"):
    d = full(desc)
    parts = [verb, _ints([d[k] for k in INTS]), str(len(d["map_points"])), str(len(d["cand_points"])), _h32([d[k] for k in FLOATS])]
    for k, _, dt in VECTORS:
        parts.append(_ints(d[k]) if dt == np.int32 else _h32(d[k]) if dt == f32 else _h64(d[k]))
    parts += [_h32(d["map_points"]), _ints(d["map_count"]), _h32(d["cand_points"]), _ints(d["cand_count"])]
    return " ".join(p for p in parts if p) + "\n"


def _pf(v):
    return " ".join("nan" if np.isnan(x) else "%08x" % b for x, b in zip(np.asarray(v, f32).reshape(-1), _bits(np.asarray(v, f32).reshape(-1))))


def walk_line(res):
    r = res["rec"]
    parts = ["rec", _ints([r[k] for k in ("status", "n_gated", "n_appended", "n_list", "n_erased", "n_survivors")]), _ints(r["rect2"]), _pf([r["iou"], r["iou2"]]),
             _pf(r["sum_pos_appended"]), _pf(r["sum_pos"])]
    if int(r["status"]) == DONE:
        for k in ("gate", "target", "count", "list", "erased", "survivors"):
            parts += ["|", _ints(res[k])]
        parts += ["|", _pf(res["points"])]
    return " ".join(p for p in parts if p)
