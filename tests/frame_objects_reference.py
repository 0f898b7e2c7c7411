"""The yardstick of a frame's 2D objects: steps 2, 4, 5 and 6 of the object layer (reference src/Tracking.cc:1768-1973; Tracking::AssociateObjAndPoints
:3031-3065; Object_2D::ComputeMeanAndStandardFrame and RemoveOutliersByBoxPlot, src/Object.cc:61-157; Converter::bboxOverlapratio*, src/Converter.cc:194-212) in
numpy scalars, every float operation rounded on its own.

Two forms, held equal on every scene (tests/test_frame_objects_reference_cpu.py):
  literal(frame)    upstream's loops: push_back, sort, erase
  compact(frame)    what the device runs: ordered compactions, Q1 / Q3 from counting ranks (of tied candidates the one with the smallest list position), the
                    feature coordinates through same-id links, min / max for the feature box
They can differ in one thing only: where -0.0f and +0.0f tie at a quartile, the sort decides the sign of Q1 / Q3 (and so of a zero IQR or max_th) and the rank
count takes the earlier list entry; no `z > max_th` verdict depends on it (zero_sign_invariant below).  same() compares with those three zeros' signs dropped.

cv::Mat conventions: products accumulate in double and round once; `sum_pos_3d / n` is convertTo with alpha = 1.0 / n, i.e.
sum * (float)alpha + 0.0f.  OpenCV is not at hand to pin that reading, so every box also carries `variant`: whether plain IEEE sum / (float)n gives other bits."""
import numpy as np

f32, f64 = np.float32, np.float64

BOXPLOT_MIN_POINTS, QUARTILE_DIVISOR, IQR_FACTOR, FEATURE_RECT_MIN_POINTS = 8, 4, 1.5, 4
CROWD_RATIO, CROWD_MAX, LARGE_AREA_RATIO, FEW_POINTS, FEW_POINTS_ON_EDGE, FEW_POINTS_EDGE_PIXELS, ON_EDGE_PIXELS = 0.05, 4, 0.5, 5, 10, 20, 5
SAME_OBJECT_IOU, SURROUND_IOU, SURROUND_RATIO = 0.3, 0.05, 0.85
MAX_KEYPOINTS, MAX_BOXES = 4096, 256

RECORD_DTYPE = np.dtype([("n_assigned", np.int32), ("n", np.int32), ("sum_pos", np.float32, 3), ("pos", np.float32, 3), ("std", np.float32, 3),
                         ("q1", np.float32), ("q3", np.float32), ("max_th", np.float32), ("boxplot_ran", np.int32), ("center_2d", np.float32, 2),
                         ("has_feature_rect", np.int32), ("feature_rect", np.int32, 4), ("num_overlaps", np.int32), ("bad", np.int32), ("on_edge", np.int32)])


def _arrays(fr):
    return (np.asarray(fr["kp_x"], f32).reshape(-1), np.asarray(fr["kp_y"], f32).reshape(-1), np.asarray(fr["mp_id"], np.int32).reshape(-1),
            np.asarray(fr["mp_xyz"], f32).reshape(-1, 3), np.asarray(fr["boxes"], np.int32).reshape(-1, 4), np.asarray(fr["score"], f32).reshape(-1),
            np.asarray(fr["Tcw"], f32).reshape(4, 4))


def cv_round(v):
    """saturate_cast<int>(float) = cvRound: nearest, ties to even"""
    return int(np.rint(f32(v)))


def contains(box, px, py):
    """cv::Rect_<int>::contains(Point_<int>(pt)) (:3046)"""
    x, y = cv_round(px), cv_round(py)
    return int(box[0]) <= x < int(box[0]) + int(box[2]) and int(box[1]) <= y < int(box[1]) + int(box[3])


def camera_row(T, r, X):
    acc = f64(T[r, 0]) * f64(X[0]) + f64(T[r, 1]) * f64(X[1]) + f64(T[r, 2]) * f64(X[2])
    return f32(acc + f64(T[r, 3]))


def mat_div(s, n):
    alpha = f32(f64(1.0) / f64(n))
    return f32(f32(f32(s) * alpha) + f32(0.0))


def plain_div(s, n):
    return f32(f32(s) / f32(n))


def area(b):
    return int(b[2]) * int(b[3])


def overlap_area(a, b):
    x1, y1 = max(int(a[0]), int(b[0])), max(int(a[1]), int(b[1]))
    w, h = min(int(a[0]) + int(a[2]), int(b[0]) + int(b[2])) - x1, min(int(a[1]) + int(a[3]), int(b[1]) + int(b[3])) - y1
    return 0 if w <= 0 or h <= 0 else w * h


def ratio(a, b):
    o = overlap_area(a, b)
    return f32(f32(o) / f32(area(a) + area(b) - o))


def ratio_former(a, b):
    return f32(f32(overlap_area(a, b)) / f32(area(a)))


def ratio_latter(a, b):
    return f32(f32(overlap_area(a, b)) / f32(area(b)))


def num_overlaps(boxes, f):
    return sum(1 for l in range(len(boxes)) if l != f and f64(ratio_latter(boxes[f], boxes[l])) > CROWD_RATIO)


def remove_bad_boxes(boxes, score, cols, rows, n, num):
    """:1879-1945 -> (bad, on_edge) per box"""
    M = len(boxes)
    bad, edge = [num[f] > CROWD_MAX for f in range(M)], [False] * M
    for f in range(M):
        if bad[f]:
            continue
        x, y, w, h = (int(v) for v in boxes[f])
        if f64(f32(f32(area(boxes[f])) / f32(cols * rows))) > LARGE_AREA_RATIO:
            bad[f] = True
        if n[f] < FEW_POINTS:
            bad[f] = True
        elif FEW_POINTS <= n[f] < FEW_POINTS_ON_EDGE:
            if x < FEW_POINTS_EDGE_PIXELS or y < FEW_POINTS_EDGE_PIXELS or x + w > cols - FEW_POINTS_EDGE_PIXELS or y + h > rows - FEW_POINTS_EDGE_PIXELS:
                bad[f] = True
        if x < ON_EDGE_PIXELS or y < ON_EDGE_PIXELS or x + w > cols - ON_EDGE_PIXELS or y + h > rows - ON_EDGE_PIXELS:
            edge[f] = True
        for l in range(M):
            if bad[l] or f == l:
                continue
            if f64(ratio(boxes[f], boxes[l])) > SAME_OBJECT_IOU:
                if score[f] < score[l]:
                    bad[f] = True
                elif score[f] >= score[l]:
                    bad[l] = True
            if f64(ratio(boxes[f], boxes[l])) > SURROUND_IOU:
                if f64(ratio_former(boxes[f], boxes[l])) > SURROUND_RATIO:
                    bad[f] = True
                if f64(ratio_latter(boxes[f], boxes[l])) > SURROUND_RATIO:
                    bad[l] = True
    return bad, edge


def boxplot_gate(n):
    """the inner gate of RemoveOutliersByBoxPlot (src/Object.cc:131): True = it returns"""
    return n // 4 <= 0 or n * 3 // 4 >= n - 1


def thresholds(q1, q3):
    iqr = f32(f32(q3) - f32(q1))
    return f32(f64(q3) + IQR_FACTOR * f64(iqr))


def zero_sign_invariant(z, q1, q3):
    """True when flipping the sign of a zero Q1 / Q3 changes neither max_th's value nor a `z > max_th` verdict"""
    want = [bool(v > thresholds(q1, q3)) for v in z]
    for a in ((q1, -q1) if q1 == 0 else (q1,)):
        for b in ((q3, -q3) if q3 == 0 else (q3,)):
            th = thresholds(a, b)
            if not (th == thresholds(q1, q3) or (np.isnan(th) and np.isnan(thresholds(q1, q3)))) or [bool(v > th) for v in z] != want:
                return False
    return True


def _mean_and_standard(xyz, lst, s):
    n = len(lst)
    pos = [mat_div(s[a], n) for a in range(3)]
    sum2 = [f32(0), f32(0), f32(0)]
    for i in lst:
        for a in range(3):
            d = f32(xyz[i, a] - pos[a])
            sum2[a] = f32(sum2[a] + f32(d * d))
    return pos, [np.sqrt(f32(sum2[a] / f32(n))) for a in range(3)]


def _finish(fr, lists_a, lists_k, sums, stats, feat_of):
    """steps 5 and 6 and the records, shared by the two forms: feat_of(i) = the keypoint whose coordinates keypoint i's map point carries in `feature`"""
    kx, ky, ids, xyz, boxes, score, T = _arrays(fr)
    M, cols, rows = len(boxes), int(fr["cols"]), int(fr["rows"])
    rec, variant = np.zeros(M, RECORD_DTYPE), []
    fx, fy, cx, cy = f32(fr["fx"]), f32(fr["fy"]), f32(fr["cx"]), f32(fr["cy"])
    for k in range(M):
        r, lst = rec[k], lists_k[k]
        r["n_assigned"], r["n"] = len(lists_a[k]), len(lst)
        r["sum_pos"] = sums[k]
        pos, sd, ran, q1, q3, th = stats[k]
        pos = [mat_div(sums[k][a], len(lst)) for a in range(3)]      # :1806, the same value again
        r["pos"], r["std"], r["boxplot_ran"], r["q1"], r["q3"], r["max_th"] = pos, sd, ran, q1, q3, th
        plain = [plain_div(sums[k][a], len(lst)) for a in range(3)]
        variant.append(any(np.asarray(p, f32).view(np.uint32) != np.asarray(q, f32).view(np.uint32) and not (np.isnan(p) and np.isnan(q)) for p, q in zip(pos, plain)))
        xc, yc, zc = (camera_row(T, a, pos) for a in range(3))
        invzc = f32(f64(1.0) / f64(zc))
        r["center_2d"] = [f32(f32(f32(fx * xc) * invzc) + cx), f32(f32(f32(fy * yc) * invzc) + cy)]
        if len(lst) >= FEATURE_RECT_MIN_POINTS:
            xs, ys = [kx[feat_of(i)] for i in lst], [ky[feat_of(i)] for i in lst]
            x_min, x_max, y_min, y_max = min(xs), max(xs), min(ys), max(ys)
            if x_min < 0:
                x_min = f32(0)
            if y_min < 0:
                y_min = f32(0)
            if x_max > f32(cols):
                x_max = f32(cols)
            if y_max > f32(rows):
                y_max = f32(rows)
            r["has_feature_rect"] = 1
            r["feature_rect"] = [int(np.trunc(x_min)), int(np.trunc(y_min)), int(np.trunc(f32(x_max - x_min))), int(np.trunc(f32(y_max - y_min)))]
        r["num_overlaps"] = num_overlaps(boxes, k)
    bad, edge = remove_bad_boxes(boxes, score, cols, rows, [int(v) for v in rec["n"]], [int(v) for v in rec["num_overlaps"]])
    rec["bad"], rec["on_edge"] = bad, edge
    return dict(records=rec, assigned=[np.array(l, np.int32) for l in lists_a], kept=[np.array(l, np.int32) for l in lists_k], variant=variant)


def literal(fr):
    with np.errstate(all="ignore"):
        kx, ky, ids, xyz, boxes, score, T = _arrays(fr)
        M = len(boxes)
        lists, sums, feature = [[] for _ in range(M)], [[f32(0), f32(0), f32(0)] for _ in range(M)], {}
        px, py = np.rint(kx).astype(np.int64), np.rint(ky).astype(np.int64)      # (cvRound of every keypoint, once)
        for i in range(len(kx)):
            if ids[i] < 0:
                continue
            for k in range(M):
                b = boxes[k]
                if b[0] <= px[i] < int(b[0]) + int(b[2]) and b[1] <= py[i] < int(b[1]) + int(b[3]):
                    feature[int(ids[i])] = i
                    lists[k].append(i)
                    sums[k] = [f32(sums[k][a] + xyz[i, a]) for a in range(3)]
        kept, stats = [], []
        for k in range(M):
            lst = list(lists[k])
            pos, sd = _mean_and_standard(xyz, lst, sums[k])
            ran, q1, q3, th = 0, f32(0), f32(0), f32(0)
            if len(lst) >= BOXPLOT_MIN_POINTS:
                z_c = sorted(camera_row(T, 2, xyz[i]) for i in lst)
                if not boxplot_gate(len(z_c)):
                    q1, q3 = z_c[len(z_c) // QUARTILE_DIVISOR], z_c[len(z_c) * 3 // QUARTILE_DIVISOR]
                    th = thresholds(q1, q3)
                    j = 0
                    while j < len(lst):      # the erase loop of :142-154
                        if camera_row(T, 2, xyz[lst[j]]) > th:
                            del lst[j]
                        else:
                            j += 1
                    ran = 1
                    pos, sd = _mean_and_standard(xyz, lst, sums[k])
            kept.append(lst)
            stats.append((pos, sd, ran, q1, q3, th))
        return _finish(fr, lists, kept, sums, stats, lambda i: feature[int(ids[i])])


def same_id_links(ids):
    nxt, later = np.full(len(ids), -1, np.int64), {}
    for i in range(len(ids) - 1, -1, -1):
        if ids[i] >= 0:
            nxt[i] = later.get(int(ids[i]), -1)
            later[int(ids[i])] = i
    return nxt


def compact(fr):
    with np.errstate(all="ignore"):
        kx, ky, ids, xyz, boxes, score, T = _arrays(fr)
        M = len(boxes)
        px, py = np.rint(kx).astype(np.int64), np.rint(ky).astype(np.int64)
        inside = [(ids >= 0) & (b[0] <= px) & (px < int(b[0]) + int(b[2])) & (b[1] <= py) & (py < int(b[1]) + int(b[3])) for b in boxes]
        any_box = np.logical_or.reduce(inside) if M else np.zeros(len(kx), bool)
        nxt = same_id_links(ids)

        def feat_of(i):      # k_frame_features: the last keypoint of the chain that lies in any box
            last, j = i, nxt[i]
            while j >= 0:
                if any_box[j]:
                    last = j
                j = nxt[j]
            return last

        lists, kept, sums, stats = [], [], [], []
        for k in range(M):
            place = np.cumsum(inside[k]) - 1      # the prefix count: a hit's place in the list
            lst = np.zeros(int(inside[k].sum()), np.int64)
            lst[place[inside[k]]] = np.nonzero(inside[k])[0]
            s = [f32(0), f32(0), f32(0)]
            for i in lst:
                s = [f32(s[a] + xyz[i, a]) for a in range(3)]
            n_a = len(lst)
            ran, q1, q3, th = 0, f32(0), f32(0), f32(0)
            keep = np.ones(n_a, bool)
            if n_a >= BOXPLOT_MIN_POINTS:
                z = np.array([camera_row(T, 2, xyz[i]) for i in lst], f32)
                lt, le = (z[None, :] < z[:, None]).sum(1), (z[None, :] <= z[:, None]).sum(1)
                k1, k3 = n_a // QUARTILE_DIVISOR, n_a * 3 // QUARTILE_DIVISOR
                q1, q3 = z[np.nonzero((lt <= k1) & (k1 < le))[0][0]], z[np.nonzero((lt <= k3) & (k3 < le))[0][0]]
                th = thresholds(q1, q3)
                keep, ran = ~(z > th), 1
            place = np.cumsum(keep) - 1
            lst_k = np.zeros(int(keep.sum()), np.int64)
            lst_k[place[keep]] = lst[keep]
            pos, sd = _mean_and_standard(xyz, lst_k, s)
            lists.append([int(i) for i in lst])
            kept.append([int(i) for i in lst_k])
            sums.append(s)
            stats.append((pos, sd, ran, q1, q3, th))
        return _finish(fr, lists, kept, sums, stats, feat_of)


def drop_zero_signs(rec):
    """the records with +0.0 for a zero q1, q3 or max_th"""
    out = rec.copy()
    for k in ("q1", "q3", "max_th"):
        out[k] = out[k] + f32(0.0)
    return out


def same_records(a, b):
    """field by field: floats as 32-bit patterns, NaN by isnan"""
    for name in RECORD_DTYPE.names:
        x, y = np.asarray(a[name]), np.asarray(b[name])
        if x.shape != y.shape:
            return False
        if x.dtype == np.float32:
            nan = np.isnan(x)
            if not (np.array_equal(nan, np.isnan(y)) and np.array_equal(x.view(np.uint32)[~nan], y.view(np.uint32)[~nan])):
                return False
        elif not np.array_equal(x, y):
            return False
    return True


def same(a, b, zero_signs=True):
    """two results: every field of every record and both lists; zero_signs=False drops the signs of zero quartiles first (literal against compact)"""
    ra, rb = (a["records"], b["records"]) if zero_signs else (drop_zero_signs(a["records"]), drop_zero_signs(b["records"]))
    return (same_records(ra, rb) and len(a["assigned"]) == len(b["assigned"]) and all(np.array_equal(p, q) for p, q in zip(a["assigned"], b["assigned"]))
            and all(np.array_equal(p, q) for p, q in zip(a["kept"], b["kept"])))


def hx(a):
    return " ".join("%08x" % v for v in np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32))


def walk_script(fr):
    """a frame as tools/frame_objects_walk.cpp reads it"""
    kx, ky, ids, xyz, boxes, score, T = _arrays(fr)
    head = "frame %d %d %d %d %s %s" % (len(kx), len(boxes), fr["cols"], fr["rows"], hx([fr["fx"], fr["fy"], fr["cx"], fr["cy"]]), hx(T))
    kps = " ".join("%s %d %s" % (hx([kx[i], ky[i]]), ids[i], hx(xyz[i])) for i in range(len(kx)))
    bxs = " ".join("%d %d %d %d %s" % (tuple(int(v) for v in boxes[k]) + (hx([score[k]]),)) for k in range(len(boxes)))
    return " ".join(p for p in (head, kps, bxs) if p) + "\n"


def walk_lines(res, zero_signs=True):
    """a result as tools/frame_objects_walk.cpp prints it (NaN as `nan`: its payload is nobody's contract)"""
    rec = res["records"] if zero_signs else drop_zero_signs(res["records"])
    out = []
    for k, r in enumerate(rec):
        fl = np.concatenate([r["sum_pos"], r["pos"], r["std"], [r["q1"], r["q3"], r["max_th"]], r["center_2d"]]).astype(np.float32)
        out.append("rec %d %d %d %d %d %d %d %d %d %d %d %s" % (r["n_assigned"], r["n"], r["boxplot_ran"], r["has_feature_rect"], *[int(v) for v in r["feature_rect"]],
                                                               r["num_overlaps"], r["bad"], r["on_edge"],
                                                               " ".join("nan" if np.isnan(v) else "%08x" % np.float32(v).view(np.uint32) for v in fl)))
        out.append(("a " + " ".join(str(int(i)) for i in res["assigned"][k])).rstrip())
        out.append(("k " + " ".join(str(int(i)) for i in res["kept"][k])).rstrip())
    return out
