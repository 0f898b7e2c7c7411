"""The yardstick of the yolox feature: what YOLOX::Detect does around the network (reference src/YOLOX.cc:51-62, :85-274; the grey image of
src/Tracking.cc:324-330) in numpy float32 scalars, twice:

    literal      the loops of :166-209, the Hoare quicksort of :85-122, NmsSortedBboxes, the rescale and clip; oracle.resize_linear per channel for the letterbox
    vectorised   numpy arrays, with the device's tie rule (equal probs in proposal order)

Each takes the exponential as a parameter: exp_double (np.float32(math.exp(float(x)))), or a table of recorded values of a machine's expf (exp_table).  np.exp on
float32 is numpy's own SIMD routine and is not used."""
import math

import numpy as np

F = np.float32
STRIDES = (8, 16, 32)                                   # src/YOLOX.cc:238
MEAN = (F(0.485), F(0.456), F(0.406))                   # :219 (std::vector<float>)
STD = (F(0.229), F(0.224), F(0.225))                    # :220
PAD = 114                                               # :59
CONF, NMS = F(0.3), F(0.65)                             # BBOX_CONF_THRESH, NMS_THRESH passed on as floats
OBJECT = np.dtype([("x", "<f4"), ("y", "<f4"), ("w", "<f4"), ("h", "<f4"), ("prob", "<f4"), ("label", "<i4")])
TRACKING_MIN_PROB = 0.5                                 # src/Tracking.cc:434
TRACKING_CLASSES = (0, 24, 28, 39, 56, 57, 58, 59, 60, 62, 63, 66, 67, 73)      # :439


# ---------------------------------------------------------------- the exponential
def exp_double(x):
    try:
        with np.errstate(over="ignore"):
            return F(math.exp(float(x)))
    except OverflowError:
        return F(np.inf)


def exp_table(inputs, outputs):
    """the recorded exponential of a machine: float32 bit pattern -> float32"""
    t = {int(a): F(b) for a, b in zip(np.asarray(inputs, np.float32).view(np.uint32), np.asarray(outputs, np.float32))}
    return lambda x: t[int(F(x).view(np.uint32))]


# ---------------------------------------------------------------- geometry
def geometry(cols, rows, S):
    """(r, unpad_w, unpad_h) of :53-56, or None where cv::resize would assert"""
    r = F(min(S / (cols * 1.0), S / (rows * 1.0)))
    uw, uh = int(F(r * F(cols))), int(F(r * F(rows)))
    return None if uw < 1 or uh < 1 else (r, uw, uh)


def anchors(S):
    """(grid0, grid1, stride) rows of GenerateGridsAndStride (:64-77)"""
    return [(g0, g1, s) for s in STRIDES for g1 in range(S // s) for g0 in range(S // s)]


# ---------------------------------------------------------------- pre-processing
def blob_table():
    return np.array([[(F(v) / F(255.0) - MEAN[c]) / STD[c] for v in range(256)] for c in range(3)], np.float32)


def letterbox(img, S, resize):
    """StaticResize: resize = oracle.resize_linear, applied per channel"""
    g = geometry(img.shape[1], img.shape[0], S)
    assert g is not None
    _, uw, uh = g
    out = np.full((S, S, 3), PAD, np.uint8)
    for c in range(3):
        out[:uh, :uw, c] = resize(np.ascontiguousarray(img[:, :, c]), uw, uh)
    return out


def blob_literal(canvas):
    """BlobFromImage (:211-233) pixel by pixel: B and R swapped first"""
    S = canvas.shape[0]
    rgb = canvas[:, :, ::-1]
    blob = np.zeros((3, S, S), np.float32)
    for c in range(3):
        for h in range(S):
            for w in range(S):
                blob[c, h, w] = (F(rgb[h, w, c]) / F(255.0) - MEAN[c]) / STD[c]
    return blob


def blob_vectorised(canvas):
    t = blob_table()
    return np.stack([t[c][canvas[:, :, 2 - c]] for c in range(3)])


def gray(img, rgb):
    """OpenCV 3.x 8-bit RGB2GRAY / BGR2GRAY"""
    a = img.astype(np.int64)
    r, b = (a[:, :, 0], a[:, :, 2]) if rgb else (a[:, :, 2], a[:, :, 0])
    return ((r * 4899 + a[:, :, 1] * 9617 + b * 1868 + 8192) >> 14).astype(np.uint8)


# ---------------------------------------------------------------- the literal decode
def proposals_literal(feat, S, nc, conf, ex):
    out = []
    for a, (g0, g1, stride) in enumerate(anchors(S)):
        f = feat[a]
        xc = F(F(f[0] + F(g0)) * F(stride))
        yc = F(F(f[1] + F(g1)) * F(stride))
        with np.errstate(over="ignore", invalid="ignore"):
            w = F(ex(f[2]) * F(stride))
            h = F(ex(f[3]) * F(stride))
            x0 = F(xc - F(w * F(0.5)))
            y0 = F(yc - F(h * F(0.5)))
        for c in range(nc):
            with np.errstate(over="ignore", invalid="ignore", under="ignore"):
                p = F(f[4] * f[5 + c])
            if p > conf:
                out.append((x0, y0, w, h, p, c))
    return out


def qsort_descent(v, left, right):
    """:85-122, the two sections one after the other"""
    i, j = left, right
    p = v[(left + right) // 2][4]
    while i <= j:
        while v[i][4] > p:
            i += 1
        while v[j][4] < p:
            j -= 1
        if i <= j:
            v[i], v[j] = v[j], v[i]
            i += 1
            j -= 1
    if left < j:
        qsort_descent(v, left, j)
    if i < right:
        qsort_descent(v, i, right)


def _rmax(a, b):
    return b if a < b else a


def _rmin(a, b):
    return b if b < a else a


def iou_terms(a, b):
    """(inter, union) of the later box a and the picked box b, as :154-155 with cv::Rect_<float>::operator&"""
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        x1, y1 = _rmax(a[0], b[0]), _rmax(a[1], b[1])
        w = F(_rmin(F(a[0] + a[2]), F(b[0] + b[2])) - x1)
        h = F(_rmin(F(a[1] + a[3]), F(b[1] + b[3])) - y1)
        if w <= 0 or h <= 0:
            w = h = F(0)
        inter = F(w * h)
        return inter, F(F(F(a[2] * a[3]) + F(b[2] * b[3])) - inter)


def nms_literal(v, nms, trace=None):
    picked = []
    for i in range(len(v)):
        keep = True
        for j in picked:
            inter, union = iou_terms(v[i], v[j])
            with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
                q = F(inter / union)
            if trace is not None:
                trace.append(q)
            if q > nms:
                keep = False
        if keep:
            picked.append(i)
    return picked


def rescale_clip(o, scale, img_w, img_h):
    """:258-272"""
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        x0, y0 = F(o[0] / scale), F(o[1] / scale)
        x1, y1 = F(F(o[0] + o[2]) / scale), F(F(o[1] + o[3]) / scale)
        x0 = _rmax(_rmin(x0, F(img_w - 1)), F(0))
        y0 = _rmax(_rmin(y0, F(img_h - 1)), F(0))
        x1 = _rmax(_rmin(x1, F(img_w - 1)), F(0))
        y1 = _rmax(_rmin(y1, F(img_h - 1)), F(0))
        return (x0, y0, F(x1 - x0), F(y1 - y0), o[4], o[5])


def records(rows):
    out = np.zeros(len(rows), OBJECT)
    for k, r in enumerate(rows):
        out[k] = tuple(r)
    return out


def count_tied(probs):
    b = np.sort(np.asarray(probs, np.float32).view(np.uint32))
    if len(b) < 2:
        return 0
    same = b[1:] == b[:-1]
    return int((np.concatenate([[False], same]) | np.concatenate([same, [False]])).sum())


def decode_literal(feat, S, img_w, img_h, ex=exp_double, nc=80, conf=CONF, nms=NMS, stable=False):
    """DecodeOutputs (:235-274).  stable = False: the reference's own order.  Returns dict(objects, proposals (sorted), picked, n_tied, ious (every quotient the
    greedy loop compared))."""
    feat = np.asarray(feat, np.float32).reshape(-1, 5 + nc)
    scale = geometry(img_w, img_h, S)[0]
    v = proposals_literal(feat, S, nc, conf, ex)
    if stable:
        v = [v[k] for k in sorted(range(len(v)), key=lambda k: (-float(v[k][4]), k))]
    elif v:
        qsort_descent(v, 0, len(v) - 1)
    ious = []
    picked = nms_literal(v, nms, ious)
    return dict(objects=records([rescale_clip(v[k], scale, img_w, img_h) for k in picked]), proposals=records(v), picked=picked,
                n_tied=count_tied([r[4] for r in v]), ious=np.array(ious, np.float32))


# ---------------------------------------------------------------- the vectorised decode (stable tie rule)
def decode_vectorised(feat, S, img_w, img_h, ex=exp_double, nc=80, conf=CONF, nms=NMS):
    feat = np.asarray(feat, np.float32).reshape(-1, 5 + nc)
    scale = geometry(img_w, img_h, S)[0]
    A = np.array(anchors(S), np.int32)
    g0, g1, st = A[:, 0].astype(np.float32), A[:, 1].astype(np.float32), A[:, 2].astype(np.float32)
    ew = np.array([ex(x) for x in feat[:, 2]], np.float32)
    eh = np.array([ex(x) for x in feat[:, 3]], np.float32)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        xc, yc = (feat[:, 0] + g0) * st, (feat[:, 1] + g1) * st
        w, h = ew * st, eh * st
        x0, y0 = xc - w * F(0.5), yc - h * F(0.5)
        prob = feat[:, 4:5] * feat[:, 5:]
    ai, ci = np.nonzero(prob > conf)      # row-major: anchor outer, class inner = proposal order
    p = prob[ai, ci]
    order = np.argsort(-p.astype(np.float64), kind="stable")
    ai, ci, p = ai[order], ci[order], p[order]
    bx, by, bw, bh = x0[ai], y0[ai], w[ai], h[ai]
    picked = []
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        area = bw * bh
        for i in range(len(p)):
            if picked:
                j = np.array(picked)
                x1 = np.where(bx[i] < bx[j], bx[j], bx[i])
                y1 = np.where(by[i] < by[j], by[j], by[i])
                ra, rb = bx[i] + bw[i], bx[j] + bw[j]
                ww = np.where(rb < ra, rb, ra) - x1
                ba, bb = by[i] + bh[i], by[j] + bh[j]
                hh = np.where(bb < ba, bb, ba) - y1
                empty = (ww <= 0) | (hh <= 0)
                inter = np.where(empty, F(0), ww) * np.where(empty, F(0), hh)
                if ((inter / ((area[i] + area[j]) - inter)) > nms).any():
                    continue
            picked.append(i)
    props = np.zeros(len(p), OBJECT)
    for k, a in (("x", bx), ("y", by), ("w", bw), ("h", bh), ("prob", p), ("label", ci)):
        props[k] = a
    return dict(objects=records([rescale_clip(tuple(props[k]), scale, img_w, img_h) for k in picked]), proposals=props, picked=picked, n_tied=count_tied(p))


# ---------------------------------------------------------------- Tracking's filter
def tracking_boxes(objects):
    """src/Tracking.cc:431-452: prob >= 0.5, the class list, descending score (equal scores keep their order)"""
    keep = [o for o in objects if not float(o["prob"]) < TRACKING_MIN_PROB and int(o["label"]) in TRACKING_CLASSES]
    keep.sort(key=lambda o: -float(o["prob"]))
    return records([tuple(o) for o in keep])


def same_records(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
