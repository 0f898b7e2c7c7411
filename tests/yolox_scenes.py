"""Seeded head outputs for the yolox decode, each naming the branch of DecodeOutputs (reference src/YOLOX.cc:235-274) it reaches and carrying the predicate that
says so.  Inputs are built from exactly representable numbers and numpy's uniform / integer draws only (no libm call), so a fresh run gives the same bytes on
every machine.

    scenes() -> {name: dict(feat (anchors, 85) float32, S, img (w, h), branch, reaches(result) -> bool, tie (bool), [max_proposals], [overflow])}

`result` is a decode of tests/yolox_reference.py (objects, proposals, picked, n_tied[, ious]).  S = 64 has 84 anchors: 0 .. 63 an 8 x 8 grid of stride 8,
64 .. 79 a 4 x 4 grid of stride 16, 80 .. 83 a 2 x 2 grid of stride 32.  exp(1.0) * 8 = 21.75: two such boxes dx apart overlap by (21.75 - dx) / (21.75 + dx), which
is 0.65 at dx = 4.61."""
import numpy as np

F = np.float32
NC = 80


def _anchor_count(S):
    return sum((S // s) ** 2 for s in (8, 16, 32))


def _head(S):
    return np.zeros((_anchor_count(S), 5 + NC), np.float32)


def _put(feat, a, fx, fy, fw, fh, obj, classes):
    feat[a, :5] = (fx, fy, fw, fh, obj)
    for c, v in classes.items():
        feat[a, 5 + c] = v


def _scene(feat, S, img, branch, reaches, tie=False, **kw):
    return dict(feat=feat, S=S, img=img, branch=branch, reaches=reaches, tie=tie, **kw)


def _grid_scene(count):
    """`count` proposals on distinct anchors, distinct probs, neighbours overlapping by a quarter: all of them survive (one, two words of a matrix row)"""
    f = _head(64)
    for a in range(count):
        _put(f, a, 0.5, 0.5, 0.5, 0.5, 1.0, {a % NC: 0.35 + 0.005 * a})
    return _scene(f, 64, (100, 80), "%d proposals" % count, lambda r, n=count: len(r["proposals"]) == n and len(r["objects"]) == n and r["n_tied"] == 0)


def _stacked(count):
    """`count` proposals on one spot (anchors 27, 28 shifted onto each other): one survives"""
    f = _head(64)
    left = count
    for k, a in enumerate((27, 28, 35, 36)):
        m = min(left, NC)
        g0, g1 = a % 8, a // 8
        _put(f, a, 3.5 - g0, 3.5 - g1, 1.0, 1.0, 1.0, {c: 0.31 + 0.002 * c + 0.0001 * k for c in range(m)})
        left -= m
    assert left == 0
    return f


def scenes():
    out = {}
    out["none"] = _scene(_head(64), 64, (100, 80), "no proposal", lambda r: len(r["proposals"]) == 0 and len(r["objects"]) == 0)

    f = _head(64)
    _put(f, 9, 0.25, 0.75, 1.0, 0.5, 0.9, {17: 0.8})
    out["one"] = _scene(f, 64, (100, 80), "exactly one proposal", lambda r: len(r["proposals"]) == 1 and len(r["objects"]) == 1)

    f = _head(64)
    _put(f, 20, 0.5, 0.5, 1.0, 1.0, 1.0, {0: F(0.3), 1: np.nextafter(F(0.3), F(1))})
    out["at_threshold"] = _scene(f, 64, (100, 80), "a prob equal to the threshold is excluded",
                                 lambda r: len(r["proposals"]) == 1 and int(r["proposals"]["label"][0]) == 1)

    f = _head(64)
    _put(f, 66, 0.5, 0.5, 0.25, 0.25, 1.0, {c: 0.31 + 0.005 * c for c in range(NC)})
    out["all_classes"] = _scene(f, 64, (100, 80), "all 80 classes of one anchor", lambda r: len(r["proposals"]) == 80 and len(r["objects"]) == 1 and int(r["objects"]["label"][0]) == 79)

    f = _head(64)
    _put(f, 18, 0.5, 0.5, 1.0, 1.0, 0.9, {3: 0.9})
    _put(f, 19, -0.625, 0.5, 1.0, 1.0, 0.9, {41: 0.7})      # 3 px to the right of anchor 18's box: IoU 0.76
    out["cross_label"] = _scene(f, 64, (100, 80), "suppression across labels", lambda r: len(r["proposals"]) == 2 and len(r["objects"]) == 1 and int(r["objects"]["label"][0]) == 3)

    f = _head(64)
    _put(f, 82, 0.5, 0.5, 0.0, 0.0, 1.0, {5: 0.9})          # 32 x 32
    _put(f, 76, 0.5, 0.5, 0.0, 0.0, 1.0, {5: 0.8})          # 16 x 16 inside it: IoU 0.25, kept
    _put(f, 83, 0.4375, 0.5, 0.0, -0.25, 1.0, {6: 0.95})    # 32 x 24.9
    _put(f, 79, -0.125, 0.0, 0.5, 0.25, 1.0, {6: 0.6})      # 26.4 x 20.5 inside it: IoU 0.68, suppressed
    out["nested"] = _scene(f, 64, (100, 80), "nested boxes on both sides", lambda r: len(r["proposals"]) == 4 and len(r["objects"]) == 3 and (r["ious"] > 0).sum() >= 2)

    f = _head(64)
    for k, (a, dx, p) in enumerate(((9, 0.0, 0.9), (9 + 1, -1.0 + 0.375, 0.8), (9 + 2, -2.0 + 0.75, 0.7), (41, 0.0, 0.85), (42, -1.0 + 0.5, 0.75), (43, -2.0 + 0.625, 0.65))):
        _put(f, a, 0.5 + dx, 0.5, 1.0, 1.0, 1.0, {k: p})
    out["clusters"] = _scene(f, 64, (100, 80), "clusters on both sides of 0.65",
                             lambda r: len(r["proposals"]) == 6 and len(r["objects"]) == 4 and (r["ious"] > F(0.65)).any() and ((r["ious"] < F(0.65)) & (r["ious"] > 0.5)).any())

    f = _head(64)
    _put(f, 0, -1.0, -1.0, 1.0, 1.0, 1.0, {0: 0.9})         # beyond the left and top borders
    _put(f, 63, 1.5, 1.5, 1.5, 1.5, 1.0, {1: 0.8})          # beyond the right and bottom ones
    _put(f, 7, 1.5, -1.0, 0.5, 0.5, 1.0, {2: 0.7})
    _put(f, 56, -1.0, 1.5, 0.5, 0.5, 1.0, {3: 0.6})
    out["clipped"] = _scene(f, 64, (100, 80), "boxes clipped at all four borders",
                            lambda r: len(r["objects"]) == 4 and (r["objects"]["x"] == 0).any() and (r["objects"]["y"] == 0).any()
                            and (r["objects"]["x"] + r["objects"]["w"] == 99).any() and (r["objects"]["y"] + r["objects"]["h"] == 79).any())

    f = _head(64)
    _put(f, 10, 0.5, 0.5, -120.0, 1.0, 1.0, {0: 0.9})
    _put(f, 10 + 8, 0.5, -0.5, -120.0, 1.0, 1.0, {1: 0.8})  # the same zero-width box from the anchor below
    out["zero_area"] = _scene(f, 64, (100, 80), "a zero-area box from exp underflow: 0 / 0 is compared and the box is kept",
                              lambda r: len(r["objects"]) == 2 and (r["proposals"]["w"] == 0).all() and np.isnan(r["ious"]).any())

    f = _head(64)
    _put(f, 30, 0.5, 0.5, 100.0, 1.0, 1.0, {0: 0.9})
    _put(f, 31, 0.5, 0.5, 1.0, 100.0, 1.0, {1: 0.85})
    _put(f, 33, 0.5, 0.5, 1.0, 1.0, 1.0, {2: 0.8})
    out["infinite"] = _scene(f, 64, (100, 80), "an infinite box from exp overflow", lambda r: np.isinf(r["proposals"]["w"]).any() and np.isinf(r["proposals"]["h"]).any()
                             and len(r["proposals"]) == 3)

    for count in (63, 64, 65):
        out["count_%d" % count] = _grid_scene(count)

    out["capacity_128"] = _scene(_stacked(128), 64, (100, 80), "as many proposals as max_proposals", lambda r: len(r["proposals"]) == 128 and len(r["objects"]) == 1,
                                 max_proposals=128)
    out["capacity_129"] = _scene(_stacked(129), 64, (100, 80), "one proposal more than max_proposals", lambda r: len(r["proposals"]) == 129, max_proposals=128, overflow=True)

    f = _head(64)
    for k, a in enumerate((3, 21, 40, 58, 13)):      # five boxes apart from each other with one prob, around two others
        _put(f, a, 0.5, 0.5, 0.25, 0.25, 1.0, {10 + k: 0.75})
    _put(f, 25, 0.5, 0.5, 0.25, 0.25, 1.0, {1: 0.9})
    _put(f, 50, 0.5, 0.5, 0.25, 0.25, 1.0, {2: 0.5, 3: 0.5})
    out["tie"] = _scene(f, 64, (100, 80), "equal probs: the tie rule decides the order", lambda r: r["n_tied"] == 7 and len(r["objects"]) == 7, tie=True)

    rs = np.random.RandomState(6401)
    f = _head(64)
    f[:, 0:2] = rs.random_sample((84, 2)).astype(np.float32)
    f[:, 2:4] = (rs.random_sample((84, 2)) * 2.0 - 0.5).astype(np.float32)
    f[:, 4] = rs.random_sample(84).astype(np.float32)
    f[:, 5:] = (rs.random_sample((84, NC)) * 0.5).astype(np.float32)
    out["random_64"] = _scene(f, 64, (90, 120), "a dense random head", lambda r: len(r["proposals"]) >= 100 and 2 <= len(r["objects"]) < len(r["proposals"]) and r["n_tied"] == 0)

    rs = np.random.RandomState(64001)
    f = _head(640)
    for a in rs.choice(8400, 300, replace=False):
        f[a, 0:2] = rs.random_sample(2)
        f[a, 2:4] = rs.random_sample(2) * 2.0
        f[a, 4] = 0.5 + 0.5 * rs.random_sample()
        for c in rs.choice(NC, 2, replace=False):
            f[a, 5 + c] = rs.random_sample()
    out["head_640"] = _scene(f, 640, (848, 480), "a 640 head with a few hundred proposals", lambda r: 200 <= len(r["proposals"]) <= 600 and len(r["objects"]) >= 20 and r["n_tied"] == 0)
    return out
