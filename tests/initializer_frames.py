"""The text tests/cpp/initializer/initializer_driver.cpp reads for a problem of tests/initializer_scenes.py, and its output parsed."""
import numpy as np


def randi_of(sets, n):
    """the RandomInt results that make the draw loop of src/Initializer.cc:82-97 produce `sets`"""
    out = []
    for row in np.asarray(sets):
        avail = list(range(n))
        for idx in row:
            randi = avail.index(int(idx))
            out.append(randi)
            avail[randi] = avail[-1]
            avail.pop()
    return out


def frames_text(prob, sigma=None, randi=None):
    """(text, vMatches12): the frames, vMatches12 as Tracking holds it (-1 where a keypoint of frame 1 has no match) and the generator's replay"""
    k1, k2, m = np.asarray(prob["keys1"], np.float32), np.asarray(prob["keys2"], np.float32), np.asarray(prob["matches12"])
    v12 = -np.ones(len(k1), np.int64)
    v12[m[:, 0]] = m[:, 1]
    randi = randi_of(prob["sets"], len(m)) if randi is None else list(randi)
    rows = ["%.9g %.9g %.9g %.9g %.9g %d" % (tuple(prob["K"]) + (prob["sigma"] if sigma is None else sigma, len(randi) // 8))]
    for k in (k1, k2):
        rows.append("%d" % len(k))
        rows.append(" ".join("%.9g %.9g" % (x, y) for x, y in k))
    rows.append(" ".join("%d" % v for v in v12))
    rows.append("%d" % len(randi))
    rows.append(" ".join("%d" % v for v in randi))
    return "\n".join(rows) + "\n", v12


def parse_result(stdout):
    out = {}
    for line in stdout.strip().split("\n"):
        f = line.split()
        if f[0] == "call":
            out["call"] = f
        elif f[0] == "random":
            out.update(seeds=int(f[2]), draws=int(f[4]), bad=int(f[6]))
        elif f[0] == "returned":
            out["returned"] = f[1] == "1"
        elif f[0] in ("R21", "t21"):
            out[f[0]] = np.array(f[3:], np.float32).reshape(int(f[1]), int(f[2]))
            if f[0] == "t21" and out[f[0]].shape == (3, 1):
                out[f[0]] = out[f[0]].reshape(3)
        elif f[0] == "p3d":
            out["p3d"] = np.array(f[2:], np.float32).reshape(int(f[1]), 3)
        elif f[0] == "triangulated":
            out["triangulated"] = np.array(f[2:], np.int64).astype(bool)
    return out
