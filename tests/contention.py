"""Contention meter for the greedy guided searches (numpy, no GPU).

ORBmatcher walks its queries in index order and a keypoint claimed by an earlier query is skipped by every later one
(src/ORBmatcher.cc:87-89, 123 for SearchByProjection(Frame, MapPoints); :1413-1424 for SearchByProjection(Cur, Last)).  A scene only
tests that order if it decides something, so this module replays both searches twice from the same candidate lists -- greedily, as the
reference does, and with every query decided on its own (claims ignored, prior occupancy kept) -- and counts what the order decided:
  differ        queries whose outcome (matched keypoint or none) differs between the two replays
  differ_ratio  ... because the ratio test passes in one replay and fails in the other (a claimed keypoint moved the best or the second best)
  differ_best   ... otherwise: another best free candidate, or one beyond TH_HIGH
  tie_equal     greedy decisions with best == second best (the first of equal distances wins)
  tie_th        greedy decisions with best == TH_HIGH
  tie_ratio     greedy decisions at one level with best == nnratio * second (float32, as the reference compares)
  hist_equal    (Cur, Last) rotation-histogram bins whose count equals that of a bin on the other side of the keep / drop line
  hist_tenth    (Cur, Last) bins kept or dropped with a count of exactly 0.1 x the fullest bin
  hist_boundary (Cur, Last) greedy matches whose rotation times the bin factor is exactly half-way between two bins in float32
The same replays are the brute force the CPU suite holds the oracle to (`points`, `frames`)."""
import numpy as np

F32 = np.float32
TH_HIGH, HISTO = 100, 30


def _cround(x):
    """C round() of float32 values: half away from zero."""
    return (np.floor(np.abs(x) + F32(0.5)) * np.sign(x)).astype(np.int64)


def hamming(a, b):
    """(len(a), len(b)) Hamming distances of 32-byte descriptors."""
    A = np.unpackbits(np.asarray(a, np.uint8), axis=1).astype(np.int32)
    B = np.unpackbits(np.asarray(b, np.uint8), axis=1).astype(np.int32)
    return A.sum(1)[:, None] + B.sum(1)[None, :] - 2 * (A @ B.T)


class Grid:
    """Frame::AssignFeaturesToGrid / GetFeaturesInArea (src/Frame.cc:599-614, 696-761) over arrays: 64 x 48 cells, keypoints visited
    cell by cell (column-major) and in index order inside a cell."""
    def __init__(self, F):
        self.F = F
        self.iw = F32(64) / F32(F32(F["max_x"]) - F32(F["min_x"]))
        self.ih = F32(48) / F32(F32(F["max_y"]) - F32(F["min_y"]))
        self.kx, self.ky = np.asarray(F["kp_x"], F32), np.asarray(F["kp_y"], F32)
        self.px = _cround((self.kx - F32(F["min_x"])) * self.iw)
        self.py = _cround((self.ky - F32(F["min_y"])) * self.ih)
        inside = (self.px >= 0) & (self.px < 64) & (self.py >= 0) & (self.py < 48)
        self.order = np.array(sorted(np.nonzero(inside)[0], key=lambda i: (self.px[i], self.py[i], i)), np.int64)
        self.oct = np.asarray(F["kp_octave"], np.int64)

    def area(self, x, y, r, lo, hi):
        F, o = self.F, self.order
        x, y, r = F32(x), F32(y), F32(r)
        x0 = max(0, int(np.floor((x - F32(F["min_x"]) - r) * self.iw)))
        x1 = min(63, int(np.ceil((x - F32(F["min_x"]) + r) * self.iw)))
        y0 = max(0, int(np.floor((y - F32(F["min_y"]) - r) * self.ih)))
        y1 = min(47, int(np.ceil((y - F32(F["min_y"]) + r) * self.ih)))
        if x0 >= 64 or x1 < 0 or y0 >= 48 or y1 < 0:
            return o[:0]
        px, py, oc = self.px[o], self.py[o], self.oct[o]
        ok = (px >= x0) & (px <= x1) & (py >= y0) & (py <= y1)
        if lo > 0 or hi >= 0:
            ok &= oc >= lo
            if hi >= 0:
                ok &= oc <= hi
        ok &= (np.abs(self.kx[o] - x) < r) & (np.abs(self.ky[o] - y) < r)
        return o[ok]


def _replay(cands, dist, occ0, octs, greedy, ratio):
    """The selection loop of both searches over candidate lists (query order = list order).  ratio None: no ratio test (Cur, Last).
    Returns per query (taken keypoint or -1, best keypoint or -1, best, best2, level, level2)."""
    occ = occ0.copy()
    out = []
    for q, c in enumerate(cands):
        best, best2, bl, bl2, bi = 256, 256, -1, -1, -1
        for i in c:
            if occ[i]:
                continue
            d = int(dist[q, i])
            if d < best:
                best2, best, bl2, bl, bi = best, d, bl, int(octs[i]), int(i)
            elif d < best2:
                bl2, best2 = int(octs[i]), d
        take = -1
        if best <= TH_HIGH and not (ratio is not None and bl == bl2 and best > F32(ratio) * F32(best2)):
            take = bi
            if greedy:
                occ[bi] = True
        out.append((take, bi, best, best2, bl, bl2))
    return out


def points_candidates(F, M, th):
    """SearchByProjection(Frame&, vector<MapPoint*>, th) candidate lists (src/ORBmatcher.cc:51-100) in grid order; None for a skipped query."""
    g = Grid(F)
    ur = np.asarray(F["u_right"], F32)
    out = []
    for m in range(len(M["level"])):
        if M["skip"][m]:
            out.append(np.zeros(0, np.int64))
            continue
        lvl = int(M["level"][m])
        r = F32(2.5) if M["view_cos"][m] > F32(0.998) else F32(4.0)
        if th != 1.0:
            r = F32(r * F32(th))
        rs = F32(r * F32(F["scale_factors"][lvl]))
        c = g.area(M["proj_x"][m], M["proj_y"][m], rs, lvl - 1, lvl)
        keep = ~((ur[c] > 0) & (np.abs(F32(M["proj_xr"][m]) - ur[c]) > rs))
        out.append(c[keep])
    return out


def points(F, M, th, ratio, greedy=True):
    """Brute-force SearchByProjection(Frame&, MapPoints, th): the keypoint every map point takes (-1: none), and the replay's rows."""
    cands = points_candidates(F, M, th)
    dist = hamming(M["descriptors"], F["descriptors"])
    occ0 = np.asarray(F["occupied"], bool) if F.get("occupied") is not None else np.zeros(len(F["kp_x"]), bool)
    rows = _replay(cands, dist, occ0, np.asarray(F["kp_octave"]), greedy, ratio)
    return np.array([r[0] for r in rows], np.int64), rows, cands


def _project_last(cur, last):
    """Rcw * Xw + tcw with double accumulation and one rounding to float (oracle/match_cpu.cpp, cv::gemm's small-matrix path)."""
    T = np.asarray(cur["Tcw"], F32).astype(np.float64)
    Xw = np.asarray(last["Xw"], F32).astype(np.float64)
    xc = (Xw @ T[:3, :3].T + T[:3, 3]).astype(F32)
    invz = (1.0 / xc[:, 2].astype(np.float64)).astype(F32)
    u = F32(cur["fx"]) * xc[:, 0] * invz + F32(cur["cx"])
    v = F32(cur["fy"]) * xc[:, 1] * invz + F32(cur["cy"])
    return u.astype(F32), v.astype(F32), invz


def _level_window(cur, last, mono):
    Tc = np.asarray(cur["Tcw"], F32).astype(np.float64)
    Tl = np.asarray(last["Tcw"], F32).astype(np.float64)
    twc = (-(Tc[:3, :3].T @ Tc[:3, 3])).astype(F32).astype(np.float64)
    tlc = (Tl[:3, :3] @ twc + Tl[:3, 3]).astype(F32)
    mb = F32(cur["mb"])
    return bool(tlc[2] > mb and not mono), bool(-tlc[2] > mb and not mono)


def frames_candidates(cur, last, th, mono):
    """SearchByProjection(Frame& Cur, const Frame& Last, th, bMono) candidate lists (src/ORBmatcher.cc:1340-1411) in grid order."""
    g = Grid(cur)
    u, v, invz = _project_last(cur, last)
    fwd, bwd = _level_window(cur, last, mono)
    urk = np.asarray(cur["u_right"], F32)
    out = []
    for i in range(len(last["valid"])):
        c = np.zeros(0, np.int64)
        if last["valid"][i] and invz[i] >= 0 and F32(cur["min_x"]) <= u[i] <= F32(cur["max_x"]) and F32(cur["min_y"]) <= v[i] <= F32(cur["max_y"]):
            o = int(last["octave"][i])
            rad = F32(F32(th) * F32(cur["scale_factors"][o]))
            lo, hi = (o, -1) if fwd else (0, o) if bwd else (o - 1, o + 1)
            c = g.area(u[i], v[i], rad, lo, hi)
            ur = F32(u[i] - F32(cur["mbf"]) * invz[i])
            c = c[~((urk[c] > 0) & (np.abs(ur - urk[c]) > rad))]
        out.append(c)
    return out


def rotation_bins(last_angle, cur_angle, factor=F32(HISTO / 360.0)):
    rot = (F32(last_angle) - F32(cur_angle)).astype(F32)
    rot = np.where(rot < 0, (rot + F32(360.0)).astype(F32), rot).astype(F32)
    prod = (rot * F32(factor)).astype(F32)
    b = _cround(prod)
    return np.where(b == HISTO, 0, b), prod


def three_maxima(counts):
    """ORBmatcher::ComputeThreeMaxima (src/ORBmatcher.cc:1603-1644) and the 0.1 cut of the caller: the bins that stay."""
    m1 = m2 = m3 = 0
    i1 = i2 = i3 = -1
    for b, s in enumerate(counts):
        if s > m1:
            m3, m2, m1, i3, i2, i1 = m2, m1, s, i2, i1, b
        elif s > m2:
            m3, m2, i3, i2 = m2, s, i2, b
        elif s > m3:
            m3, i3 = s, b
    if m2 < F32(0.1) * F32(m1):
        i2 = i3 = -1
    elif m3 < F32(0.1) * F32(m1):
        i3 = -1
    return {b for b in (i1, i2, i3) if b >= 0}


def frames(cur, last, th, mono, check_orientation=True, greedy=True):
    """Brute-force SearchByProjection(Cur, Last): per current keypoint the last-frame index it matched (-1: none), the number of matches,
    the replay's rows, the candidate lists and the histogram counts (None without the orientation check)."""
    cands = frames_candidates(cur, last, th, mono)
    dist = hamming(last["descriptors"], cur["descriptors"])
    occ0 = np.asarray(cur["occupied"], bool) if cur.get("occupied") is not None else np.zeros(len(cur["kp_x"]), bool)
    rows = _replay(cands, dist, occ0, np.asarray(cur["kp_octave"]), greedy, None)
    cm = np.full(len(cur["kp_x"]), -1, np.int64)
    hist = None
    for i, r in enumerate(rows):
        if r[0] >= 0:
            cm[r[0]] = i
    if check_orientation:
        k = np.nonzero(cm >= 0)[0]
        bins, _ = rotation_bins(np.asarray(last["angle"])[cm[k]], np.asarray(cur["kp_angle"])[k])
        hist = np.bincount(bins, minlength=HISTO)
        keep = three_maxima(hist)
        cm[k[~np.isin(bins, list(keep))]] = -1
    return cm, int((cm >= 0).sum()), rows, cands, hist


def _ties(rows, ratio):
    t = dict(tie_equal=0, tie_th=0, tie_ratio=0)
    for take, bi, best, best2, bl, bl2 in rows:
        if bi < 0:
            continue
        t["tie_equal"] += int(best == best2)
        t["tie_th"] += int(best == TH_HIGH)
        if ratio is not None and bl == bl2 and best2 < 256:
            t["tie_ratio"] += int(F32(best) == F32(ratio) * F32(best2))
    return t


def _differ(g, i, ratio):
    def refused(r):
        return ratio is not None and r[2] <= TH_HIGH and r[4] == r[5] and r[2] > F32(ratio) * F32(r[3])
    d = dict(differ=0, differ_best=0, differ_ratio=0)
    for a, b in zip(g, i):
        if a[0] != b[0]:
            d["differ"] += 1
            d["differ_ratio" if refused(a) != refused(b) else "differ_best"] += 1
    return d


def meter_points(F, M, th, ratio):
    _, g, _ = points(F, M, th, ratio, True)
    _, i, _ = points(F, M, th, ratio, False)
    out = dict(queries=len(g), matched=int(sum(r[0] >= 0 for r in g)))
    out.update(_differ(g, i, ratio))
    out.update(_ties(g, ratio))
    return out


def meter_frames(cur, last, th, mono):
    cm, nm, g, _, hist = frames(cur, last, th, mono, True, True)
    _, _, i, _, _ = frames(cur, last, th, mono, True, False)
    out = dict(queries=len(g), matched=int(sum(r[0] >= 0 for r in g)), kept=nm)
    out.update(_differ(g, i, None))
    out.update(_ties(g, None))
    keep = three_maxima(hist)
    kept = {int(hist[b]) for b in keep}
    dropped = {int(hist[b]) for b in range(HISTO) if b not in keep and hist[b] > 0}
    out["hist_equal"] = len(kept & dropped)
    m1 = int(hist.max()) if len(hist) else 0
    out["hist_tenth"] = int(sum(F32(hist[b]) == F32(0.1) * F32(m1) for b in range(HISTO) if hist[b] > 0))
    k = [r[0] for r in g if r[0] >= 0]
    qi = [q for q, r in enumerate(g) if r[0] >= 0]
    if k:
        _, prod = rotation_bins(np.asarray(last["angle"])[qi], np.asarray(cur["kp_angle"])[k])
        out["hist_boundary"] = int((prod - np.floor(prod) == F32(0.5)).sum())
    else:
        out["hist_boundary"] = 0
    return out
