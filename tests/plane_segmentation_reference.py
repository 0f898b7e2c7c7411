"""Yardstick of the plane segmentation (csrc/plane_seg.hip, csrc/plane_seg_internal.h): Frame::ComputePlanesFromPEAC restated step by step.

Reference: src/Frame.cc:349-460 (cloud, per-plane voxel grid, PlaneNotSeen), include/Frame.h:67-85 (ImagePointCloud::get),
include/PEAC/AHCPlaneFitter.hpp (run :209, refineDetails :297-377, floodFill :426-474, findBlockMembership :483-585, initGraph :784-953,
ahCluster :981-1187), AHCPlaneSeg.hpp (Stats::compute :125-156, block constructor :211-285, merge constructor :293-316, mergeNbsFrom :379-409),
AHCParamSet.hpp (:68-76 defaults, T_mse :87-99, T_ang :112-132, T_dz :144-146), DisjointSet.hpp.

A double is a Python float (IEEE binary64, one rounding per operation); a float is a numpy.float32.  The readings DESIGN.md section 4k fixes:
  * an invalid pixel has z = 0, so get() is false;
  * std::pow(v, 2) is v * v;
  * the 3 x 3 eigen-solve is eig3_jacobi below (eig3_eigh, numpy.linalg.eigh, is the second variant, for the scenes' condition);
  * a neighbour set iterates in creation sequence, the queue orders by (mse, creation sequence), the size sort is stable, a NaN never enters the queue;
  * the voxel grid is the public PCL 1.8 algorithm with the sum of a voxel taken in ascending pixel index;
  * the membership image holds the final plane id or -1 (upstream leaves its trail counters behind).
"""
import math
from types import SimpleNamespace

import numpy as np

F32 = np.float32
NAN = float("nan")
FLT_MAX = float(np.finfo(np.float32).max)
INT_MAX = 2147483647

# src/Frame.cc:396, :436, :362-365
DEPTH_MAX, DEPTH_MIN, LEAF = 4.0, 0.2, 0.05
SEEN_DIST, SEEN_ANGLE = 0.2, 0.9397
# AHCPlaneFitter.hpp:152-156
MAX_STEP, MIN_SUPPORT, WINDOW = 100000, 3000, 10
# floodFill :443, :453
TRAIL_STOP, DIST_FACTOR, DIST_EPS = -6, 9, 1e-5
JACOBI_SWEEPS = 8


def default_cfg(width=640, height=480, fx=517.306408, fy=516.469215, cx=318.643040, cy=255.313989, **kw):
    c = SimpleNamespace(
        width=width, height=height, fx=F32(fx), fy=F32(fy), cx=F32(cx), cy=F32(cy), window=WINDOW, min_support=MIN_SUPPORT, max_step=MAX_STEP,
        depth_min=DEPTH_MIN, depth_max=DEPTH_MAX, leaf=F32(LEAF),
        # AHCParamSet.hpp:68-76; MACRO_DEG2RAD(d) is ((d)*M_PI/180.0)
        depth_sigma=1.6e-6, std_tol_init=5.0, std_tol_merge=8.0, z_near=500.0, z_far=4000.0, angle_near=15.0 * math.pi / 180.0,
        angle_far=90.0 * math.pi / 180.0, similarity_merge=math.cos(60.0 * math.pi / 180.0), similarity_refine=math.cos(30.0 * math.pi / 180.0),
        depth_alpha=0.04, depth_change_tol=0.02)
    for k, v in kw.items():
        assert hasattr(c, k), k
        setattr(c, k, v)
    return c


# ---- AHCParamSet.hpp
def t_mse_init(c, z):
    v = c.depth_sigma * z * z + c.std_tol_init
    return v * v


def t_mse_merge(c, z):
    v = c.depth_sigma * z * z + c.std_tol_merge
    return v * v


def t_ang_init(c, z):
    cz = z
    cz = c.z_near if cz < c.z_near else cz      # std::max(clipped_z, z_near)
    cz = c.z_far if c.z_far < cz else cz        # std::min(clipped_z, z_far)
    factor = (c.angle_far - c.angle_near) / (c.z_far - c.z_near)
    return math.cos(factor * cz + c.angle_near - factor * c.z_near)


def t_dz(c, z):
    return c.depth_alpha * abs(z) + c.depth_change_tol


# ---- step 1: src/Frame.cc:391-405
def pixel_valid(c, d):
    return not (math.isnan(d) or d > c.depth_max or d < c.depth_min)


def pixel_point(c, m, n, d):
    x = (float(n) - float(c.cx)) * d
    x = x / float(c.fx)
    y = (float(m) - float(c.cy)) * d
    y = y / float(c.fy)
    return x, y, d


# ---- the eigen-solve: cyclic Jacobi, pairs (0,1) (0,2) (1,2), JACOBI_SWEEPS sweeps whatever the input, then three compare-exchanges to ascending order
def eig3_jacobi(K):
    S = [[K[i][j] for j in range(3)] for i in range(3)]
    V = [[1.0 if i == j else 0.0 for j in range(3)] for i in range(3)]
    for _ in range(JACOBI_SWEEPS):
        for p, q in ((0, 1), (0, 2), (1, 2)):
            apq = S[p][q]
            c, s = 1.0, 0.0
            if apq != 0.0:
                theta = (S[q][q] - S[p][p]) / (2.0 * apq)
                t = (-1.0 if theta < 0.0 else 1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
                c = 1.0 / math.sqrt(t * t + 1.0)
                s = t * c
            for k in range(3):
                a, b = S[k][p], S[k][q]
                S[k][p] = c * a - s * b
                S[k][q] = s * a + c * b
            for k in range(3):
                a, b = S[p][k], S[q][k]
                S[p][k] = c * a - s * b
                S[q][k] = s * a + c * b
            for k in range(3):
                a, b = V[k][p], V[k][q]
                V[k][p] = c * a - s * b
                V[k][q] = s * a + c * b
    l = [S[0][0], S[1][1], S[2][2]]
    for a, b in ((0, 1), (1, 2), (0, 1)):
        if l[b] < l[a]:
            l[a], l[b] = l[b], l[a]
            for k in range(3):
                V[k][a], V[k][b] = V[k][b], V[k][a]
    return l, V


def eig3_eigh(K):
    w, v = np.linalg.eigh(np.array(K, np.float64))
    return [float(x) for x in w], [[float(v[i][j]) for j in range(3)] for i in range(3)]


EIG = dict(jacobi=eig3_jacobi, eigh=eig3_eigh)


# ---- Stats::compute, AHCPlaneSeg.hpp:125-156.  sums: sx sy sz sxx syy szz sxy syz sxz
def fit(sums, N, eig):
    sx, sy, sz, sxx, syy, szz, sxy, syz, sxz = sums
    sc = 1.0 / float(N)
    center = [sx * sc, sy * sc, sz * sc]
    K = [[sxx - sx * sx * sc, sxy - sx * sy * sc, sxz - sx * sz * sc], [0.0, syy - sy * sy * sc, syz - sy * sz * sc], [0.0, 0.0, szz - sz * sz * sc]]
    K[1][0] = K[0][1]
    K[2][0] = K[0][2]
    K[2][1] = K[1][2]
    sv, V = eig(K)
    if V[0][0] * center[0] + V[1][0] * center[1] + V[2][0] * center[2] <= 0:
        normal = [V[0][0], V[1][0], V[2][0]]
    else:
        normal = [-V[0][0], -V[1][0], -V[2][0]]
    mse = sv[0] * sc
    curvature = sv[0] / (sv[0] + sv[1] + sv[2])
    return center, normal, mse, curvature


FLAG_MISSING, FLAG_DISCONTINUITY = 1, 2      # bits of a block record's flag; 0: the block holds window * window points


def _record(flag, sums, N, eig):
    if flag or N < 4:
        return dict(flag=flag, N=0, sums=[0.0] * 9, center=[0.0] * 3, normal=[0.0] * 3, mse=NAN, curvature=NAN)
    center, normal, mse, curvature = fit(sums, N, eig)
    return dict(flag=0, N=N, sums=list(sums), center=center, normal=normal, mse=mse, curvature=curvature)


# ---- step 2, first half: the block constructor, AHCPlaneSeg.hpp:211-285, literally.  A block is rejected by its first offending pixel; which one it is does
# not matter (the flag says what the WHOLE block holds: any invalid pixel, any discontinuity of a valid pixel), so the loops below do not stop early.
def block_records(c, depth, eig=eig3_jacobi):
    W, H, w = c.width, c.height, c.window
    Nh, Nw = H // w, W // w
    out = []
    for bi in range(Nh):
        for bj in range(Nw):
            flag = 0
            sums = [0.0] * 9
            N = 0
            for i in range(bi * w, bi * w + w):
                for j in range(bj * w, bj * w + w):
                    d = float(depth[i, j])
                    if not pixel_valid(c, d):
                        flag |= FLAG_MISSING
                        continue
                    x, y, z = pixel_point(c, i, j, d)
                    if j + 1 < W:
                        zn = float(depth[i, j + 1])
                        if pixel_valid(c, zn) and abs(z - zn) > t_dz(c, z):
                            flag |= FLAG_DISCONTINUITY
                    if i + 1 < H:
                        zn = float(depth[i + 1, j])
                        if pixel_valid(c, zn) and abs(z - zn) > t_dz(c, z):
                            flag |= FLAG_DISCONTINUITY
                    sums[0] += x
                    sums[1] += y
                    sums[2] += z
                    sums[3] += x * x
                    sums[4] += y * y
                    sums[5] += z * z
                    sums[6] += x * y
                    sums[7] += y * z
                    sums[8] += x * z
                    N += 1
            out.append(_record(flag, sums, N, eig))
    return out


def cloud_vec(c, depth):
    """(valid (H, W) bool, x, y, z (H, W) float64) with pixel_point's operations, whole image at a time"""
    d = depth.astype(np.float64)
    with np.errstate(invalid="ignore"):
        valid = ~(np.isnan(d) | (d > c.depth_max) | (d < c.depth_min))
    n = np.arange(c.width, dtype=np.float64)[None, :]
    m = np.arange(c.height, dtype=np.float64)[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        x = (n - float(c.cx)) * d / float(c.fx)
        y = (m - float(c.cy)) * d / float(c.fy)
    return valid, x, y, d


def block_records_vec(c, depth, eig=eig3_jacobi):
    """block_records with the hundred additions of a sum in the same order, every block at once"""
    W, H, w = c.width, c.height, c.window
    Nh, Nw = H // w, W // w
    valid, x, y, z = cloud_vec(c, depth)
    with np.errstate(invalid="ignore"):
        tz = c.depth_alpha * np.abs(z) + c.depth_change_tol
        disc = np.zeros((H, W), bool)
        disc[:, :-1] |= valid[:, :-1] & valid[:, 1:] & (np.abs(z[:, :-1] - z[:, 1:]) > tz[:, :-1])
        disc[:-1, :] |= valid[:-1, :] & valid[1:, :] & (np.abs(z[:-1, :] - z[1:, :]) > tz[:-1, :])

    def blocks(a):
        return a[:Nh * w, :Nw * w].reshape(Nh, w, Nw, w)
    missing = (~blocks(valid)).any(axis=(1, 3))
    discont = blocks(disc).any(axis=(1, 3))
    flag = missing * FLAG_MISSING + discont * FLAG_DISCONTINUITY
    bx, by, bz = blocks(x), blocks(y), blocks(z)
    S = np.zeros((9, Nh, Nw))
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(w):
            for j in range(w):
                px, py, pz = bx[:, i, :, j], by[:, i, :, j], bz[:, i, :, j]
                S[0] += px
                S[1] += py
                S[2] += pz
                S[3] += px * px
                S[4] += py * py
                S[5] += pz * pz
                S[6] += px * py
                S[7] += py * pz
                S[8] += px * pz
    out = []
    for bi in range(Nh):
        for bj in range(Nw):
            out.append(_record(int(flag[bi, bj]), [float(S[k, bi, bj]) for k in range(9)], w * w, eig))
    return out


# ---- DisjointSet.hpp
class DisjointSet:
    def __init__(self, n):
        self.parent = list(range(n))
        self.size = [1] * n

    def find(self, x):
        r = x
        while self.parent[r] != r:
            r = self.parent[r]
        while self.parent[x] != r:
            self.parent[x], x = r, self.parent[x]
        return r

    def set_size(self, x):
        return self.size[self.find(x)]

    def union(self, x, y):
        xr, yr = self.find(x), self.find(y)
        if xr == yr:
            return xr
        if self.size[xr] < self.size[yr]:
            self.parent[xr] = yr
            self.size[yr] += self.size[xr]
            return yr
        self.parent[yr] = xr
        self.size[xr] += self.size[yr]
        return xr


def _similarity(a, b):
    return abs(a.normal[0] * b.normal[0] + a.normal[1] * b.normal[1] + a.normal[2] * b.normal[2])


class Segmenter:
    """steps 2 (edges) to 4 over block records; nodes[] is the creation sequence"""

    def __init__(self, c, depth, records, eig=eig3_jacobi):
        self.c, self.depth, self.eig = c, depth, eig
        self.Nh, self.Nw = c.height // c.window, c.width // c.window
        self.ds = DisjointSet(self.Nh * self.Nw)
        self.nodes = []
        self.queue = []          # (mse, node index), a list kept as a set: the minimum is looked up
        self.extracted = []
        self.merges = []         # (rid of p, rid of the neighbour, N of the merged node), in order
        self.init_graph(records)

    def new_node(self, **kw):
        n = SimpleNamespace(nouse=False, nbs=set(), id=len(self.nodes), **kw)
        self.nodes.append(n)
        return n

    def connect(self, a, b):
        a.nbs.add(b.id)
        b.nbs.add(a.id)

    def disconnect_all(self, a):
        for k in a.nbs:
            self.nodes[k].nbs.discard(a.id)
        a.nbs = set()

    # initGraph :784-953
    def init_graph(self, records):
        c, Nh, Nw = self.c, self.Nh, self.Nw
        G = [None] * (Nh * Nw)
        for b, r in enumerate(records):
            if r["flag"] == 0 and r["mse"] < t_mse_init(c, r["center"][2]):
                G[b] = self.new_node(rid=b, N=r["N"], sums=list(r["sums"]), center=list(r["center"]), normal=list(r["normal"]), mse=r["mse"], curvature=r["curvature"])
                self.queue.append((r["mse"], G[b].id))
        self.n_initial = len(self.nodes)
        for i in range(Nh):
            j = 1
            while j < Nw:
                cidx = i * Nw + j
                if G[cidx - 1] is None:
                    j -= 1
                elif G[cidx] is None:
                    pass
                elif j < Nw - 1 and G[cidx + 1] is None:
                    j += 1
                else:
                    th = t_ang_init(c, G[cidx].center[2])
                    if (j < Nw - 1 and _similarity(G[cidx - 1], G[cidx + 1]) >= th) or (j == Nw - 1 and _similarity(G[cidx], G[cidx - 1]) >= th):
                        self.connect(G[cidx], G[cidx - 1])
                        if j < Nw - 1:
                            self.connect(G[cidx], G[cidx + 1])
                    else:
                        j -= 1
                j += 2
        for j in range(Nw):
            i = 1
            while i < Nh:
                cidx = i * Nw + j
                if G[cidx - Nw] is None:
                    i -= 1
                elif G[cidx] is None:
                    pass
                elif i < Nh - 1 and G[cidx + Nw] is None:
                    i += 1
                else:
                    th = t_ang_init(c, G[cidx].center[2])
                    if (i < Nh - 1 and _similarity(G[cidx - Nw], G[cidx + Nw]) >= th) or (i == Nh - 1 and _similarity(G[cidx], G[cidx - Nw]) >= th):
                        self.connect(G[cidx], G[cidx - Nw])
                        if i < Nh - 1:
                            self.connect(G[cidx], G[cidx + Nw])
                    else:
                        i -= 1
                i += 2
        self.n_edges = sum(len(n.nbs) for n in self.nodes) // 2

    def merged(self, pa, pb):
        sums = [a + b for a, b in zip(pa.sums, pb.sums)]
        N = pa.N + pb.N
        center, normal, mse, curvature = fit(sums, N, self.eig)
        return dict(rid=pa.rid if pa.N >= pb.N else pb.rid, N=N, sums=sums, center=center, normal=normal, mse=mse, curvature=curvature)

    # ahCluster :981-1187
    def cluster(self):
        c = self.c
        step = 0
        while self.queue and step <= c.max_step:
            top = min(self.queue)
            self.queue.remove(top)
            p = self.nodes[top[1]]
            if p.nouse:
                continue
            cand, cand_nb = None, None
            for k in sorted(p.nbs):
                nb = self.nodes[k]
                if _similarity(p, nb) < c.similarity_merge:
                    continue
                m = self.merged(p, nb)
                if cand is None or cand["mse"] > m["mse"] or (cand["mse"] == m["mse"] and cand["N"] < m["mse"]):
                    cand, cand_nb = m, nb
            if cand is not None and cand["mse"] < t_mse_merge(c, cand["center"][2]):
                n = self.new_node(**cand)
                self.queue.append((n.mse, n.id))
                self.merges.append((p.rid, cand_nb.rid, n.N))
                self.ds.union(p.rid, cand_nb.rid)
                n.nbs = (p.nbs | cand_nb.nbs) - {p.id, cand_nb.id}
                self.disconnect_all(p)
                self.disconnect_all(cand_nb)
                for k in n.nbs:
                    self.nodes[k].nbs.add(n.id)
                p.nouse = cand_nb.nouse = True
            else:
                if p.N >= c.min_support:
                    self.extracted.append(p)
                self.disconnect_all(p)
            step += 1
        while self.queue:
            top = min(self.queue)
            self.queue.remove(top)
            p = self.nodes[top[1]]
            if p.N >= c.min_support:
                self.extracted.append(p)
            self.disconnect_all(p)
        self.extracted.sort(key=lambda n: -n.N)      # stable
        return step

    # findBlockMembership :483-585
    def block_membership(self):
        c, Nh, Nw, w, W = self.c, self.Nh, self.Nw, self.c.window, self.c.width
        ds = self.ds
        rid2plid = {}
        for plid, p in enumerate(self.extracted):
            rid2plid.setdefault(p.rid, plid)
        self.trail = np.full(c.width * c.height, -1, np.int32)
        img = self.trail.reshape(c.height, c.width)
        self.blk_map = [0] * (Nh * Nw)
        self.valid_plane = [False] * len(self.extracted)
        self.rf = []
        blk = self.blk_map
        for i in range(Nh):
            for j in range(Nw):
                blkid = i * Nw + j
                setid = ds.find(blkid)
                if ds.set_size(setid) * w * w >= c.min_support:
                    nbs = []
                    if j > 0:
                        nbs.append(blkid - 1)
                    if j < Nw - 1:
                        nbs.append(blkid + 1)
                    if i > 0:
                        nbs.append(blkid - Nw)
                    if i < Nh - 1:
                        nbs.append(blkid + Nw)
                    same = all(ds.find(k) == setid for k in nbs)
                    plid = rid2plid.setdefault(setid, 0)
                    if same:
                        blk[blkid] = plid
                        img[i * w:(i + 1) * w, j * w:(j + 1) * w] = plid
                        self.valid_plane[plid] = True
                    else:
                        blk[blkid] = -1
                else:
                    blk[blkid] = -1
                if blk[blkid] < 0:
                    if i > 0 and blk[blkid - Nw] >= 0:
                        s = (i * w - 1) * W + j * w
                        for k in range(1, w):
                            self.rf.append((s + k, blk[blkid - Nw]))
                    if j > 0 and blk[blkid - 1] >= 0:
                        s = (i * w) * W + j * w - 1
                        for k in range(w - 1):
                            self.rf.append((s + k * W, blk[blkid - 1]))
                else:
                    plid = blk[blkid]
                    if i > 0 and blk[blkid - Nw] != plid:
                        s = (i * w) * W + j * w
                        for k in range(w - 1):
                            self.rf.append((s + k, plid))
                    if j > 0 and blk[blkid - 1] != plid:
                        s = (i * w) * W + j * w
                        for k in range(1, w):
                            self.rf.append((s + k * W, plid))
        self.n_seeds = len(self.rf)

    # floodFill :426-474
    def flood_fill(self):
        c, W, H, w, Nw, Nh = self.c, self.c.width, self.c.height, self.c.window, self.Nw, self.Nh
        trail, blk, rf, depth = self.trail, self.blk_map, self.rf, self.depth
        dist = np.full(W * H, FLT_MAX, np.float32)
        self.connects = []
        self.n_stopped = 0          # neighbours met at trail <= -6
        self.n_retaken = 0          # pixels claimed by a plane and taken by a nearer one
        k = 0
        while k < len(rf):
            s, plid = rf[k]
            k += 1
            sy = s // W
            sx = s - sy * W
            pl = self.extracted[plid]
            nbs = []
            if sx > 0:
                nbs.append(s - 1)
            if sx < W - 1:
                nbs.append(s + 1)
            if sy > 0:
                nbs.append(s - W)
            if sy < H - 1:
                nbs.append(s + W)
            for ci in nbs:
                t = int(trail[ci])
                if t <= TRAIL_STOP:
                    self.n_stopped += 1
                    continue
                if t >= 0 and t == plid:
                    continue
                cy = ci // W
                cx = ci - cy * W
                by, bx = cy // w, cx // w
                if by < Nh and bx < Nw and blk[by * Nw + bx] >= 0:
                    continue
                d = float(depth[cy, cx])
                near = False
                if pixel_valid(c, d):
                    x, y, z = pixel_point(c, cy, cx, d)
                    sd = pl.normal[0] * (x - pl.center[0]) + pl.normal[1] * (y - pl.center[1]) + pl.normal[2] * (z - pl.center[2])
                    cdist = F32(abs(sd))
                    cd = float(cdist)
                    near = cd * cd < DIST_FACTOR * pl.mse + DIST_EPS
                if near:
                    if t >= 0:
                        npl = self.extracted[t]
                        if _similarity(pl, npl) >= c.similarity_refine:
                            self.connect(npl, pl)
                            self.connects.append((t, plid))
                    if cdist < dist[ci]:
                        if t >= 0:
                            self.n_retaken += 1
                        trail[ci] = plid
                        dist[ci] = cdist
                        rf.append((ci, plid))
                    elif t < 0:
                        trail[ci] = t - 1
                elif t < 0:
                    trail[ci] = t - 1

    # refineDetails :297-377
    def refine(self):
        self.block_membership()
        self.flood_fill()
        old = self.extracted
        self.old = old
        self.extracted = []
        self.queue = [(p.mse, p.id) for i, p in enumerate(old) if self.valid_plane[i]]
        self.n_merges_first = len(self.merges)
        self.cluster()
        self.plidmap = [-1] * len(old)
        for i, op in enumerate(old):
            if not self.valid_plane[i]:
                continue
            rid = self.ds.find(op.rid)
            for j, fp in enumerate(self.extracted):
                if rid == fp.rid:
                    self.plidmap[i] = j
                    break
        claimed = sorted(set(p for p, _ in self.rf[self.n_seeds:]))
        self.claims = [(p, int(self.trail[p])) for p in claimed]
        t = self.trail
        pm = np.array(self.plidmap + [-1], np.int32)
        self.membership = np.where(t >= 0, pm[np.where(t >= 0, t, -1)], -1).astype(np.int32).reshape(self.c.height, self.c.width)


# ---- pcl::VoxelGrid of PCL 1.8 (voxel_grid.hpp, applyFilter) for an all-finite cloud; pts (n, 3) float32 in ascending pixel index
def voxel_grid(pts, leaf):
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
    inv = F32(1.0) / F32(leaf)
    mn, mx = pts.min(axis=0), pts.max(axis=0)
    min_b = np.floor(mn * inv).astype(np.int64)
    max_b = np.floor(mx * inv).astype(np.int64)
    div = max_b - min_b + 1
    if int(div[0]) * int(div[1]) * int(div[2]) > INT_MAX:
        raise ValueError("voxel grid too fine")
    ijk = np.floor(pts * inv).astype(np.int64) - min_b
    key = ijk[:, 0] + ijk[:, 1] * div[0] + ijk[:, 2] * div[0] * div[1]
    order = np.argsort(key, kind="stable")
    return pts, key, order, dict(min_b=min_b, div=div)


def voxel_centroids(pts, leaf):
    """literal: one float addition per line of the sum, voxel by voxel"""
    pts, key, order, grid = voxel_grid(pts, leaf)
    out = []
    i, n = 0, len(order)
    while i < n:
        j = i
        sx, sy, sz = F32(0), F32(0), F32(0)
        while j < n and key[order[j]] == key[order[i]]:
            p = pts[order[j]]
            sx = F32(sx + p[0])
            sy = F32(sy + p[1])
            sz = F32(sz + p[2])
            j += 1
        cnt = F32(j - i)
        out.append((F32(sx / cnt), F32(sy / cnt), F32(sz / cnt)))
        i = j
    return np.array(out, np.float32).reshape(-1, 3)


def voxel_centroids_vec(pts, leaf):
    """the same additions in the same order, every voxel at once: round r adds the r-th point of each voxel that has one"""
    pts, key, order, grid = voxel_grid(pts, leaf)
    ks = key[order]
    head = np.ones(len(ks), bool)
    head[1:] = ks[1:] != ks[:-1]
    start = np.flatnonzero(head)
    count = np.diff(np.append(start, len(ks)))
    acc = np.zeros((len(start), 3), np.float32)
    sp = pts[order]
    for r in range(int(count.max())):
        live = np.flatnonzero(count > r)
        acc[live] = acc[live] + sp[start[live] + r]
    return (acc / count.astype(np.float32)[:, None]).astype(np.float32)


# ---- step 5: src/Frame.cc:411-456, :349-371
def plane_not_seen(accepted, coef):
    for pM in accepted:
        d = F32(pM[3] - coef[3])
        angle = F32(F32(F32(pM[0] * coef[0]) + F32(pM[1] * coef[1])) + F32(pM[2] * coef[2]))
        if float(d) > SEEN_DIST or float(d) < -SEEN_DIST:
            continue
        if float(angle) < SEEN_ANGLE and float(angle) > -SEEN_ANGLE:
            continue
        return False
    return True


def plane_points(c, depth, pix, vectorised):
    """float points of the pixels `pix` (ascending), src/Frame.cc:416-424"""
    if vectorised:
        _, x, y, z = cloud_vec(c, depth)
        return np.stack([x.reshape(-1)[pix], y.reshape(-1)[pix], z.reshape(-1)[pix]], axis=1).astype(np.float32)
    out = np.zeros((len(pix), 3), np.float32)
    for k, p in enumerate(pix):
        m = int(p) // c.width
        n = int(p) - m * c.width
        x, y, z = pixel_point(c, m, n, float(depth[m, n]))
        out[k] = (F32(x), F32(y), F32(z))
    return out


def run(c, depth, eig="jacobi", vectorised=False, records=None):
    """the whole function.  records: block records to start from (the replay of a device's own) instead of computing them"""
    depth = np.ascontiguousarray(depth, np.float32)
    assert depth.shape == (c.height, c.width)
    e = EIG[eig]
    if records is None:
        records = (block_records_vec if vectorised else block_records)(c, depth, e)
    sg = Segmenter(c, depth, records, e)
    sg.cluster()
    sg.refine()
    planes, accepted = [], []
    flat = sg.membership.reshape(-1)
    centroids = voxel_centroids_vec if vectorised else voxel_centroids
    for j, p in enumerate(sg.extracted):
        pix = np.flatnonzero(flat == j)
        nx, ny, nz = p.normal
        d = F32(-(nx * p.center[0] + ny * p.center[1] + nz * p.center[2]))
        coef = np.array([F32(nx), F32(ny), F32(nz), d], np.float32)
        if coef[3] < 0:
            coef = -coef
        cloud = centroids(plane_points(c, depth, pix, vectorised), c.leaf)
        kept = plane_not_seen(accepted, coef)
        if kept:
            accepted.append(coef)
        planes.append(dict(normal=list(p.normal), center=list(p.center), mse=p.mse, curvature=p.curvature, N=p.N, rid=p.rid, coef=coef, kept=kept,
                           flipped=bool(d < 0), n_pixels=len(pix), cloud=cloud))
    return dict(records=records, seg=sg, planes=planes, membership=sg.membership, blk_map=np.array(sg.blk_map, np.int32),
                claims=np.array(sg.claims, np.int32).reshape(-1, 2), plidmap=np.array(sg.plidmap, np.int32), merges=list(sg.merges))


def records_array(records):
    """block records as the (n, 18) float64 table the device returns: flag, N, nine sums, centre, normal, mse, curvature"""
    a = np.zeros((len(records), 18), np.float64)
    for k, r in enumerate(records):
        a[k, 0:1].view(np.int32)[:] = (r["flag"], r["N"])
        a[k, 1:10] = r["sums"]
        a[k, 10:13] = r["center"]
        a[k, 13:16] = r["normal"]
        a[k, 16] = r["mse"]
        a[k, 17] = r["curvature"]
    return a


def records_from_array(a):
    out = []
    for row in np.ascontiguousarray(a, np.float64).reshape(-1, 18):
        flag, N = (int(v) for v in row[0:1].view(np.int32))
        out.append(dict(flag=flag, N=N, sums=[float(v) for v in row[1:10]], center=[float(v) for v in row[10:13]], normal=[float(v) for v in row[13:16]],
                        mse=float(row[16]), curvature=float(row[17])))
    return out


# ---- the forms tools/plane_segmentation_walk.cpp reads and prints
def scene_bytes(c, depth):
    import struct
    head = struct.pack("<ii4f3if13d", c.width, c.height, float(c.fx), float(c.fy), float(c.cx), float(c.cy), c.window, c.min_support, c.max_step, float(c.leaf),
                       c.depth_min, c.depth_max, c.depth_sigma, c.std_tol_init, c.std_tol_merge, c.z_near, c.z_far, c.angle_near, c.angle_far, c.similarity_merge,
                       c.similarity_refine, c.depth_alpha, c.depth_change_tol)
    assert len(head) == 144
    return head + np.ascontiguousarray(depth, np.float32).tobytes()


def _hex64(v):
    return "%016x" % int(np.array([v], np.float64).view(np.uint64)[0])


def _hex32(v):
    return "%08x" % int(np.array([v], np.float32).view(np.uint32)[0])


def script_text(r):
    """what `walk script` prints for the scene whose run() gave r"""
    sg = r["seg"]
    out = ["blocks %d" % len(r["records"])]
    for b in r["records"]:
        out.append(" ".join(["%d %d" % (b["flag"], b["N"])] + [_hex64(v) for v in b["sums"] + b["center"] + b["normal"] + [b["mse"], b["curvature"]]]))
    out.append("graph %d %d" % (sg.n_initial, sg.n_edges))
    out.append("merges %d %d" % (len(sg.merges), sg.n_merges_first))
    out += ["%d %d %d" % m for m in sg.merges]
    out.append("fill %d %d %d %d" % (sg.n_seeds, len(sg.connects), sg.n_stopped, sg.n_retaken))
    out.append(" ".join(["blkmap"] + [str(v) for v in sg.blk_map]))
    out.append(" ".join(["plidmap"] + [str(v) for v in sg.plidmap]))
    out.append(" ".join(["claims %d" % len(sg.claims)] + ["%d %d" % c for c in sg.claims]))
    out.append("planes %d" % len(r["planes"]))
    for p in r["planes"]:
        out.append(" ".join([_hex64(v) for v in p["normal"] + p["center"] + [p["mse"], p["curvature"]]] + ["%d %d" % (p["N"], p["rid"])] + [_hex32(v) for v in p["coef"]]
                            + ["%d" % p["kept"]]))
    for k, p in enumerate(r["planes"]):
        out.append(" ".join(["cloud %d %d %d" % (k, p["n_pixels"], len(p["cloud"]))] + [_hex32(v) for v in p["cloud"].reshape(-1)]))
    return "\n".join(out) + "\n"


def result_arrays(r):
    """a run() result as plain arrays: what the device's read-backs are compared with and what tests/golden/plane_segmentation holds"""
    P = r["planes"]
    clouds = [p["cloud"].reshape(-1, 3) for p in P]
    return dict(
        records=records_array(r["records"]), membership=r["membership"].astype(np.int32), blk_map=r["blk_map"], plidmap=r["plidmap"], claims=r["claims"],
        normal=np.array([p["normal"] for p in P], np.float64).reshape(-1, 3), center=np.array([p["center"] for p in P], np.float64).reshape(-1, 3),
        mse=np.array([p["mse"] for p in P], np.float64), curvature=np.array([p["curvature"] for p in P], np.float64),
        N=np.array([p["N"] for p in P], np.int32), rid=np.array([p["rid"] for p in P], np.int32),
        coef=np.array([p["coef"] for p in P], np.float32).reshape(-1, 4), kept=np.array([p["kept"] for p in P], np.uint8),
        n_pixels=np.array([p["n_pixels"] for p in P], np.int32), cloud_count=np.array([len(c) for c in clouds], np.int32),
        clouds=np.concatenate(clouds + [np.zeros((0, 3), np.float32)]).astype(np.float32))


BULK = ("records", "membership", "claims", "clouds")      # at VGA the golden files hold a SHA-256 of these instead


def digest(a):
    import hashlib
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8).copy()


def cluster_graph(c, nodes, edges, eig=eig3_jacobi):
    """ahCluster alone over hand-built nodes [(rid, N, nine sums)] in creation order and edges [(a, b)] of node indices: what `walk cluster` runs.
    Returns (steps, merges, [(node index, rid, N, mse) of the extracted planes in their final order])."""
    sg = Segmenter.__new__(Segmenter)
    sg.c, sg.eig, sg.nodes, sg.queue, sg.extracted, sg.merges = c, eig, [], [], [], []
    sg.ds = DisjointSet(max(n[0] for n in nodes) + 1)
    for rid, N, sums in nodes:
        center, normal, mse, curvature = fit(sums, N, eig)
        n = sg.new_node(rid=rid, N=N, sums=list(sums), center=center, normal=normal, mse=mse, curvature=curvature)
        if mse == mse:
            sg.queue.append((mse, n.id))
    for a, b in edges:
        sg.connect(sg.nodes[a], sg.nodes[b])
    steps = sg.cluster()
    return steps, list(sg.merges), [(n.id, n.rid, n.N, n.mse) for n in sg.extracted]


def graph_text(nodes, edges, min_support):
    out = ["min_support %d" % min_support]
    out += ["node %d %d %s" % (rid, N, " ".join(_hex64(v) for v in sums)) for rid, N, sums in nodes]
    out += ["edge %d %d" % e for e in edges]
    return "\n".join(out) + "\n"


def cluster_text(res):
    steps, merges, extracted = res
    out = ["steps %d" % steps, "merges %d" % len(merges)] + ["%d %d %d" % m for m in merges] + ["extracted %d" % len(extracted)]
    out += ["%d %d %d %s" % (i, rid, N, _hex64(mse)) for i, rid, N, mse in extracted]
    return "\n".join(out) + "\n"


def sums_of(points):
    """the nine sums of a list of (x, y, z), pushed in order (Stats::push, AHCPlaneSeg.hpp:82-87)"""
    s = [0.0] * 9
    for x, y, z in points:
        s[0] += x
        s[1] += y
        s[2] += z
        s[3] += x * x
        s[4] += y * y
        s[5] += z * z
        s[6] += x * y
        s[7] += y * z
        s[8] += x * z
    return s
