"""Initializer (reference src/Initializer.cc): the homography / fundamental RANSAC and the two-view reconstruction of
Tracking::MonocularInitialization through eao_initializer_initialize (csrc/initializer.hip).

prob: keys1 (n1,2) / keys2 (n2,2) f32 undistorted keypoints, matches12 (N,2) i32 pairs (first, second) ascending in first, K (fx, fy, cx, cy),
sigma, min_parallax, min_triangulated.  sets: (iterations, 8) indices into 0 .. N-1 in draw order (draw_sets restates the loop)."""
import ctypes as C

import numpy as np

from . import _lib

BRANCH_H, BRANCH_F = 0, 1
MAX_MOTIONS = 8


def pairs_of(vMatches12):
    """mvMatches12 of Initializer::Initialize (:49-63): (i, vMatches12[i]) for every i with a match."""
    v = np.asarray(vMatches12, np.int64)
    i = np.nonzero(v >= 0)[0]
    return np.stack([i, v[i]], 1).astype(np.int32)


def draw_sets(n, iterations, random_int):
    """The draw loop of :78-97 over random_int(lo, hi) (DUtils::Random::RandomInt after SeedRandOnce(0)), with its swap-with-back removal."""
    sets = np.zeros((iterations, 8), np.int32)
    for it in range(iterations):
        avail = list(range(n))
        for j in range(8):
            randi = random_int(0, len(avail) - 1)
            sets[it, j] = avail[randi]
            avail[randi] = avail[-1]
            avail.pop()
    return sets


def initialize(prob, sets, inspect=False):
    """Initializer::Initialize after its draws.  Returns dict(returned, branch, no_model, degenerate, SH, SF, RH, best_h, best_f, H21 (3,3), F21 (3,3), R21 (3,3),
    t21 (3,), parallax, cos_parallax, n_good, motion, n_motions, n_inliers, p3d (n1,3), triangulated (n1,)) and, with inspect, hyp_H21 / hyp_H12 / hyp_F21
    (iterations,3,3), hyp_SH / hyp_SF (iterations,), hyp_inlier_H / hyp_inlier_F (iterations,N), inlier (N,), mot_R (8,3,3), mot_t (8,3), mot_n_good (8,),
    mot_cos (8,), mot_good (8,n1), mot_p3d (8,n1,3)."""
    k1 = np.ascontiguousarray(prob["keys1"], np.float32).reshape(-1, 2)
    k2 = np.ascontiguousarray(prob["keys2"], np.float32).reshape(-1, 2)
    m12 = np.ascontiguousarray(prob["matches12"], np.int32).reshape(-1, 2)
    sets = np.ascontiguousarray(sets, np.int32).reshape(-1, 8)
    n1, n2, N, it = len(k1), len(k2), len(m12), len(sets)
    P, R = _lib.InitializerProblem(), _lib.InitializerResult()
    P.n1, P.n2, P.keys1_xy, P.keys2_xy, P.n_matches, P.matches12 = n1, n2, _lib.ptr(k1), _lib.ptr(k2), N, _lib.ptr(m12)
    P.fx, P.fy, P.cx, P.cy = [float(v) for v in prob["K"]]
    P.sigma, P.min_parallax, P.min_triangulated = float(prob.get("sigma", 1.0)), float(prob.get("min_parallax", 1.0)), int(prob.get("min_triangulated", 50))
    keep = dict(p3d=np.zeros((max(n1, 1), 3), np.float32), triangulated=np.zeros(max(n1, 1), np.uint8))
    if inspect:
        keep.update(hyp_H21=np.zeros((max(it, 1), 3, 3), np.float32), hyp_H12=np.zeros((max(it, 1), 3, 3), np.float32), hyp_F21=np.zeros((max(it, 1), 3, 3), np.float32),
                    hyp_SH=np.zeros(max(it, 1), np.float32), hyp_SF=np.zeros(max(it, 1), np.float32),
                    hyp_inlier_H=np.zeros((max(it, 1), max(N, 1)), np.uint8), hyp_inlier_F=np.zeros((max(it, 1), max(N, 1)), np.uint8), inlier=np.zeros(max(N, 1), np.uint8),
                    mot_R=np.zeros((MAX_MOTIONS, 3, 3), np.float32), mot_t=np.zeros((MAX_MOTIONS, 3), np.float32), mot_n_good=np.zeros(MAX_MOTIONS, np.int32),
                    mot_cos=np.zeros(MAX_MOTIONS, np.float32), mot_good=np.zeros((MAX_MOTIONS, max(n1, 1)), np.uint8), mot_p3d=np.zeros((MAX_MOTIONS, max(n1, 1), 3), np.float32))
    for k, a in keep.items():
        setattr(R, k, _lib.ptr(a))
    _lib.check(_lib.load().eao_initializer_initialize(C.byref(P), _lib.ptr(sets), it, C.byref(R)))
    out = dict(returned=bool(R.returned), branch=int(R.branch), no_model=bool(R.no_model), degenerate=bool(R.degenerate), SH=np.float32(R.SH), SF=np.float32(R.SF),
               RH=np.float32(R.RH), best_h=int(R.best_h), best_f=int(R.best_f), H21=np.array(R.H21[:], np.float32).reshape(3, 3),
               F21=np.array(R.F21[:], np.float32).reshape(3, 3), R21=np.array(R.R21[:], np.float32).reshape(3, 3), t21=np.array(R.t21[:], np.float32),
               parallax=np.float32(R.parallax), cos_parallax=np.float32(R.cos_parallax), n_good=int(R.n_good), motion=int(R.motion), n_motions=int(R.n_motions),
               n_inliers=int(R.n_inliers))
    out.update(keep)
    return out
