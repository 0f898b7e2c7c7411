"""numpy yardstick of the triangulation loop of LocalMapping::CreateNewMapPoints (reference src/LocalMapping.cc:288-454, KeyFrame::UnprojectStereo
src/KeyFrame.cc:654-670), written from the reference text and vectorised over the pairs of one neighbour (every pair is independent).

Arithmetic, decided once and shared with the kernel:
  * float32 expressions are evaluated operation by operation in float32 (numpy float32 arrays; no fused multiply-add);
  * a cv::Mat product, Mat::dot and cv::norm accumulate the exact float products in float64 in storage order and round once;
  * x3D / w multiplies by 1. / w in float64 and rounds once; invz = 1.0 / z is a float64 division rounded to float32;
  * cos(2 * atan2(mb / 2, depth)) in float64, rounded to float32;
  * 5.991 * sigma2 and 7.8 * sigma2 are float64 products compared against the float32 sum; cosParallaxRays < 0.9998 is a float64 comparison;
  * comparisons are written as upstream writes them, so a NaN falls through the same gates.
point_and_branch() is the branch choice and the point; gates_after_point() restates everything from z1 on and takes ANY point -- the GPU test replays the
device's own points through it.  Two SVD variants: float64 eigh of A^T A ("eigh") and a float32 one-sided Jacobi on A as OpenCV's JacobiSVD runs it ("jacobi32")."""
import numpy as np

f32, f64 = np.float32, np.float64

# ---- the loop's literals (tests/golden/triangulation_constants.json)
LOW_PARALLAX_COS = 0.9998      # src/LocalMapping.cc:323
CHI2_MONO = 5.991              # :378, :404
CHI2_STEREO = 7.8              # :389, :415
RATIO_FACTOR_BASE = 1.5        # :236  ratioFactor = 1.5f * mfScaleFactor
# ----

# eao_tri_verdict (include/eao_fusion.h)
EMPTY, TRIANGULATED, UNPROJECTED_1, UNPROJECTED_2, LOW_PARALLAX, W_ZERO, BEHIND_1, BEHIND_2, REPROJ_1, REPROJ_2, ZERO_DIST, SCALE, NO_DEPTH = range(13)
VERDICT_NAMES = ["EMPTY", "TRIANGULATED", "UNPROJECTED_1", "UNPROJECTED_2", "LOW_PARALLAX", "W_ZERO", "BEHIND_1", "BEHIND_2", "REPROJ_1", "REPROJ_2", "ZERO_DIST",
                 "SCALE", "NO_DEPTH"]
ACCEPTING = (TRIANGULATED, UNPROJECTED_1, UNPROJECTED_2)
HAS_POINT = (TRIANGULATED, UNPROJECTED_1, UNPROJECTED_2, BEHIND_1, BEHIND_2, REPROJ_1, REPROJ_2, ZERO_DIST, SCALE)
CAMERA_SCALARS = ("fx", "fy", "cx", "cy", "invfx", "invfy", "mb", "mbf")


def ratio_factor(scale_factor):
    """:236  1.5f * mfScaleFactor, a float32 product"""
    return f32(f32(RATIO_FACTOR_BASE) * f32(scale_factor))


def _cam(cam):
    c = {k: f32(cam[k]) for k in CAMERA_SCALARS}
    c["R"] = np.asarray(cam["Rcw"], f32).reshape(3, 3)
    c["t"] = np.asarray(cam["tcw"], f32).reshape(3)
    c["Ow"] = np.asarray(cam["Ow"], f32).reshape(3)
    return c


def _ddot3(a, b):
    """sum of three exact float products in float64, in storage order; a, b: sequences of three float32 arrays / scalars"""
    s = np.asarray(a[0], f64) * np.asarray(b[0], f64)
    s = s + np.asarray(a[1], f64) * np.asarray(b[1], f64)
    s = s + np.asarray(a[2], f64) * np.asarray(b[2], f64)
    return s


def _gather(K1, K2, row):
    idx1 = np.nonzero(np.asarray(row) >= 0)[0]
    idx2 = np.asarray(row)[idx1]
    g = {"idx1": idx1, "idx2": idx2}
    for tag, K, idx in (("1", K1, idx1), ("2", K2, idx2)):
        g["kx" + tag] = np.asarray(K["kp_x"], f32)[idx]
        g["ky" + tag] = np.asarray(K["kp_y"], f32)[idx]
        g["ur" + tag] = np.asarray(K["u_right"], f32)[idx]
        g["o" + tag] = np.asarray(K["kp_octave"], np.int64)[idx]
        g["depth" + tag] = np.asarray(K["depth"], f32)[idx]
        g["rawx" + tag] = np.asarray(K["raw_x"] if K.get("raw_x") is not None else K["kp_x"], f32)[idx]
        g["rawy" + tag] = np.asarray(K["raw_y"] if K.get("raw_y") is not None else K["kp_y"], f32)[idx]
        g["s2" + tag] = np.asarray(K["level_sigma2"], f32)[g["o" + tag]]
        g["sf" + tag] = np.asarray(K["scale_factors"], f32)[g["o" + tag]]
    return g


def _smallest_right_singular_vector_eigh(A):
    """A: (N, 4, 4) float32.  Eigenvector of the smallest eigenvalue of A^T A (float64, from the float A), as float64 (N, 4)."""
    Ad = A.astype(f64)
    S = np.zeros((len(A), 4, 4), f64)
    for i in range(4):
        for k in range(4):
            s = Ad[:, 0, i] * Ad[:, 0, k]
            for r in range(1, 4):
                s = s + Ad[:, r, i] * Ad[:, r, k]
            S[:, i, k] = s
    bad = ~np.isfinite(S).all(axis=(1, 2))
    S[bad] = np.eye(4)
    _w, V = np.linalg.eigh(S)
    v = V[:, :, 0].copy()
    v[bad] = np.nan
    return v


def _smallest_right_singular_vector_jacobi32(A, sweeps=30):
    """One-sided Jacobi on the columns of A in float32 storage with float64 inner products, as OpenCV's JacobiSVDImpl_<float> rotates the rows of A^T and of V^T
    (modules/core/src/lapack.cpp): up to 30 sweeps, a pair is skipped when |p| <= eps * sqrt(a * b).  Returns the row of V^T of the smallest singular value."""
    N = len(A)
    At = np.ascontiguousarray(np.transpose(A, (0, 2, 1))).astype(f32)      # row i = column i of A
    Vt = np.tile(np.eye(4, dtype=f32), (N, 1, 1))
    eps = f64(np.finfo(f32).eps) * 10
    W = (At.astype(f64) ** 2).sum(axis=2)
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            for i in range(3):
                for j in range(i + 1, 4):
                    Ai, Aj = At[:, i, :], At[:, j, :]
                    a, b = W[:, i], W[:, j]
                    p = (Ai.astype(f64) * Aj.astype(f64)).sum(axis=1)
                    act = np.abs(p) > eps * np.sqrt(a * b)
                    p2 = p * 2
                    beta = a - b
                    gamma = np.hypot(p2, beta)
                    neg = beta < 0
                    delta = (gamma - beta) * 0.5
                    s_neg = np.sqrt(delta / gamma)
                    c_neg = p2 / (gamma * s_neg * 2)
                    c_pos = np.sqrt((gamma + beta) / (gamma * 2))
                    s_pos = p2 / (gamma * c_pos * 2)
                    c = np.where(act, np.where(neg, c_neg, c_pos), 1.0).astype(f32)[:, None]
                    s = np.where(act, np.where(neg, s_neg, s_pos), 0.0).astype(f32)[:, None]
                    t0 = c * Ai + s * Aj
                    t1 = -s * Ai + c * Aj
                    At[:, i, :], At[:, j, :] = t0, t1
                    W[:, i] = (t0.astype(f64) ** 2).sum(axis=1)
                    W[:, j] = (t1.astype(f64) ** 2).sum(axis=1)
                    Vi, Vj = Vt[:, i, :], Vt[:, j, :]
                    v0 = c * Vi + s * Vj
                    v1 = -s * Vi + c * Vj
                    Vt[:, i, :], Vt[:, j, :] = v0, v1
    k = np.argmin(np.where(np.isfinite(W), W, np.inf), axis=1)
    return Vt[np.arange(N), k, :].astype(f64)


SVD_VARIANTS = {"eigh": _smallest_right_singular_vector_eigh, "jacobi32": _smallest_right_singular_vector_jacobi32}


def _unproject(c, z, u, v):
    """KeyFrame::UnprojectStereo, for every pair (the caller masks z > 0)"""
    x = (u - c["cx"]) * z * c["invfx"]
    y = (v - c["cy"]) * z * c["invfy"]
    R, Ow = c["R"], c["Ow"]
    return np.stack([(_ddot3((R[0, i], R[1, i], R[2, i]), (x, y, z)) + f64(Ow[i])).astype(f32) for i in range(3)], axis=1)      # Rwc * x3Dc + Ow


def point_and_branch(K1, cam1, K2, cam2, row, svd="eigh"):
    """:295-353.  Per populated slot of `row` (in slot order): the branch taken -- TRIANGULATED / UNPROJECTED_1 / UNPROJECTED_2 (a point exists), or the verdict
    that ends the pair without one (LOW_PARALLAX, W_ZERO, NO_DEPTH) -- the point (zero where there is none), and the signed relative margins of the parallax
    comparisons that chose the branch (NaN where a comparison was not evaluated)."""
    g = _gather(K1, K2, row)
    c1, c2 = _cam(cam1), _cam(cam2)
    n = len(g["idx1"])
    st1, st2 = g["ur1"] >= 0, g["ur2"] >= 0
    with np.errstate(all="ignore"):
        xn1 = ((g["kx1"] - c1["cx"]) * c1["invfx"], (g["ky1"] - c1["cy"]) * c1["invfy"], np.ones(n, f32))
        xn2 = ((g["kx2"] - c2["cx"]) * c2["invfx"], (g["ky2"] - c2["cy"]) * c2["invfy"], np.ones(n, f32))
        ray1 = [_ddot3((c1["R"][0, i], c1["R"][1, i], c1["R"][2, i]), xn1).astype(f32) for i in range(3)]      # Rwc = Rcw.t()
        ray2 = [_ddot3((c2["R"][0, i], c2["R"][1, i], c2["R"][2, i]), xn2).astype(f32) for i in range(3)]
        cosR = (_ddot3(ray1, ray2) / (np.sqrt(_ddot3(ray1, ray1)) * np.sqrt(_ddot3(ray2, ray2)))).astype(f32)
        cps = cosR + f32(1)
        cs1 = np.cos(2.0 * np.arctan2(f64(c1["mb"] / f32(2)), g["depth1"].astype(f64))).astype(f32)
        cs2 = np.cos(2.0 * np.arctan2(f64(c2["mb"] / f32(2)), g["depth2"].astype(f64))).astype(f32)
        cps1 = np.where(st1, cs1, cps)
        cps2 = np.where(~st1 & st2, cs2, cps)      # `else if (bStereo2)`, :317
        cpsm = np.where(cps2 < cps1, cps2, cps1)      # std::min(cps1, cps2)
        tri = (cosR < cpsm) & (cosR > 0) & (st1 | st2 | (cosR.astype(f64) < LOW_PARALLAX_COS))
        un1 = ~tri & st1 & (cps1 < cps2)
        un2 = ~tri & ~un1 & st2 & (cps2 < cps1)
        branch = np.full(n, LOW_PARALLAX, np.int32)
        branch[tri], branch[un1], branch[un2] = TRIANGULATED, UNPROJECTED_1, UNPROJECTED_2
        X = np.zeros((n, 3), f32)
        # linear triangulation, :325-341
        T1 = np.concatenate([c1["R"], c1["t"][:, None]], axis=1)      # 3 x 4
        T2 = np.concatenate([c2["R"], c2["t"][:, None]], axis=1)
        A = np.zeros((n, 4, 4), f32)
        for k in range(4):
            A[:, 0, k] = xn1[0] * T1[2, k] - T1[0, k]
            A[:, 1, k] = xn1[1] * T1[2, k] - T1[1, k]
            A[:, 2, k] = xn2[0] * T2[2, k] - T2[0, k]
            A[:, 3, k] = xn2[1] * T2[2, k] - T2[1, k]
        if tri.any():
            vt = SVD_VARIANTS[svd](A[tri]).astype(f32)
            wz = vt[:, 3] == 0
            iw = 1.0 / vt[:, 3].astype(f64)
            Xt = (vt[:, :3].astype(f64) * iw[:, None]).astype(f32)
            Xt[wz] = 0
            X[tri] = Xt
            bt = branch[tri]
            bt[wz] = W_ZERO
            branch[tri] = bt
        for un, c, tag, code in ((un1, c1, "1", UNPROJECTED_1), (un2, c2, "2", UNPROJECTED_2)):
            if un.any():
                z = g["depth" + tag][un]
                ok = z > 0
                Xu = _unproject(c, z, g["rawx" + tag][un], g["rawy" + tag][un])
                Xu[~ok] = 0
                X[un] = Xu
                bu = branch[un]
                bu[~ok] = NO_DEPTH
                branch[un] = bu
        # signed relative margins of the comparisons of :323, :344, :348.  Two cosines near 1 are compared through 1 - cos, the quantity that carries the
        # parallax (a float32 cosine resolves 6e-8, which is 3e-4 of 1 - 0.9998), relative to the larger of the two sides.
        nanv = np.full(n, np.nan)

        def par(lhs, rhs):      # lhs < rhs between cosines
            a, b = 1.0 - np.asarray(lhs, f64), 1.0 - np.asarray(rhs, f64)
            return (a - b) / np.maximum(np.maximum(np.abs(a), np.abs(b)), np.finfo(f64).tiny)
        margins = np.stack([
            np.where(st1 | st2, par(cosR, cpsm), nanv),                                           # cosParallaxRays < cosParallaxStereo (monocular pairs: cos < cos + 1)
            cosR.astype(f64),                                                                     # cosParallaxRays > 0
            np.where(st1 | st2, nanv, par(cosR, LOW_PARALLAX_COS)),                               # cosParallaxRays < 0.9998 (monocular pairs)
            np.where(~tri & (st1 | st2), np.abs(par(cps1, cps2)), nanv),                          # cosParallaxStereo1 < cosParallaxStereo2 / the reverse
        ], axis=1)
    return dict(idx1=g["idx1"], idx2=g["idx2"], branch=branch, x3d=X, margins=margins, cosR=cosR)


GATE_NAMES = ["z1", "z2", "reproj1", "reproj2", "scale_low", "scale_high"]


def gates_after_point(K1, cam1, K2, cam2, row, ratio_factor_, X):
    """:355-435 in exact float32 / float64 steps, for ANY points X (n_pairs, 3) of the populated slots of `row` in slot order.  Returns (gate, margins): the code
    of the first gate that fires -- BEHIND_1, BEHIND_2, REPROJ_1, REPROJ_2, ZERO_DIST, SCALE -- or 0 where the pair passes all of them, and the signed relative
    margins of GATE_NAMES (positive = passes; NaN where upstream does not reach the gate)."""
    g = _gather(K1, K2, row)
    c1, c2 = _cam(cam1), _cam(cam2)
    X = np.asarray(X, f32).reshape(-1, 3)
    rf = f32(ratio_factor_)
    Xc = (X[:, 0], X[:, 1], X[:, 2])
    st1, st2 = g["ur1"] >= 0, g["ur2"] >= 0
    with np.errstate(all="ignore"):
        def cam_coord(c, r):
            return (_ddot3((c["R"][r, 0], c["R"][r, 1], c["R"][r, 2]), Xc) + f64(c["t"][r])).astype(f32)
        z1, z2 = cam_coord(c1, 2), cam_coord(c2, 2)

        def reproj(c, z, st, kx, ky, ur, s2):
            x, y = cam_coord(c, 0), cam_coord(c, 1)
            invz = (1.0 / z.astype(f64)).astype(f32)
            u = c["fx"] * x * invz + c["cx"]
            v = c["fy"] * y * invz + c["cy"]
            eX, eY = u - kx, v - ky
            u_r = u - c1["mbf"] * invz      # mpCurrentKeyFrame->mbf on BOTH sides (:384, :410)
            eR = u_r - ur
            e_mono = eX * eX + eY * eY
            e_st = eX * eX + eY * eY + eR * eR
            lhs = np.where(st, e_st, e_mono).astype(f64)
            rhs = np.where(st, CHI2_STEREO * s2.astype(f64), CHI2_MONO * s2.astype(f64))
            return lhs > rhs, (rhs - lhs) / rhs
        out1, m1 = reproj(c1, z1, st1, g["kx1"], g["ky1"], g["ur1"], g["s21"])
        out2, m2 = reproj(c2, z2, st2, g["kx2"], g["ky2"], g["ur2"], g["s22"])
        n1v = [X[:, i] - c1["Ow"][i] for i in range(3)]
        n2v = [X[:, i] - c2["Ow"][i] for i in range(3)]
        dist1, dist2 = np.sqrt(_ddot3(n1v, n1v)).astype(f32), np.sqrt(_ddot3(n2v, n2v)).astype(f32)
        zero = (dist1 == 0) | (dist2 == 0)
        ratioDist = dist2 / dist1
        ratioOctave = g["sf1"] / g["sf2"]
        lo, hi = ratioDist * rf, ratioOctave * rf
        sc = (lo < ratioOctave) | (ratioDist > hi)
        gate = np.zeros(len(X), np.int32)
        for code, fired in ((SCALE, sc), (ZERO_DIST, zero), (REPROJ_2, out2), (REPROJ_1, out1), (BEHIND_2, z2 <= 0), (BEHIND_1, z1 <= 0)):      # the earliest gate wins
            gate[fired] = code
        d1 = np.maximum(dist1.astype(f64), np.finfo(f64).tiny)
        d2 = np.maximum(dist2.astype(f64), np.finfo(f64).tiny)
        margins = np.stack([z1.astype(f64) / d1, z2.astype(f64) / d2, m1, m2, (lo.astype(f64) - ratioOctave) / ratioOctave, (hi.astype(f64) - ratioDist) / hi], axis=1)
        # upstream leaves at the first gate that fires: the later ones are not reached
        order = {BEHIND_1: 0, BEHIND_2: 1, REPROJ_1: 2, REPROJ_2: 3, ZERO_DIST: 3, SCALE: 5, 0: 5}
        last = np.array([order[int(c)] for c in gate])
        margins[np.arange(6)[None, :] > last[:, None]] = np.nan
    return gate, margins


def triangulate_neighbour(K1, cam1, K2, cam2, row, ratio_factor_, svd="eigh"):
    """The whole loop for one neighbour: verdict (n1,) and x3d (n1, 3) as eao_triangulate_matches_batch writes them, plus per populated slot (slot order) the
    smallest |margin| of any comparison upstream evaluated for it."""
    n1 = len(row)
    verdict, x3d = np.zeros(n1, np.int32), np.zeros((n1, 3), f32)
    pb = point_and_branch(K1, cam1, K2, cam2, row, svd)
    gate, gm = gates_after_point(K1, cam1, K2, cam2, row, ratio_factor_, pb["x3d"])
    has = np.isin(pb["branch"], ACCEPTING)
    v = np.where(has, np.where(gate != 0, gate, pb["branch"]), pb["branch"]).astype(np.int32)
    gm[~has] = np.nan
    allm = np.concatenate([pb["margins"], gm], axis=1)
    with np.errstate(all="ignore"):
        near = np.nanmin(np.where(np.isnan(allm), np.inf, np.abs(allm)), axis=1) if len(allm) else np.zeros(0)
    verdict[pb["idx1"]] = v
    x3d[pb["idx1"]] = pb["x3d"]
    return dict(verdict=verdict, x3d=x3d, idx1=pb["idx1"], idx2=pb["idx2"], branch=pb["branch"], pair_verdict=v, margins=allm, near=near)


def triangulate_batch(K1, cam1, K2s, cams2, match12, ratio_factor_, svd="eigh"):
    """Every neighbour: (verdict[n_nb, n1], x3d[n_nb, n1, 3], list of per-neighbour dicts)."""
    rows = np.asarray(match12, np.int32).reshape(len(K2s), -1)
    per = [triangulate_neighbour(K1, cam1, K2s[k], cams2[k], rows[k], ratio_factor_, svd) for k in range(len(K2s))]
    n1 = rows.shape[1]
    verdict = np.stack([p["verdict"] for p in per]) if per else np.zeros((0, n1), np.int32)
    x3d = np.stack([p["x3d"] for p in per]) if per else np.zeros((0, n1, 3), f32)
    return verdict, x3d, per
