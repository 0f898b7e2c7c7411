"""The yardstick of eao_initializer_initialize: Initializer::Initialize (reference src/Initializer.cc) after its draws, restated in numpy.  Float expressions stay
in float32 op for op (numpy rounds every float32 operation once); OpenCV's arithmetic follows the conventions of csrc/initializer.hip (a small product accumulates
in double in storage order and rounds once; cv::norm, Mat::dot, cv::determinant in double; the 3 x 3 inverse by cofactors over a double determinant).

The null-vector / SVD step comes in three variants:
  f32        a float32 SVD of the float A: one-sided (Hestenes) Jacobi on the columns, rotations applied in float32 with double dot products -- the scheme of a
             float cv::SVD (numpy.linalg.svd computes in double whatever the input type, so it cannot serve here),
  f64        numpy's float64 SVD of the float A, rounded to float,
  f64jacobi  the eigenvector of A^T A (double, from the float A) by cyclic Jacobi with the device's sweep counts, rounded to float.
The score comes as the exact double sum rounded once (`double`, the library's) and as upstream's sequential float sum (`float`)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from reference_literals import literals  # noqa: E402

f32, f64 = np.float32, np.float64
VARIANTS = ("f32", "f64", "f64jacobi")
BRANCH_H, BRANCH_F = 0, 1
SWEEPS = {3: 8, 4: 8, 9: 12}      # csrc/small_dense.h

_C = literals("initializer")
RATIO_H = float(_C["RATIO_H"])
CHI2_H, CHI2_F, CHI2_SCORE = f32(_C["CHI2_H"]), f32(_C["CHI2_F"]), f32(_C["CHI2_SCORE"])
COS_PARALLAX = float(_C["COS_PARALLAX"])
DEGENERATE = float(_C["DEGENERATE"])
SIMILAR, MIN_GOOD_FRACTION, SECOND_BEST = float(_C["SIMILAR"]), float(_C["MIN_GOOD_FRACTION"]), float(_C["SECOND_BEST"])
REPROJ_FACTOR = float(_C["REPROJ_FACTOR"])
PARALLAX_RANK = int(_C["PARALLAX_RANK"])
MIN_PARALLAX, MIN_TRIANGULATED = float(_C["MIN_PARALLAX"]), int(_C["MIN_TRIANGULATED"])
CV_PI = 3.1415926535897932384626433832795


# ---------------------------------------------------------------------- OpenCV's small-matrix arithmetic
def gemm(A, B):
    """float product: each element accumulates in double, k in storage order, and rounds once"""
    A, B = np.asarray(A, f32).astype(f64), np.asarray(B, f32).astype(f64)
    acc = A[..., :, 0:1] * B[..., 0:1, :]
    for k in range(1, A.shape[-1]):
        acc = acc + A[..., :, k:k + 1] * B[..., k:k + 1, :]
    return acc.astype(f32)


def det3(m):
    m = np.asarray(m, f32).astype(f64)
    return (m[..., 0, 0] * (m[..., 1, 1] * m[..., 2, 2] - m[..., 1, 2] * m[..., 2, 1]) - m[..., 0, 1] * (m[..., 1, 0] * m[..., 2, 2] - m[..., 1, 2] * m[..., 2, 0])
            + m[..., 0, 2] * (m[..., 1, 0] * m[..., 2, 1] - m[..., 1, 1] * m[..., 2, 0]))


def inv3(m):
    """cv::Mat::inv() of 3 x 3 CV_32F (batched): cofactors over a double determinant, rounded once; zero when the determinant is zero"""
    m = np.asarray(m, f32).astype(f64)
    d = np.asarray(det3(m))
    with np.errstate(all="ignore"):
        di = np.where(d != 0, 1.0 / np.where(d != 0, d, 1.0), 0.0)[..., None, None]
        a = lambda i, j: m[..., i, j]      # noqa: E731
        co = np.stack([np.stack([a(1, 1) * a(2, 2) - a(1, 2) * a(2, 1), a(0, 2) * a(2, 1) - a(0, 1) * a(2, 2), a(0, 1) * a(1, 2) - a(0, 2) * a(1, 1)], -1),
                       np.stack([a(1, 2) * a(2, 0) - a(1, 0) * a(2, 2), a(0, 0) * a(2, 2) - a(0, 2) * a(2, 0), a(0, 2) * a(1, 0) - a(0, 0) * a(1, 2)], -1),
                       np.stack([a(1, 0) * a(2, 1) - a(1, 1) * a(2, 0), a(0, 1) * a(2, 0) - a(0, 0) * a(2, 1), a(0, 0) * a(1, 1) - a(0, 1) * a(1, 0)], -1)], -2)
        out = (co * di).astype(f32)
    out[np.broadcast_to((d == 0)[..., None, None], out.shape)] = 0
    return out


def jacobi_eig(S, sweeps):
    """batched cyclic Jacobi on symmetric S (B, n, n) in double, a fixed number of sweeps, the device's update order; returns (diagonal (B, n), V (B, n, n))"""
    S = np.array(S, f64)
    B, n, _ = S.shape
    V = np.broadcast_to(np.eye(n), S.shape).copy()
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            for p in range(n - 1):
                for q in range(p + 1, n):
                    apq = S[:, p, q]
                    nz = apq != 0
                    theta = (S[:, q, q] - S[:, p, p]) / (2.0 * np.where(nz, apq, 1.0))
                    t = np.where(theta < 0, -1.0, 1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                    c = np.where(nz, 1.0 / np.sqrt(t * t + 1.0), 1.0)
                    s = np.where(nz, t * c, 0.0)
                    c, s = c[:, None], s[:, None]
                    a, b = S[:, :, p].copy(), S[:, :, q].copy()
                    S[:, :, p], S[:, :, q] = c * a - s * b, s * a + c * b
                    a, b = S[:, p, :].copy(), S[:, q, :].copy()
                    S[:, p, :], S[:, q, :] = c * a - s * b, s * a + c * b
                    a, b = V[:, :, p].copy(), V[:, :, q].copy()
                    V[:, :, p], V[:, :, q] = c * a - s * b, s * a + c * b
    return np.diagonal(S, axis1=1, axis2=2).copy(), V


def jacobi_svd_f32(A, sweeps=12):
    """batched one-sided Jacobi SVD in float32 of A (B, k, n): returns (w (B, n) descending column norms, Vt (B, n, n))"""
    W = np.array(A, f32)
    B, k, n = W.shape
    V = np.broadcast_to(np.eye(n, dtype=f32), (B, n, n)).copy()
    eps = float(np.finfo(f32).eps)
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            for i in range(n - 1):
                for j in range(i + 1, n):
                    wi, wj = W[:, :, i].astype(f64), W[:, :, j].astype(f64)
                    a, b, p = (wi * wi).sum(1), (wj * wj).sum(1), (wi * wj).sum(1)
                    act = np.abs(p) > eps * np.sqrt(a * b)
                    beta = a - b
                    gamma = np.hypot(2.0 * p, beta)
                    pos = beta >= 0
                    c = np.where(pos, np.sqrt((gamma + beta) / (2.0 * gamma)), 0.0)
                    sn = np.where(pos, p / (gamma * np.where(c != 0, c, 1.0)), np.sqrt((gamma - beta) / (2.0 * gamma)))
                    c = np.where(pos, c, p / (gamma * np.where(sn != 0, sn, 1.0)))
                    c = np.where(act, c, 1.0).astype(f32)[:, None]
                    sn = np.where(act, sn, 0.0).astype(f32)[:, None]
                    x, y = W[:, :, i].copy(), W[:, :, j].copy()
                    W[:, :, i], W[:, :, j] = c * x + sn * y, c * y - sn * x
                    x, y = V[:, :, i].copy(), V[:, :, j].copy()
                    V[:, :, i], V[:, :, j] = c * x + sn * y, c * y - sn * x
    w = np.sqrt((W.astype(f64) ** 2).sum(1))
    order = np.argsort(-w, 1, kind="stable")
    return np.take_along_axis(w, order, 1).astype(f32), np.take_along_axis(V, order[:, None, :], 2).transpose(0, 2, 1)


def null_vector(A, variant):
    """the right singular vector of the smallest singular value of the float systems A (B, k, n), as float (B, n); with the gap figures (s_1, s_{n-1}, s_n)"""
    A = np.asarray(A, f32)
    n = A.shape[-1]
    sv = np.linalg.svd(A.astype(f64), compute_uv=False)
    if sv.shape[-1] < n:
        sv = np.concatenate([sv, np.zeros(sv.shape[:-1] + (n - sv.shape[-1],))], -1)
    gaps = np.stack([sv[:, 0], sv[:, n - 2], sv[:, n - 1]], 1)
    if variant == "f32":
        v = jacobi_svd_f32(A)[1][:, n - 1, :]
    elif variant == "f64":
        v = np.linalg.svd(A.astype(f64), full_matrices=True)[2][:, n - 1, :]
    else:
        Ad = A.astype(f64)
        S = np.zeros((len(A), n, n))
        for r in range(A.shape[1]):
            S = S + Ad[:, r, :, None] * Ad[:, r, None, :]
        d, V = jacobi_eig(S, SWEEPS[n])
        j, best = np.zeros(len(A), np.int64), d[:, 0].copy()      # the device's scan: strict `<` from entry 0 (a NaN never replaces, a NaN at 0 is never replaced)
        with np.errstate(invalid="ignore"):
            for c in range(1, n):
                less = d[:, c] < best
                j, best = np.where(less, c, j), np.where(less, d[:, c], best)
        v = V[np.arange(len(A)), :, j]
    return v.astype(f32), gaps


def svd3(A, variant):
    """full SVD of one float 3 x 3: U, w (descending), Vt as floats"""
    A = np.asarray(A, f32)
    if variant == "f64":
        U, w, Vt = np.linalg.svd(A.astype(f64))
        return U.astype(f32), w.astype(f32), Vt.astype(f32)
    if variant == "f32":      # V and w in float32; U as the device forms it (no division by a vanishing singular value)
        w32, Vt32 = jacobi_svd_f32(A[None])
        Ad, V = A.astype(f64), Vt32[0].T.astype(f64)
        return _left_vectors(Ad, V), w32[0], Vt32[0].copy()
    Ad = A.astype(f64)
    S = np.zeros((3, 3))
    for r in range(3):
        S = S + Ad[r, :, None] * Ad[r, None, :]
    d, V = jacobi_eig(S[None], SWEEPS[3])
    d, V = d[0], V[0]
    for a, b in ((0, 1), (1, 2), (0, 1)):
        if d[a] < d[b]:
            d[[a, b]] = d[[b, a]]
            V[:, [a, b]] = V[:, [b, a]]
    return _left_vectors(Ad, V), np.sqrt(np.maximum(d, 0)).astype(f32), V.T.astype(f32)


def _left_vectors(Ad, V):
    """U of a 3 x 3 SVD from A and V: u0, u1 are A v normalised (Gram-Schmidt), u2 = u0 x u1 with the sign of A v2"""
    av = [Ad @ V[:, i] for i in range(3)]
    n0 = np.linalg.norm(av[0])
    u0 = av[0] / n0 if n0 > 0 else np.array([1.0, 0, 0])
    b = av[1] - (u0 @ av[1]) * u0
    n1 = np.linalg.norm(b)
    if not n1 > 1e-300:
        e = np.eye(3)[int(np.argmin(np.abs(u0)))]
        b = np.cross(u0, e)
        n1 = np.linalg.norm(b)
    u1 = b / n1
    u2 = np.cross(u0, u1)
    if u2 @ av[2] < 0:
        u2 = -u2
    return np.stack([u0, u1, u2], 1).astype(f32)


# ---------------------------------------------------------------------- the host part
def normalize(keys):
    """Initializer::Normalize (:749-795) over all keypoints of a frame, sequential float sums"""
    k = np.asarray(keys, f32).reshape(-1, 2)
    n = len(k)
    seq = lambda v: np.cumsum(v, dtype=f32)[-1]      # noqa: E731  (accumulate is sequential)
    mean = np.array([seq(k[:, 0]), seq(k[:, 1])], f32) / f32(n)
    pn = k - mean
    dev = np.array([seq(np.abs(pn[:, 0])), seq(np.abs(pn[:, 1]))], f32) / f32(n)
    with np.errstate(all="ignore"):
        s = (1.0 / dev.astype(f64)).astype(f32)
    pn = pn * s
    T = np.eye(3, dtype=f32)
    T[0, 0], T[1, 1] = s
    T[0, 2], T[1, 2] = -mean[0] * s[0], -mean[1] * s[1]
    return pn, T


def pack(prob):
    """the pairs (u1, v1, u2, v2) raw and normalised, `first`, T1, T2"""
    k1, k2 = np.asarray(prob["keys1"], f32).reshape(-1, 2), np.asarray(prob["keys2"], f32).reshape(-1, 2)
    m = np.asarray(prob["matches12"], np.int64).reshape(-1, 2)
    pn1, T1 = normalize(k1)
    pn2, T2 = normalize(k2)
    return dict(raw=np.concatenate([k1[m[:, 0]], k2[m[:, 1]]], 1), nrm=np.concatenate([pn1[m[:, 0]], pn2[m[:, 1]]], 1), first=m[:, 0], T1=T1, T2=T2, n1=len(k1))


def draw_sets(n, iterations, random_int):
    """:78-97"""
    sets = np.zeros((iterations, 8), np.int32)
    for it in range(iterations):
        avail = list(range(n))
        for j in range(8):
            randi = random_int(0, len(avail) - 1)
            sets[it, j] = avail[randi]
            avail[randi] = avail[-1]
            avail.pop()
    return sets


# ---------------------------------------------------------------------- hypotheses
def systems_h(P):
    """ComputeH21's A (:239-257) for sets of eight normalised pairs P (B, 8, 4)"""
    u1, v1, u2, v2 = (P[..., k] for k in range(4))
    z, o = np.zeros_like(u1), np.ones_like(u1)
    even = np.stack([z, z, z, -u1, -v1, -o, v2 * u1, v2 * v1, v2], -1)
    odd = np.stack([u1, v1, o, z, z, z, -u2 * u1, -u2 * v1, -u2], -1)
    return np.stack([even, odd], 2).reshape(P.shape[0], 16, 9).astype(f32)


def systems_f(P):
    """ComputeF21's A (:281-289)"""
    u1, v1, u2, v2 = (P[..., k] for k in range(4))
    return np.stack([u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, np.ones_like(u1)], -1).astype(f32)


def hypotheses(pk, sets, variant):
    """every H21i / H12i / F21i of FindHomography (:148-161) and FindFundamental (:199-212), with the conditioning figure of each: (s8 - s9) / s1 for H, s8 / s1 for F"""
    P = pk["nrm"][np.asarray(sets, np.int64)]
    T1, T2 = pk["T1"], pk["T2"]
    hn, gh = null_vector(systems_h(P), variant)
    fp, gf = null_vector(systems_f(P), variant)
    B = len(P)
    H21 = gemm(gemm(np.broadcast_to(inv3(T2), (B, 3, 3)), hn.reshape(B, 3, 3)), np.broadcast_to(T1, (B, 3, 3)))
    H12 = inv3(H21)
    Fn = np.zeros((B, 3, 3), f32)
    for b in range(B):
        U, w, Vt = svd3(fp[b].reshape(3, 3), variant)
        w = w.copy()
        w[2] = 0
        Fn[b] = gemm(gemm(U, np.diag(w)), Vt)
    F21 = gemm(gemm(np.broadcast_to(T2.T.copy(), (B, 3, 3)), Fn), np.broadcast_to(T1, (B, 3, 3)))
    with np.errstate(all="ignore"):
        return dict(H21=H21, H12=H12, F21=F21, gap_h=(gh[:, 1] - gh[:, 2]) / gh[:, 0], gap_f=gf[:, 1] / gf[:, 0])


# ---------------------------------------------------------------------- scores
def _inv_sigma_square(sigma):
    s = f32(sigma)
    with np.errstate(all="ignore"):
        return f32(1.0 / f64(s * s))


def _score(terms, added, how):
    t = np.where(added, terms, f32(0)).astype(f32).reshape(-1)
    if how == "float":
        return np.cumsum(t, dtype=f32)[-1]
    return f32(np.sum(t.astype(f64)))      # every term a multiple of 2^-23 below 8: exact in any order


def check_homography(H21, H12, raw, sigma, how="double"):
    """CheckHomography (:305-388): flags (N,), score, and the two chi-squares (N, 2) of each pair"""
    H, Hi = np.asarray(H21, f32).reshape(9), np.asarray(H12, f32).reshape(9)
    u1, v1, u2, v2 = (np.asarray(raw, f32)[:, k] for k in range(4))
    iss = _inv_sigma_square(sigma)
    with np.errstate(all="ignore"):
        w2 = (1.0 / (Hi[6] * u2 + Hi[7] * v2 + Hi[8]).astype(f64)).astype(f32)
        a, b = (Hi[0] * u2 + Hi[1] * v2 + Hi[2]) * w2, (Hi[3] * u2 + Hi[4] * v2 + Hi[5]) * w2
        chi1 = ((u1 - a) * (u1 - a) + (v1 - b) * (v1 - b)) * iss
        w1 = (1.0 / (H[6] * u1 + H[7] * v1 + H[8]).astype(f64)).astype(f32)
        a, b = (H[0] * u1 + H[1] * v1 + H[2]) * w1, (H[3] * u1 + H[4] * v1 + H[5]) * w1
        chi2 = ((u2 - a) * (u2 - a) + (v2 - b) * (v2 - b)) * iss
        chi = np.stack([chi1, chi2], 1)
        out = chi > CHI2_H
        return ~out.any(1), _score(CHI2_H - chi, ~out, how), chi


def check_fundamental(F21, raw, sigma, how="double"):
    """CheckFundamental (:390-468)"""
    F = np.asarray(F21, f32).reshape(9)
    u1, v1, u2, v2 = (np.asarray(raw, f32)[:, k] for k in range(4))
    iss = _inv_sigma_square(sigma)
    with np.errstate(all="ignore"):
        a2, b2, c2 = F[0] * u1 + F[1] * v1 + F[2], F[3] * u1 + F[4] * v1 + F[5], F[6] * u1 + F[7] * v1 + F[8]
        num2 = a2 * u2 + b2 * v2 + c2
        chi1 = (num2 * num2 / (a2 * a2 + b2 * b2)) * iss
        a1, b1, c1 = F[0] * u2 + F[3] * v2 + F[6], F[1] * u2 + F[4] * v2 + F[7], F[2] * u2 + F[5] * v2 + F[8]
        num1 = a1 * u1 + b1 * v1 + c1
        chi2 = (num1 * num1 / (a1 * a1 + b1 * b1)) * iss
        chi = np.stack([chi1, chi2], 1)
        out = chi > CHI2_F
        return ~out.any(1), _score(CHI2_SCORE - chi, ~out, how), chi


def first_argmax(scores):
    """the loop of :165-170 / :216-221: strict >, from 0; -1 when nothing scores"""
    best, idx = f32(0), -1
    for k, s in enumerate(np.asarray(scores, f32)):
        if s > best:
            best, idx = s, k
    return idx, best


def choose(SH, SF):
    """:112-118"""
    with np.errstate(all="ignore"):
        RH = f32(SH) / (f32(SH) + f32(SF))
    return RH, (BRANCH_H if f64(RH) > RATIO_H else BRANCH_F)


# ---------------------------------------------------------------------- reconstruction
def K_of(K):
    fx, fy, cx, cy = (f32(v) for v in K)
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], f32)


def decompose_e(F21, K, variant):
    """ReconstructF's head and DecomposeE (:479-487, :909-929): the four (R, t) in the order of :494-497"""
    Km = K_of(K)
    E = gemm(gemm(Km.T.copy(), F21), Km)
    U, w, Vt = svd3(E, variant)
    t = U[:, 2].copy()
    t = (t.astype(f64) * (1.0 / np.sqrt(np.sum(t.astype(f64) ** 2)))).astype(f32)
    W = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], f32)
    R1 = gemm(gemm(U, W), Vt)
    if det3(R1) < 0:
        R1 = -R1
    R2 = gemm(gemm(U, W.T.copy()), Vt)
    if det3(R2) < 0:
        R2 = -R2
    return [(R1, t), (R2, t), (R1, -t), (R2, -t)]


def decompose_h(H21, K, variant):
    """ReconstructH's head (:584-686): the eight (R, t), or None at the return of :597"""
    Km = K_of(K)
    A = gemm(gemm(inv3(Km), H21), Km)
    U, w, Vt = svd3(A, variant)
    s = f32(det3(U) * det3(Vt))
    d1, d2, d3 = w
    with np.errstate(all="ignore"):
        if f64(d1 / d2) < DEGENERATE or f64(d2 / d3) < DEGENERATE:
            return None
        aux1 = np.sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3))
        aux3 = np.sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3))
        x1, x3 = [aux1, aux1, -aux1, -aux1], [aux3, -aux3, aux3, -aux3]
        aux_st = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2)
        ct = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2)
        st = [aux_st, -aux_st, -aux_st, aux_st]
        aux_sp = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2)
        cp = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2)
        sp = [aux_sp, -aux_sp, -aux_sp, aux_sp]
        out = []
        for half in range(2):
            for i in range(4):
                Rp = np.eye(3, dtype=f32)
                if half == 0:
                    Rp[0, 0], Rp[0, 2], Rp[2, 0], Rp[2, 2] = ct, -st[i], st[i], ct
                    tp, sc = np.array([x1[i], 0, -x3[i]], f32), d1 - d3
                else:
                    Rp[0, 0], Rp[0, 2], Rp[1, 1], Rp[2, 0], Rp[2, 2] = cp, sp[i], -1, sp[i], -cp
                    tp, sc = np.array([x1[i], 0, x3[i]], f32), d1 + d3
                URp = (f64(s) * (U.astype(f64)[:, 0:1] * Rp.astype(f64)[0:1, :] + U.astype(f64)[:, 1:2] * Rp.astype(f64)[1:2, :] + U.astype(f64)[:, 2:3] * Rp.astype(f64)[2:3, :])).astype(f32)
                R = gemm(URp, Vt)
                tp = (tp.astype(f64) * f64(sc)).astype(f32)
                t = gemm(U, tp.reshape(3, 1)).reshape(3)
                t = (t.astype(f64) * (1.0 / np.sqrt(np.sum(t.astype(f64) ** 2)))).astype(f32)
                out.append((R, t))
        return out


def triangulate(raw, R, t, K, variant):
    """Triangulate (:734-747) of every pair: (N, 3) float, non-finite where the division makes it so"""
    Km = K_of(K)
    P1 = np.concatenate([Km, np.zeros((3, 1), f32)], 1)
    P2 = gemm(Km, np.concatenate([np.asarray(R, f32), np.asarray(t, f32).reshape(3, 1)], 1))
    raw = np.asarray(raw, f32)
    A = np.stack([raw[:, 0:1] * P1[2] - P1[0], raw[:, 1:2] * P1[2] - P1[1], raw[:, 2:3] * P2[2] - P2[0], raw[:, 3:4] * P2[2] - P2[1]], 1).astype(f32)
    v, _ = null_vector(A, variant)
    with np.errstate(all="ignore"):
        return (v[:, :3].astype(f64) * (1.0 / v[:, 3:4].astype(f64))).astype(f32)


def check_rt_gates(X, raw, R, t, K, th2):
    """CheckRT's gates (:841-892) on given points X (N, 3): accepted (N,), good (N,), cosParallax (N,), and the relative distance of each pair to its nearest gate"""
    X, raw, R, t = np.asarray(X, f32), np.asarray(raw, f32), np.asarray(R, f32), np.asarray(t, f32)
    fx, fy, cx, cy = (f32(v) for v in K)
    th2 = f32(th2)
    with np.errstate(all="ignore"):
        fin = np.isfinite(X).all(1)
        O2 = -gemm(R.T.copy(), t.reshape(3, 1)).reshape(3)
        Xd = X.astype(f64)
        dist1 = np.sqrt(Xd[:, 0] * Xd[:, 0] + Xd[:, 1] * Xd[:, 1] + Xd[:, 2] * Xd[:, 2]).astype(f32)
        n2 = X - O2
        n2d = n2.astype(f64)
        dist2 = np.sqrt(n2d[:, 0] * n2d[:, 0] + n2d[:, 1] * n2d[:, 1] + n2d[:, 2] * n2d[:, 2]).astype(f32)
        dot = Xd[:, 0] * n2d[:, 0] + Xd[:, 1] * n2d[:, 1] + Xd[:, 2] * n2d[:, 2]
        cosp = (dot / (dist1 * dist2).astype(f64)).astype(f32)
        par = cosp.astype(f64) < COS_PARALLAX
        C2 = gemm(X, R.T.copy()) + t      # (R*p3dC1)^T, the same sums in the same order
        ok = fin & ~((X[:, 2] <= 0) & par) & ~((C2[:, 2] <= 0) & par)
        iz1 = (1.0 / X[:, 2].astype(f64)).astype(f32)
        ex, ey = fx * X[:, 0] * iz1 + cx - raw[:, 0], fy * X[:, 1] * iz1 + cy - raw[:, 1]
        e1 = ex * ex + ey * ey
        iz2 = (1.0 / C2[:, 2].astype(f64)).astype(f32)
        ex, ey = fx * C2[:, 0] * iz2 + cx - raw[:, 2], fy * C2[:, 1] * iz2 + cy - raw[:, 3]
        e2 = ex * ex + ey * ey
        ok = ok & ~(e1 > th2) & ~(e2 > th2)
        # every gate's distance as a relative figure of the same kind as MARGIN_REL (a chi-square over its gate): the squared errors over th2; the cosine gate in
        # the quantity it bounds, 1 - cos (half the squared parallax angle), over 1 - COS_PARALLAX; a depth over the point's distance to that camera (the depth's
        # own scale: z / dist is the cosine of the ray's angle to the optical axis, and `<= 0` turns where it passes zero)
        margin = np.minimum.reduce([np.abs(e1 / th2 - 1), np.abs(e2 / th2 - 1), np.abs((1 - cosp.astype(f64)) / (1 - COS_PARALLAX) - 1),
                                    np.abs(X[:, 2]) / np.maximum(dist1, f32(1e-30)), np.abs(C2[:, 2]) / np.maximum(dist2, f32(1e-30))])
        margin = np.where(np.isfinite(margin), margin, 0.0)
    return ok, ok & par, cosp, margin


def im1_error(X, raw, K):
    return check_rt_gates(X, raw, np.eye(3, dtype=f32), np.zeros(3, f32), K, 1.0)


def parallax_of(c):
    with np.errstate(all="ignore"):
        return f32(np.arccos(f64(f32(c))) * 180 / CV_PI)


def check_rt(raw, first, inlier, R, t, K, sigma, n1, variant, X=None):
    """CheckRT (:798-907): dict(n_good, good (n1,), p3d (n1, 3), cosine, parallax, accepted (N,), margin (N,))"""
    s2 = f32(sigma) * f32(sigma)
    th2 = f32(REPROJ_FACTOR * f64(s2))
    Xa = triangulate(raw, R, t, K, variant) if X is None else X
    acc, good, cosp, margin = check_rt_gates(Xa, raw, R, t, K, th2)
    inl = np.asarray(inlier, bool)
    acc, good = acc & inl, good & inl
    p3d, vg = np.zeros((n1, 3), f32), np.zeros(n1, np.uint8)
    p3d[first[acc]] = Xa[acc]
    vg[first[good]] = 1
    n = int(acc.sum())
    cosine = f32(np.sort(cosp[acc])[min(PARALLAX_RANK, n - 1)]) if n > 0 else f32(1)
    return dict(n_good=n, good=vg, p3d=p3d, cosine=cosine, parallax=parallax_of(cosine) if n > 0 else f32(0), accepted=acc, margin=margin, X=Xa)


def rule_f(n_good, parallax, N, min_parallax, min_triangulated):
    """:499-569 -> (returned, best)"""
    g = [int(v) for v in n_good]
    maxGood = max(g)
    nMinGood = max(int(MIN_GOOD_FRACTION * N), int(min_triangulated))
    nsimilar = sum(1 for v in g if v > SIMILAR * maxGood)
    best = g.index(maxGood)
    if maxGood < nMinGood or nsimilar > 1:
        return False, best
    return bool(f32(parallax[best]) > f32(min_parallax)), best


def rule_h(n_good, parallax, N, min_parallax, min_triangulated):
    """:689-731 -> (returned, best)"""
    bestGood, second, best, bestPar = 0, 0, -1, f32(-1)
    for i, g in enumerate(int(v) for v in n_good):
        if g > bestGood:
            second, bestGood, best, bestPar = bestGood, g, i, f32(parallax[i])
        elif g > second:
            second = g
    ret = second < SECOND_BEST * bestGood and bestPar >= f32(min_parallax) and bestGood > int(min_triangulated) and bestGood > MIN_GOOD_FRACTION * N
    return bool(ret), best


def reconstruct(pk, prob, branch, M, inlier, variant):
    """ReconstructH / ReconstructF over the winner M with its flags"""
    K, sigma = prob["K"], prob.get("sigma", 1.0)
    mp, mt = prob.get("min_parallax", MIN_PARALLAX), prob.get("min_triangulated", MIN_TRIANGULATED)
    out = dict(returned=False, degenerate=False, motion=-1, motions=[], rt=[], R21=np.zeros((3, 3), f32), t21=np.zeros(3, f32), n_good=0, parallax=f32(0),
               p3d=np.zeros((pk["n1"], 3), f32), triangulated=np.zeros(pk["n1"], np.uint8))
    mots = decompose_h(M, K, variant) if branch == BRANCH_H else decompose_e(M, K, variant)
    if mots is None:
        out["degenerate"] = True
        return out
    rt = [check_rt(pk["raw"], pk["first"], inlier, R, t, K, sigma, pk["n1"], variant) for R, t in mots]
    N = int(np.asarray(inlier, bool).sum())
    ret, best = (rule_h if branch == BRANCH_H else rule_f)([r["n_good"] for r in rt], [r["parallax"] for r in rt], N, mp, mt)
    out.update(returned=ret, motion=best, motions=mots, rt=rt)
    if best >= 0:
        out.update(n_good=rt[best]["n_good"], parallax=rt[best]["parallax"])
    if ret:
        out.update(R21=mots[best][0], t21=mots[best][1], p3d=rt[best]["p3d"], triangulated=rt[best]["good"])
    return out


def initialize(prob, sets, variant="f64jacobi", how="double", pk=None, hyp=None):
    """Initializer::Initialize after its draws (:99-121)"""
    pk = pk or pack(prob)
    sigma = prob.get("sigma", 1.0)
    hyp = hyp or hypotheses(pk, sets, variant)
    B = len(hyp["H21"])
    rh = [check_homography(hyp["H21"][b], hyp["H12"][b], pk["raw"], sigma, how) for b in range(B)]
    rf = [check_fundamental(hyp["F21"][b], pk["raw"], sigma, how) for b in range(B)]
    SHs, SFs = np.array([r[1] for r in rh], f32), np.array([r[1] for r in rf], f32)
    bh, SH = first_argmax(SHs)
    bf, SF = first_argmax(SFs)
    RH, branch = choose(SH, SF)
    win = bh if branch == BRANCH_H else bf
    out = dict(hyp=hyp, hyp_SH=SHs, hyp_SF=SFs, hyp_inlier_H=np.array([r[0] for r in rh]), hyp_inlier_F=np.array([r[0] for r in rf]),
               hyp_chi_H=np.array([r[2] for r in rh]), hyp_chi_F=np.array([r[2] for r in rf]),
               best_h=bh, best_f=bf, SH=SH, SF=SF, RH=RH, branch=branch, no_model=win < 0, returned=False, degenerate=False, motion=-1, pk=pk)
    if win < 0:
        return out
    inlier = (rh if branch == BRANCH_H else rf)[win][0]
    M = hyp["H21"][win] if branch == BRANCH_H else hyp["F21"][win]
    out.update(inlier=inlier, n_inliers=int(inlier.sum()))
    out.update(reconstruct(pk, prob, branch, M, inlier, variant))
    return out


def unit(M):
    """a matrix scaled to unit Frobenius norm with the sign of its largest entry fixed (the null vector's sign is not held)"""
    M = np.asarray(M, f64)
    flat = M.reshape(M.shape[:-2] + (-1,))
    nrm = np.sqrt((flat * flat).sum(-1, keepdims=True))
    with np.errstate(all="ignore"):
        flat = flat / nrm
    big = np.take_along_axis(flat, np.argmax(np.abs(flat), -1)[..., None], -1)
    return (flat * np.where(big < 0, -1.0, 1.0)).reshape(M.shape)
