"""Sim3Solver (reference src/Sim3Solver.cc) restated in numpy: the yardstick of csrc/sim3_solver.hip.

Float where upstream holds CV_32F, double where it holds double.  OpenCV's own arithmetic is not in the reference tree (parity unpinned,
DESIGN.md); the choices, each made once and shared with the device:
  - small matrix products (Pr2 * Pr1.t(), R * Pr2, R * X + t, sRinv * t): each element accumulates in double, k = 0, 1, 2 in order, rounds once
    to float; an added or subtracted vector is then added in float (the rule eao_optimize_sim3 documents for Rcw * Xw + tcw),
  - a double scalar applied to a float matrix (C / 3, 2 * ang / norm, ms12i * R, (1.0 / ms12i) * R.t(), ms12i * (R * O2)): multiplies in double,
    rounds once; a chain of scalars folds into one double first,
  - cv::reduce, Mat::dot, cv::norm: double accumulation in storage order,
  - N11 .. N44: float expressions (at<float> operands), left to right,
  - cv::eigen on the symmetric 4 x 4 float matrix: EIGEN = "f64" -- numpy.linalg.eigh on the promoted matrix, the eigenvector of the largest
    eigenvalue rounded to float -- or "f32jacobi" -- a cyclic Jacobi solve in float32.  The device runs a cyclic Jacobi in double.  The two
    variants bracket what an OpenCV build may do; their spread is where tests/sim3_solver_tolerances.py comes from.  The eigenvector's sign is
    free: atan2(|v|, w) with v / |v| gives the same rotation for q and -q,
  - cv::Rodrigues: in double as OpenCV writes it (theta = |r|, c, s, c1 = 1 - c, R = c I + c1 r r^T + s [r]x), rounded once to float.
Reproduced, not repaired: a zero imaginary part gives 0 / 0 and a NaN T12; Project does not check depth; comparisons with NaN are false."""
import math

import numpy as np

F = np.float32
EIGEN = "f64"          # module default; compute_sim3(..., eigen=) overrides


def _dot3(a, b):
    """one element of a small gemm: float operands, double accumulation in order, one rounding"""
    return F(float(a[0]) * float(b[0]) + float(a[1]) * float(b[1]) + float(a[2]) * float(b[2]))


def _scaled(s, v):
    return F(float(s) * float(v))


def transform_points(T, X):
    """Rcw * X + tcw per point (T: 4x4 or 3x4 float32, X: (n,3) float32) -> (n,3) float32"""
    T = np.asarray(T, F)
    X = np.asarray(X, F).reshape(-1, 3)
    Td, Xd = T.astype(np.float64), X.astype(np.float64)
    with np.errstate(all="ignore"):
        out = np.empty((len(X), 3), F)
        for i in range(3):
            acc = (Td[i, 0] * Xd[:, 0] + Td[i, 1] * Xd[:, 1]) + Td[i, 2] * Xd[:, 2]
            out[:, i] = acc.astype(F) + T[i, 3]
    return out


def to_image(Pc, K):
    """FromCameraToImage / Project's tail (:397-401, :417-421), float op by op"""
    fx, fy, cx, cy = (F(v) for v in K)
    Pc = np.asarray(Pc, F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        invz = F(1) / Pc[:, 2]
        x, y = Pc[:, 0] * invz, Pc[:, 1] * invz
        return np.stack([fx * x + cx, fy * y + cy], axis=1).astype(F)


def gates(sigma2):
    """mvnMaxError (include/Sim3Solver.h:78-79 hold size_t): (size_t)(9.210 * sigma2), read as float by err < max"""
    return np.array([F(int(9.210 * float(s))) for s in np.asarray(sigma2, F)], F).reshape(-1)


def prepare(prob):
    """What the constructor computes (:94-109): camera-frame points, image points, gates"""
    X1c, X2c = transform_points(prob["T1w"], prob["Xw1"]), transform_points(prob["T2w"], prob["Xw2"])
    return dict(X1c=X1c, X2c=X2c, im1=to_image(X1c, prob["K1"]), im2=to_image(X2c, prob["K2"]), max1=gates(prob["sigma2_1"]),
                max2=gates(prob["sigma2_2"]), K1=prob["K1"], K2=prob["K2"], fix_scale=bool(prob["fix_scale"]), n=len(X1c))


def jacobi_top(N, dtype, sweeps=10):
    """cyclic Jacobi on a symmetric 4 x 4 in `dtype`: (eigenvalues descending, eigenvector of the largest).  The device's solve with dtype
    float64; the "f32jacobi" variant with float32."""
    D = dtype
    A = np.array(N, D)
    V = np.eye(4, dtype=D)
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            for p in range(3):
                for q in range(p + 1, 4):
                    apq = A[p, q]
                    if not (apq != 0):
                        continue
                    theta = (A[q, q] - A[p, p]) / (D(2) * apq)
                    t = (D(-1) if theta < 0 else D(1)) / (abs(theta) + np.sqrt(theta * theta + D(1)))
                    c = D(1) / np.sqrt(t * t + D(1))
                    s = t * c
                    akp, akq = A[:, p].copy(), A[:, q].copy()
                    A[:, p], A[:, q] = c * akp - s * akq, s * akp + c * akq
                    apk, aqk = A[p, :].copy(), A[q, :].copy()
                    A[p, :], A[q, :] = c * apk - s * aqk, s * apk + c * aqk
                    A[p, q] = A[q, p] = D(0)
                    vkp, vkq = V[:, p].copy(), V[:, q].copy()
                    V[:, p], V[:, q] = c * vkp - s * vkq, s * vkp + c * vkq
    w = np.array([A[k, k] for k in range(4)], np.float64)
    idx = 0
    for k in range(1, 4):
        if w[k] > w[idx]:
            idx = k
    return np.sort(w)[::-1], V[:, idx].astype(F)


def top_eigenvector(N, eigen=None):
    """(eigenvalues descending in float64, float32 eigenvector of the largest) of the float32 symmetric 4 x 4"""
    eigen = eigen or EIGEN
    if eigen == "f64":
        if not np.isfinite(N).all():
            return np.full(4, np.nan), np.full(4, np.nan, F)
        w, v = np.linalg.eigh(N.astype(np.float64))
        return w[::-1].copy(), v[:, 3].astype(F)
    if eigen == "f32jacobi":
        return jacobi_top(N, np.float32)
    if eigen == "f64jacobi":
        return jacobi_top(N, np.float64)
    raise ValueError(eigen)


def rodrigues(rv):
    r = np.asarray(rv, F).astype(np.float64)
    with np.errstate(all="ignore"):
        theta = math.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]) if np.isfinite(r).all() else float("nan")
        if theta < np.finfo(np.float64).eps:
            return np.eye(3, dtype=F)
        c, s = math.cos(theta) if math.isfinite(theta) else float("nan"), math.sin(theta) if math.isfinite(theta) else float("nan")
        c1, it = 1.0 - c, 1.0 / theta
        r = r * it
        skew = [[0.0, -r[2], r[1]], [r[2], 0.0, -r[0]], [-r[1], r[0], 0.0]]
        R = np.empty((3, 3), F)
        for i in range(3):
            for j in range(3):
                R[i, j] = F(c * (1.0 if i == j else 0.0) + c1 * (r[i] * r[j]) + s * skew[i][j])
        return R


def compute_sim3(P1, P2, fix_scale, eigen=None):
    """Sim3Solver::ComputeSim3 (:226-337).  P1 / P2: (3,3) float32, column i = sampled point i (the P3Dc1i / P3Dc2i of :154-155).
    Returns dict(T12, T21 (4,4) f32, R (3,3), t (3,), s, eigenvalues (4,) descending f64)."""
    P1, P2 = np.asarray(P1, F), np.asarray(P2, F)
    with np.errstate(all="ignore"):
        def centroid(P):
            O = np.empty(3, F)
            for r in range(3):
                s = F(float(P[r, 0]) + float(P[r, 1]) + float(P[r, 2]))
                O[r] = _scaled(1.0 / 3, s)
            return O, (P - O[:, None]).astype(F)
        O1, Pr1 = centroid(P1)
        O2, Pr2 = centroid(P2)
        M = np.empty((3, 3), F)
        for i in range(3):
            for j in range(3):
                M[i, j] = _dot3(Pr2[i], Pr1[j])
        N11 = M[0, 0] + M[1, 1] + M[2, 2]
        N12 = M[1, 2] - M[2, 1]
        N13 = M[2, 0] - M[0, 2]
        N14 = M[0, 1] - M[1, 0]
        N22 = M[0, 0] - M[1, 1] - M[2, 2]
        N23 = M[0, 1] + M[1, 0]
        N24 = M[2, 0] + M[0, 2]
        N33 = -M[0, 0] + M[1, 1] - M[2, 2]
        N34 = M[1, 2] + M[2, 1]
        N44 = -M[0, 0] - M[1, 1] + M[2, 2]
        N = np.array([[N11, N12, N13, N14], [N12, N22, N23, N24], [N13, N23, N33, N34], [N14, N24, N34, N44]], F)
        evals, q = top_eigenvector(N, eigen)
        qd = q.astype(np.float64)
        nrm = math.sqrt(qd[1] * qd[1] + qd[2] * qd[2] + qd[3] * qd[3]) if np.isfinite(qd).all() else float("nan")
        ang = math.atan2(nrm, qd[0])
        k = np.float64(2 * ang) / np.float64(nrm)
        rv = np.array([_scaled(k, q[1]), _scaled(k, q[2]), _scaled(k, q[3])], F)
        R = rodrigues(rv)
        ms = F(1)
        if not fix_scale:
            nom = den = 0.0
            for i in range(3):
                for j in range(3):
                    p3 = _dot3(R[i], Pr2[:, j])
                    nom += float(Pr1[i, j]) * float(p3)
                    den += float(F(p3 * p3))
            ms = F(np.float64(nom) / np.float64(den))
        msd, inv = np.float64(ms), np.float64(1.0) / np.float64(ms)
        t = np.empty(3, F)
        for i in range(3):
            acc = np.float64(R[i, 0]) * np.float64(O2[0]) + np.float64(R[i, 1]) * np.float64(O2[1]) + np.float64(R[i, 2]) * np.float64(O2[2])
            t[i] = O1[i] - F(msd * acc)
        sR = (msd * R.astype(np.float64)).astype(F)
        sRi = (inv * R.T.astype(np.float64)).astype(F)
        ti = np.array([-_dot3(sRi[i], t) for i in range(3)], F)
    T12, T21 = np.eye(4, dtype=F), np.eye(4, dtype=F)
    T12[:3, :3], T12[:3, 3], T21[:3, :3], T21[:3, 3] = sR, t, sRi, ti
    return dict(T12=T12, T21=T21, R=R, t=t, s=ms, eigenvalues=evals)


def errors(pre, T12, T21):
    """err1, err2 of CheckInliers (:343-354) for every correspondence, float32"""
    with np.errstate(all="ignore"):
        p2im1 = to_image(transform_points(T12, pre["X2c"]), pre["K1"])
        p1im2 = to_image(transform_points(T21, pre["X1c"]), pre["K2"])
        d1 = (pre["im1"] - p2im1).astype(np.float64)
        d2 = (p1im2 - pre["im2"]).astype(np.float64)
        return (d1[:, 0] * d1[:, 0] + d1[:, 1] * d1[:, 1]).astype(F), (d2[:, 0] * d2[:, 0] + d2[:, 1] * d2[:, 1]).astype(F)


def check_inliers(pre, T12, T21):
    """mvbInliersi as uint8 (its sum is mnInliersi).  pre: prepare(problem)"""
    if pre["n"] == 0:
        return np.zeros(0, np.uint8)
    e1, e2 = errors(pre, T12, T21)
    with np.errstate(all="ignore"):
        return ((e1 < pre["max1"]) & (e2 < pre["max2"])).astype(np.uint8)


def draw_triple(N, rand_ints):
    """The sampling loop of :163-177 with its quirk: vAvailableIndices[idx] = back() with idx the drawn VALUE, not the drawn position.
    rand_ints(lo, hi) stands for DUtils::Random::RandomInt.  Over a buffer of capacity N, so that the write upstream makes one past the
    shrunken size stays inside the allocation it has there too."""
    avail = list(range(N))
    size = N
    out = []
    for _ in range(3):
        randi = rand_ints(0, size - 1)
        idx = avail[randi]
        out.append(idx)
        assert 0 <= idx < N
        avail[idx] = avail[size - 1]
        size -= 1
    return tuple(out)


def ransac_max_iterations(N, probability=0.99, min_inliers=6, max_iterations=300):
    """mRansacMaxIts as SetRansacParameters leaves it (:125-135).  N < min_inliers: upstream never uses the value (iterate returns at :146)
    and the formula would convert a NaN to int; the argument comes back."""
    if N < min_inliers:
        return max_iterations
    if min_inliers == N:
        its = 1
    else:
        eps = F(F(min_inliers) / F(N))
        its = int(math.ceil(math.log(1 - probability) / math.log(1 - math.pow(float(eps), 3))))
    return max(1, min(its, max_iterations))


def new_state():
    return dict(iterations=0, best_inliers=0, best_T12=np.zeros((4, 4), F), best_R=np.zeros((3, 3), F), best_t=np.zeros(3, F), best_s=F(0))


def sequential_rule(counts, state_iterations, best_inliers, min_inliers, max_its, n):
    """The integer part of iterate (:146-206) over the counts of a chunk.  Returns (returned, best position or -1, iterations, best_inliers, no_more)."""
    if n < min_inliers:
        return -1, -1, state_iterations, best_inliers, True
    it, best, bk, ret = state_iterations, best_inliers, -1, -1
    for k in range(min(len(counts), max(0, max_its - state_iterations))):
        it += 1
        if counts[k] >= best:
            best, bk = int(counts[k]), k
            if counts[k] > min_inliers:
                ret = k
                break
    return ret, bk, it, best, (ret < 0 and it >= max_its)


def iterate(prob, state, triples, min_inliers=20, max_its=300, eigen=None, pre=None):
    """Sim3Solver::iterate over explicit triples.  Returns the dict eao_fusion_amd.sim3_solver.sim3_solver_iterate returns with inspect."""
    pre = pre or prepare(prob)
    n = pre["n"]
    state = dict(state or new_state())
    triples = np.asarray(triples, np.int64).reshape(-1, 3)
    nh = len(triples)
    out = dict(returned=-1, n_inliers=0, T12=np.zeros((4, 4), F), inlier=np.zeros(n, np.uint8), no_more=False,
               hyp_inliers=np.zeros(nh, np.int32), hyp_T12=np.zeros((nh, 4, 4), F), hyp_T21=np.zeros((nh, 4, 4), F),
               hyp_inlier=np.zeros((nh, n), np.uint8), hyp_eigenvalues=np.zeros((nh, 4)))
    if n < min_inliers:
        out["no_more"] = True
        out["state"] = state
        return out
    n_eval = min(nh, max(0, max_its - state["iterations"]))
    hyps = []
    for k in range(n_eval):
        tr = triples[k]
        h = compute_sim3(pre["X1c"][tr].T, pre["X2c"][tr].T, pre["fix_scale"], eigen)
        hyps.append(h)
        fl = check_inliers(pre, h["T12"], h["T21"])
        out["hyp_inliers"][k], out["hyp_T12"][k], out["hyp_T21"][k], out["hyp_inlier"][k] = fl.sum(), h["T12"], h["T21"], fl
        out["hyp_eigenvalues"][k] = h["eigenvalues"]
    ret, bk, it, best, no_more = sequential_rule(out["hyp_inliers"][:n_eval], state["iterations"], state["best_inliers"], min_inliers, max_its, n)
    state["iterations"], state["best_inliers"] = it, best
    if bk >= 0:
        state.update(best_T12=hyps[bk]["T12"].copy(), best_R=hyps[bk]["R"].copy(), best_t=hyps[bk]["t"].copy(), best_s=F(hyps[bk]["s"]))
    if ret >= 0:
        out.update(returned=ret, n_inliers=best, T12=hyps[ret]["T12"].copy(), inlier=out["hyp_inlier"][ret].copy())
    out["no_more"] = no_more
    out["state"] = state
    return out
