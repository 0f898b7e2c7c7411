"""Optimizer::OptimizeSim3 (reference src/Optimizer.cc:1437-1632) restated in numpy float64, vectorised over the edges: the test
suite's yardstick for eao_optimize_sim3 (csrc/sim3.hip).

What it restates, from the g2o the reference vendors (Thirdparty/g2o/g2o):
  - g2o::Sim3 (types/sim3.h): the exp map of a 7-vector (omega, upsilon, sigma) with its four branches on |sigma| < 1e-5 and
    theta < 1e-5 -- the small-angle branches build R = I + Omega + Omega^2 as upstream does --, Quaterniond(R) (Eigen's trace branch
    and largest-diagonal branches), Hamilton products, the quaternion-vector rotation, map, inverse and composition.  No quaternion
    is renormalised.
  - VertexSim3Expmap::oplusImpl (types_seven_dof_expmap.h): S <- exp(update) * S, update[6] = 0 under fix_scale.
  - EdgeSim3ProjectXYZ / EdgeInverseSim3ProjectXYZ: obs - cam_map(project(S.map(X))) and the same with S^-1 and camera 2, no
    depth check.  Their Jacobians are numeric (core/base_binary_edge.hpp): central differences with delta = 1e-9 on the free vertex.
  - RobustKernelHuber with delta = sqrtf(th2) in float, applied to chi2 = e' Omega e; the weighted system J' (rho' Omega) J,
    J' (-rho' Omega e).
  - the Levenberg-Marquardt schedule (core/optimization_algorithm_levenberg.cpp): lambda0 = 1e-5 * max diag at iteration 0 of
    every optimize(), rho with the +1e-3 scale, 1/3 .. 2/3 cropping, nu doubling, at most 10 trials, the "3 bad iterations" stop.
  - the dense linear solver (solvers/linear_solver_dense.h): a diagonally pivoted LDL^T with an isPositive test.
  - OptimizeSim3's control flow: optimize(5), the inlier pass on the STALE chi2 (the errors of the last trial evaluated, which may
    be a rejected one), the early return when fewer than 10 correspondences survive (no write-back), optimize(10 or 5), the final pass.

The camera-frame points are formed as the library forms them: R * Xw accumulated in double and rounded once to float, + t in float.
"""
import math

import numpy as np

DELTA = 1e-9
EPS = 0.00001
TAU = 1e-5
MAX_TRIALS = 10


# ---------------------------------------------------------------------- quaternions: coefficient order x, y, z, w (Eigen)
def qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by,
                     aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx,
                     aw * bw - ax * bx - ay * by - az * bz])


def qrot(q, v):
    """q * v for v of shape (..., 3): uv = q.vec x v, uv += uv, v + w uv + q.vec x uv."""
    v = np.asarray(v, np.float64)
    x, y, z, w = q
    v0, v1, v2 = v[..., 0], v[..., 1], v[..., 2]
    u0 = y * v2 - z * v1
    u1 = z * v0 - x * v2
    u2 = x * v1 - y * v0
    u0 = u0 + u0
    u1 = u1 + u1
    u2 = u2 + u2
    return np.stack([v0 + w * u0 + (y * u2 - z * u1),
                     v1 + w * u1 + (z * u0 - x * u2),
                     v2 + w * u2 + (x * u1 - y * u0)], axis=-1)


def quat_from_R(m):
    """Eigen::Quaternion<double>(const Matrix3d&): trace branch, else the largest diagonal (later index on a strict >)."""
    m = np.asarray(m, np.float64).reshape(3, 3)
    q = np.zeros(4)
    t = m[0, 0] + m[1, 1] + m[2, 2]
    if t > 0:
        t = math.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0] = (m[2, 1] - m[1, 2]) * t
        q[1] = (m[0, 2] - m[2, 0]) * t
        q[2] = (m[1, 0] - m[0, 1]) * t
        return q
    i = 0
    if m[1, 1] > m[0, 0]:
        i = 1
    if m[2, 2] > m[i, i]:
        i = 2
    j, k = (i + 1) % 3, (i + 2) % 3
    t = math.sqrt(m[i, i] - m[j, j] - m[k, k] + 1.0)
    q[i] = 0.5 * t
    t = 0.5 / t
    q[3] = (m[k, j] - m[j, k]) * t
    q[j] = (m[j, i] + m[i, j]) * t
    q[k] = (m[k, i] + m[i, k]) * t
    return q


def quat_to_R(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


# ---------------------------------------------------------------------- g2o::Sim3 as (q, t, s)
class Sim3:
    __slots__ = ("q", "t", "s")

    def __init__(self, q, t, s):
        self.q = np.asarray(q, np.float64).copy()
        self.t = np.asarray(t, np.float64).copy()
        self.s = float(s)

    def map(self, X):
        return self.s * qrot(self.q, X) + self.t

    def inverse(self):
        qc = np.array([-self.q[0], -self.q[1], -self.q[2], self.q[3]])
        c = -1. / self.s
        return Sim3(qc, qrot(qc, c * self.t), 1. / self.s)

    def __mul__(self, o):
        return Sim3(qmul(self.q, o.q), self.s * qrot(self.q, o.t) + self.t, self.s * o.s)

    def copy(self):
        return Sim3(self.q, self.t, self.s)


def _mat3_mul(A, B):
    out = np.zeros((3, 3))
    for i in range(3):
        for j in range(3):
            out[i, j] = A[i, 0] * B[0, j] + A[i, 1] * B[1, j] + A[i, 2] * B[2, j]
    return out


def sim3_exp(u):
    """Sim3(const Vector7d&): omega = u[0:3], upsilon = u[3:6], sigma = u[6]."""
    u = np.asarray(u, np.float64)
    w0, w1, w2, sigma = u[0], u[1], u[2], u[6]
    theta = math.sqrt(w0 * w0 + w1 * w1 + w2 * w2)
    Om = np.array([[0., -w2, w1], [w2, 0., -w0], [-w1, w0, 0.]])
    Om2 = _mat3_mul(Om, Om)
    s = math.exp(sigma)
    I3 = np.eye(3)
    if abs(sigma) < EPS:
        C = 1.
        if theta < EPS:
            A, B = 1. / 2., 1. / 6.
            R = I3 + Om + Om2
        else:
            st, ct = math.sin(theta), math.cos(theta)
            th2 = theta * theta
            A = (1 - ct) / th2
            B = (theta - st) / (th2 * theta)
            R = I3 + (st / theta) * Om + ((1 - ct) / (theta * theta)) * Om2
    else:
        C = (s - 1) / sigma
        if theta < EPS:
            sigma2 = sigma * sigma
            A = ((sigma - 1) * s + 1) / sigma2
            B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma)
            R = I3 + Om + Om2
        else:
            st, ct = math.sin(theta), math.cos(theta)
            R = I3 + (st / theta) * Om + ((1 - ct) / (theta * theta)) * Om2
            a, b = s * st, s * ct
            th2, sigma2 = theta * theta, sigma * sigma
            c = th2 + sigma2
            A = (a * sigma + (1 - b) * theta) / (theta * c)
            B = (C - ((b - 1) * sigma + a * theta) / c) / th2
    W = A * Om + B * Om2 + C * I3
    ups = u[3:6]
    t = np.array([W[i, 0] * ups[0] + W[i, 1] * ups[1] + W[i, 2] * ups[2] for i in range(3)])
    return Sim3(quat_from_R(R), t, s)


# ---------------------------------------------------------------------- the problem
def camera_points(T, Xw):
    """R Xw + t as the library forms the reference's float cv::Mat expression: product in double, one rounding, + t in float."""
    T = np.asarray(T, np.float32).reshape(4, 4)
    Xw = np.asarray(Xw, np.float32).reshape(-1, 3).astype(np.float64)
    R = T[:3, :3].astype(np.float64)
    prod = (Xw[:, 0:1] * R[:, 0] + Xw[:, 1:2] * R[:, 1]) + Xw[:, 2:3] * R[:, 2]
    return (prod.astype(np.float32) + T[:3, 3]).astype(np.float64)


class Edges:
    """The edge pairs of one problem (active subset selectable)."""

    def __init__(self, prob):
        self.X1 = camera_points(prob["T1w"], prob["Xw1"])
        self.X2 = camera_points(prob["T2w"], prob["Xw2"])
        self.o1 = np.asarray(prob["obs1"], np.float32).reshape(-1, 2).astype(np.float64)
        self.o2 = np.asarray(prob["obs2"], np.float32).reshape(-1, 2).astype(np.float64)
        self.i1 = np.asarray(prob["inv_sigma2_1"], np.float32).astype(np.float64)
        self.i2 = np.asarray(prob["inv_sigma2_2"], np.float32).astype(np.float64)
        self.K1 = [float(np.float32(v)) for v in prob["K1"]]
        self.K2 = [float(np.float32(v)) for v in prob["K2"]]
        self.th2 = float(np.float32(prob["th2"]))
        self.delta = float(np.sqrt(np.float32(prob["th2"])))       # const float deltaHuber = sqrt(th2)
        self.fix_scale = bool(prob["fix_scale"])


def proj_error(S, X, o, K):
    p = S.map(X)
    u, v = p[:, 0] / p[:, 2], p[:, 1] / p[:, 2]
    fx, fy, cx, cy = K
    return np.stack([o[:, 0] - (u * fx + cx), o[:, 1] - (v * fy + cy)], axis=1)


def errors(E, S, idx, Si=None):
    Si = S.inverse() if Si is None else Si
    e12 = proj_error(S, E.X2[idx], E.o1[idx], E.K1)
    e21 = proj_error(Si, E.X1[idx], E.o2[idx], E.K2)
    return e12, e21


def chi2(e, info):
    return e[:, 0] * (info * e[:, 0]) + e[:, 1] * (info * e[:, 1])


def huber(c, delta):
    """RobustKernelHuber::robustify: (rho, rho') per edge; dsqr = delta^2 in double."""
    dsqr = delta * delta
    s = np.sqrt(np.maximum(c, 0))
    inl = c <= dsqr
    rho0 = np.where(inl, c, 2 * s * delta - dsqr)
    with np.errstate(divide="ignore", invalid="ignore"):
        rho1 = np.where(inl, 1.0, delta / s)
    return rho0, rho1


def perturbations(S, fix_scale):
    """Sim3(+-delta e_d) * S for d = 0..6 ([2d] = +delta, [2d + 1] = -delta), the update's 7th entry zeroed under fix_scale."""
    out = []
    for d in range(7):
        for sgn in (1.0, -1.0):
            u = np.zeros(7)
            u[d] = sgn * DELTA
            if fix_scale:
                u[6] = 0
            out.append(sim3_exp(u) * S)
    return out


def numeric_jacobians(E, S, idx):
    """(J12, J21), each (m, 2, 7): central differences as core/base_binary_edge.hpp forms them."""
    scalar = 1.0 / (2 * DELTA)
    P = perturbations(S, E.fix_scale)
    m = len(idx)
    J12, J21 = np.zeros((m, 2, 7)), np.zeros((m, 2, 7))
    for d in range(7):
        Sp, Sm = P[2 * d], P[2 * d + 1]
        J12[:, :, d] = scalar * (proj_error(Sp, E.X2[idx], E.o1[idx], E.K1) - proj_error(Sm, E.X2[idx], E.o1[idx], E.K1))
        J21[:, :, d] = scalar * (proj_error(Sp.inverse(), E.X1[idx], E.o2[idx], E.K2) - proj_error(Sm.inverse(), E.X1[idx], E.o2[idx], E.K2))
    return J12, J21


def ldlt_pivot_solve(A, b):
    """Diagonally pivoted LDL^T (Eigen::LDLT's pivot rule: the largest remaining |diagonal|); ok = every pivot > 0 (isPositive)."""
    n = len(b)
    A = np.array(A, np.float64)
    perm = list(range(n))
    d = np.zeros(n)
    ok = True
    for k in range(n):
        p = k + int(np.argmax(np.abs(np.diag(A)[k:])))
        if p != k:
            A[[k, p], :] = A[[p, k], :]
            A[:, [k, p]] = A[:, [p, k]]
            perm[k], perm[p] = perm[p], perm[k]
        dk = A[k, k]
        d[k] = dk
        if not dk > 0:
            ok = False
        if dk == 0:
            continue
        for i in range(k + 1, n):
            l_ = A[i, k] / dk
            for j in range(k + 1, i + 1):
                A[i, j] -= l_ * A[k, j]
                A[j, i] = A[i, j]
            A[i, k] = l_
    if not ok:
        return False, np.zeros(n)
    y = np.array([b[perm[i]] for i in range(n)], np.float64)
    for i in range(n):
        for j in range(i):
            y[i] -= A[i, j] * y[j]
    y = y / d
    for i in range(n - 1, -1, -1):
        for j in range(i + 1, n):
            y[i] -= A[j, i] * y[j]
    x = np.zeros(n)
    for i in range(n):
        x[perm[i]] = y[i]
    return True, x


def build_system(E, S, idx):
    e12, e21 = errors(E, S, idx)
    c12, c21 = chi2(e12, E.i1[idx]), chi2(e21, E.i2[idx])
    r0a, r1a = huber(c12, E.delta)
    r0b, r1b = huber(c21, E.delta)
    J12, J21 = numeric_jacobians(E, S, idx)
    H = np.zeros((7, 7))
    b = np.zeros(7)
    for J, e, info, r1 in ((J12, e12, E.i1[idx], r1a), (J21, e21, E.i2[idx], r1b)):
        w = r1 * info
        H += np.einsum("nki,n,nkj->ij", J, w, J)
        om = -(info[:, None] * e) * r1[:, None]
        b += np.einsum("nki,nk->i", J, om)
    return float(np.sum(r0a) + np.sum(r0b)), H, b


def evaluate(E, S, idx):
    """computeActiveErrors + activeRobustChi2; also the inlier gate of this state per active correspondence."""
    e12, e21 = errors(E, S, idx)
    c12, c21 = chi2(e12, E.i1[idx]), chi2(e21, E.i2[idx])
    bad = (c12 > E.th2) | (c21 > E.th2)
    return float(np.sum(huber(c12, E.delta)[0]) + np.sum(huber(c21, E.delta)[0])), bad


def lm_optimize(E, S, idx, iterations, trace):
    """SparseOptimizer::optimize(iterations) with OptimizationAlgorithmLevenberg; returns (S, iterations done, stale gate)."""
    if len(idx) == 0:
        return S, 0, np.zeros(0, bool)
    lam, ni, nBad = 0.0, 2.0, 0
    stale = None
    done = 0
    for it in range(iterations):
        currentChi, H, b = build_system(E, S, idx)
        iniChi = currentChi
        if it == 0:
            lam = TAU * float(np.max(np.abs(np.diag(H))))
            ni, nBad = 2.0, 0
        qmax, rho = 0, 0.0
        while True:
            ok, x = ldlt_pivot_solve(H + lam * np.eye(7), b)
            if E.fix_scale:
                x[6] = 0
            trial = sim3_exp(x) * S
            tempChi, stale = evaluate(E, trial, idx)
            if not ok:
                tempChi = np.finfo(np.float64).max
            rho = currentChi - tempChi
            scale = float(np.sum(x * (lam * x + b))) + 1e-3
            rho /= scale
            if rho > 0 and math.isfinite(tempChi):
                alpha = 1. - math.pow(2 * rho - 1, 3)
                alpha = min(alpha, 2. / 3.)
                lam *= max(1. / 3., alpha)
                ni = 2.0
                currentChi = tempChi
                S = trial
            else:
                lam *= ni
                ni *= 2
            qmax += 1
            if not (rho < 0 and qmax < MAX_TRIALS):
                break
        trace.append((lam, currentChi, qmax))
        done += 1
        if qmax == MAX_TRIALS or rho == 0:
            break
        if (iniChi - currentChi) * 1e3 < iniChi:
            nBad += 1
        else:
            nBad = 0
        if nBad >= 3:
            break
    return S, done, stale


def optimize_sim3(prob):
    """The whole of OptimizeSim3 over a flattened problem (the eao_sim3_problem fields).  Returns the outputs of eao_optimize_sim3 plus
    the LM trace and the iteration budgets of the two optimize() calls: dict(q, t, s, removed, n_inliers, iters, early_exit,
    trace = [(lambda, chi2, trials)] of both passes, budget = (5, 10 if the first pass rejected anything else 5; 0 on early exit))."""
    E = Edges(prob)
    n = len(E.X1)
    S0 = Sim3(prob["q"], prob["t"], prob["s"])
    removed = np.zeros(n, np.uint8)
    trace = []
    idx = np.arange(n)
    S, it0, stale = lm_optimize(E, S0.copy(), idx, 5, trace)
    nBad = int(np.sum(stale)) if n else 0
    if n:
        removed[idx[stale]] = 1
    if n - nBad < 10:
        return dict(q=S0.q.copy(), t=S0.t.copy(), s=S0.s, removed=removed, n_inliers=0, iters=np.array([it0, 0], np.int32),
                    early_exit=True, trace=trace, budget=(5, 0))
    idx2 = np.nonzero(removed == 0)[0]
    S, it1, stale2 = lm_optimize(E, S, idx2, 10 if nBad > 0 else 5, trace)
    removed[idx2[stale2]] = 1
    return dict(q=S.q.copy(), t=S.t.copy(), s=S.s, removed=removed, n_inliers=int(len(idx2) - np.sum(stale2)),
                iters=np.array([it0, it1], np.int32), early_exit=False, trace=trace, budget=(5, 10 if nBad > 0 else 5))
