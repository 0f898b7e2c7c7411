"""Optimizer::OptimizeEssentialGraph (reference src/Optimizer.cc:1141-1435) restated in numpy float64, vectorised over the edges: the
test suite's yardstick for eao_optimize_essential_graph (csrc/essential_graph.hip).

What it restates, from the g2o the reference vendors (Thirdparty/g2o/g2o):
  - g2o::Sim3::log (types/sim3.h:148-230): sigma = log(s), R = toRotationMatrix() (not renormalised), d = (trace - 1) / 2, the four
    branches on |sigma| < 1e-5 and d > 1 - 1e-5, acos(d), upsilon = W.lu().solve(t) -- a 3 x 3 partial-pivot LU.
  - EdgeSim3::computeError (types_seven_dof_expmap.h:114-122): (C * v0 * v1^-1).log(), information = identity, no robust kernel.
  - its numeric Jacobians (core/base_binary_edge.hpp:147-196): central differences, delta = 1e-9, through oplus = exp(update) * S with
    update[6] = 0 under fix_scale (that column is then exactly zero); a fixed vertex gets none.
  - the Levenberg-Marquardt schedule (core/optimization_algorithm_levenberg.cpp:61-189) with setUserLambdaInit(1e-16), a failed solve
    rejecting the trial (tempChi = DBL_MAX), optimize(20)'s stop rules.
  - the block solver without a marginalised vertex: the whole system is Hpp over the ACTIVE free vertices (those with an edge).
The linear solve is dense (numpy.linalg.solve of the permuted system); `perm` permutes the active free vertex blocks, so that the
yardstick's own sensitivity to the elimination order can be measured.

A problem is a dict: n, fixed, fix_scale, Scw (n, 8: q in x, y, z, w order, t, s), has_nc (n,), Snc (n, 8), edges (m, 3: i, j, kind; kind 0 =
loop connection, measured from Scw on both sides; kind 1 = normal edge, measured from Snc where has_nc), Xw (p, 3) float32, ref (p,)."""
import math

import numpy as np

from sim3_reference import Sim3, qmul, qrot, quat_from_R, quat_to_R, sim3_exp   # noqa: F401  (the scalar pieces; re-exported for the tests)

DELTA = 1e-9
EPS = 0.00001
LAMBDA_INIT = 1e-16
MAX_TRIALS = 10
MAX_ITERATIONS = 20


# ---------------------------------------------------------------------- arrays of Sim3: q (4, m), t (m, 3), s (m,)
class VSim3:
    __slots__ = ("q", "t", "s")

    def __init__(self, q, t, s):
        self.q, self.t, self.s = q, t, s

    @staticmethod
    def from_rows(a):
        a = np.asarray(a, np.float64).reshape(-1, 8)
        return VSim3(a[:, 0:4].T.copy(), a[:, 4:7].copy(), a[:, 7].copy())

    def rows(self):
        return np.concatenate([self.q.T, self.t, self.s[:, None]], axis=1)

    def take(self, idx):
        return VSim3(self.q[:, idx], self.t[idx], self.s[idx])

    def inverse(self):
        qc = np.stack([-self.q[0], -self.q[1], -self.q[2], self.q[3]])
        c = -1. / self.s
        return VSim3(qc, qrot(qc, c[:, None] * self.t), 1. / self.s)

    def __mul__(self, o):
        return VSim3(qmul(self.q, o.q), self.s[:, None] * qrot(self.q, o.t) + self.t, self.s * o.s)

    def map(self, X):
        return self.s[:, None] * qrot(self.q, X) + self.t


def broadcast(S, m):
    """One scalar Sim3 as m equal entries."""
    return VSim3(np.repeat(S.q[:, None], m, axis=1), np.repeat(S.t[None, :], m, axis=0), np.full(m, S.s))


def rotation_matrices(q):
    """Eigen's Quaternion::toRotationMatrix, product by product; (m, 3, 3)."""
    x, y, z, w = q
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    R = np.empty((len(x), 3, 3))
    R[:, 0, 0] = 1 - (tyy + tzz); R[:, 0, 1] = txy - twz; R[:, 0, 2] = txz + twy
    R[:, 1, 0] = txy + twz; R[:, 1, 1] = 1 - (txx + tzz); R[:, 1, 2] = tyz - twx
    R[:, 2, 0] = txz - twy; R[:, 2, 1] = tyz + twx; R[:, 2, 2] = 1 - (txx + tyy)
    return R


def lu3_solve(W, b):
    """x of W x = b for (m, 3, 3), (m, 3): partial-pivot LU (Eigen's PartialPivLU: the largest |entry| of the column, the first one on a tie)."""
    A = np.array(W, np.float64)
    y = np.array(b, np.float64)
    m = np.arange(len(A))
    for k in range(2):
        p = k + np.argmax(np.abs(A[:, k:, k]), axis=1)
        rk, rp = A[m, k].copy(), A[m, p].copy()
        A[m, k], A[m, p] = rp, rk
        yk, yp = y[m, k].copy(), y[m, p].copy()
        y[m, k], y[m, p] = yp, yk
        for i in range(k + 1, 3):
            l_ = A[:, i, k] / A[:, k, k]
            A[:, i, k + 1:] = A[:, i, k + 1:] - l_[:, None] * A[:, k, k + 1:]
            y[:, i] = y[:, i] - l_ * y[:, k]
    x = np.empty_like(y)
    x[:, 2] = y[:, 2] / A[:, 2, 2]
    x[:, 1] = (y[:, 1] - A[:, 1, 2] * x[:, 2]) / A[:, 1, 1]
    x[:, 0] = (y[:, 0] - A[:, 0, 1] * x[:, 1] - A[:, 0, 2] * x[:, 2]) / A[:, 0, 0]
    return x


def log_branches(S):
    """Per entry the branch Sim3::log takes: 2 * (|sigma| >= eps) + (d <= 1 - eps)."""
    sigma = np.log(S.s)
    R = rotation_matrices(S.q)
    d = 0.5 * (R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2] - 1)
    return 2 * (np.abs(sigma) >= EPS).astype(np.int64) + (~(d > 1 - EPS)).astype(np.int64)


def sim3_log(S):
    """Sim3::log of every entry: (m, 7) = (omega, upsilon, sigma)."""
    s = S.s
    sigma = np.log(s)
    R = rotation_matrices(S.q)
    d = 0.5 * (R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2] - 1)
    dR = np.stack([R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]], axis=1)
    small_sigma = np.abs(sigma) < EPS
    small_angle = d > 1 - EPS
    with np.errstate(all="ignore"):
        theta = np.arccos(d)
        theta2 = theta * theta
        omega = np.where(small_angle[:, None], 0.5 * dR, (theta / (2 * np.sqrt(1 - d * d)))[:, None] * dR)
        C = np.where(small_sigma, 1.0, (s - 1) / sigma)
        sigma2 = sigma * sigma
        a, b, c = s * np.sin(theta), s * np.cos(theta), theta2 + sigma * sigma
        A = np.where(small_sigma,
                     np.where(small_angle, 1. / 2., (1 - np.cos(theta)) / theta2),
                     np.where(small_angle, ((sigma - 1) * s + 1) / sigma2, (a * sigma + (1 - b) * theta) / (theta * c)))
        B = np.where(small_sigma,
                     np.where(small_angle, 1. / 6., (theta - np.sin(theta)) / (theta2 * theta)),
                     np.where(small_angle, ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma), (C - ((b - 1) * sigma + a * theta) / c) * 1. / theta2))
    m = len(s)
    Om = np.zeros((m, 3, 3))
    Om[:, 0, 1], Om[:, 0, 2] = -omega[:, 2], omega[:, 1]
    Om[:, 1, 0], Om[:, 1, 2] = omega[:, 2], -omega[:, 0]
    Om[:, 2, 0], Om[:, 2, 1] = -omega[:, 1], omega[:, 0]
    W = A[:, None, None] * Om + B[:, None, None] * (Om @ Om) + C[:, None, None] * np.eye(3)
    ups = lu3_solve(W, S.t)
    return np.concatenate([omega, ups, sigma[:, None]], axis=1)


# ---------------------------------------------------------------------- the graph
class Graph:
    def __init__(self, prob):
        self.n = int(prob["n"])
        self.fixed = int(prob["fixed"])
        self.fix_scale = bool(prob["fix_scale"])
        self.S0 = VSim3.from_rows(prob["Scw"])
        e = np.asarray(prob["edges"], np.int64).reshape(-1, 3)
        self.ei, self.ej, self.kind = e[:, 0], e[:, 1], e[:, 2]
        self.C = measurements(prob)
        active = np.zeros(self.n, bool)
        active[self.ei] = True
        active[self.ej] = True
        self.active = active
        free = active.copy()
        free[self.fixed] = False
        self.free = np.nonzero(free)[0]                 # active free vertices, ascending
        self.block = np.full(self.n, -1, np.int64)
        self.block[self.free] = np.arange(len(self.free))
        self.P = []                                     # Sim3(+-delta e_d), the 7th entry zeroed under fix_scale: [2d] = +, [2d + 1] = -
        for d in range(7):
            for sgn in (1.0, -1.0):
                u = np.zeros(7)
                u[d] = sgn * DELTA
                if self.fix_scale:
                    u[6] = 0
                self.P.append(sim3_exp(u))


def measurements(prob):
    """The edges' measurements S_ji (src/Optimizer.cc:1213-1344) as a VSim3 over the edges."""
    S = VSim3.from_rows(prob["Scw"])
    e = np.asarray(prob["edges"], np.int64).reshape(-1, 3)
    i, j, kind = e[:, 0], e[:, 1], e[:, 2]
    has = np.asarray(prob["has_nc"]).astype(bool)
    N = VSim3.from_rows(np.where(has[:, None], np.asarray(prob["Snc"], np.float64).reshape(-1, 8), S.rows()))
    normal = kind == 1
    rows_i = np.where(normal[:, None], N.rows()[i], S.rows()[i])
    rows_j = np.where(normal[:, None], N.rows()[j], S.rows()[j])
    return VSim3.from_rows(rows_j) * VSim3.from_rows(rows_i).inverse()


def edge_errors(G, S, Si=None, Sj=None):
    """(m, 7): (C * v0 * v1^-1).log() at the estimates S (Si / Sj override the two vertices' estimates per edge)."""
    Si = S.take(G.ei) if Si is None else Si
    Sj = S.take(G.ej) if Sj is None else Sj
    return sim3_log((G.C * Si) * Sj.inverse())


def numeric_jacobians(G, S, delta_pert=None):
    """(Ji, Jj), each (m, 7, 7): central differences as core/base_binary_edge.hpp forms them (a fixed vertex's block is left zero).
    delta_pert: another list of 14 perturbations with its step (the CPU test's wider-step check)."""
    P, delta = (G.P, DELTA) if delta_pert is None else delta_pert
    scalar = 1.0 / (2 * delta)
    m = len(G.ei)
    Si, Sj = S.take(G.ei), S.take(G.ej)
    Ji, Jj = np.zeros((m, 7, 7)), np.zeros((m, 7, 7))
    for d in range(7):
        Pp, Pm = broadcast(P[2 * d], m), broadcast(P[2 * d + 1], m)
        Ji[:, :, d] = scalar * (edge_errors(G, S, Si=Pp * Si, Sj=Sj) - edge_errors(G, S, Si=Pm * Si, Sj=Sj))
        Jj[:, :, d] = scalar * (edge_errors(G, S, Si=Si, Sj=Pp * Sj) - edge_errors(G, S, Si=Si, Sj=Pm * Sj))
    Ji[G.ei == G.fixed] = 0
    Jj[G.ej == G.fixed] = 0
    return Ji, Jj


def build_system(G, S):
    """chi2, H (7 nf x 7 nf, dense), b over the active free vertices."""
    e = edge_errors(G, S)
    Ji, Jj = numeric_jacobians(G, S)
    nf = len(G.free)
    H = np.zeros((nf, nf, 7, 7))
    b = np.zeros((nf, 7))
    bi, bj = G.block[G.ei], G.block[G.ej]
    fi, fj = bi >= 0, bj >= 0
    both = fi & fj
    np.add.at(H, (bi[fi], bi[fi]), np.einsum("mki,mkj->mij", Ji[fi], Ji[fi]))
    np.add.at(H, (bj[fj], bj[fj]), np.einsum("mki,mkj->mij", Jj[fj], Jj[fj]))
    Hij = np.einsum("mki,mkj->mij", Ji[both], Jj[both])
    np.add.at(H, (bi[both], bj[both]), Hij)
    np.add.at(H, (bj[both], bi[both]), np.transpose(Hij, (0, 2, 1)))
    np.add.at(b, bi[fi], -np.einsum("mki,mk->mi", Ji[fi], e[fi]))
    np.add.at(b, bj[fj], -np.einsum("mki,mk->mi", Jj[fj], e[fj]))
    return float(np.sum(e * e)), H.transpose(0, 2, 1, 3).reshape(7 * nf, 7 * nf), b.reshape(7 * nf)


def solve(H, b, lam, perm):
    """(ok, x) of (H + lam I) x = b, the vertex blocks eliminated in the order perm."""
    nf = len(b) // 7
    rows = (np.asarray(perm)[:, None] * 7 + np.arange(7)[None, :]).reshape(-1) if perm is not None else np.arange(7 * nf)
    A = (H + lam * np.eye(len(b)))[np.ix_(rows, rows)]
    try:
        xp = np.linalg.solve(A, b[rows])
    except np.linalg.LinAlgError:
        return False, np.zeros(len(b))
    x = np.zeros(len(b))
    x[rows] = xp
    return bool(np.all(np.isfinite(x))), x


def apply_update(G, S, x):
    """oplus on every active free vertex: exp(dx) * S, dx[6] = 0 under fix_scale."""
    q, t, s = S.q.copy(), S.t.copy(), S.s.copy()
    for k, v in enumerate(G.free):
        u = np.array(x[7 * k:7 * k + 7])
        if G.fix_scale:
            u[6] = 0
        T = sim3_exp(u) * Sim3(S.q[:, v], S.t[v], S.s[v])
        q[:, v], t[v], s[v] = T.q, T.t, T.s
    return VSim3(q, t, s)


def lm_optimize(G, S, trace, perm=None):
    """SparseOptimizer::optimize(20) with OptimizationAlgorithmLevenberg, lambda0 = 1e-16; returns (S, iterations, chi2 before the first)."""
    if len(G.ei) == 0 or len(G.free) == 0:
        return S, 0, 0.0
    lam, ni, nBad, done, chi0 = 0.0, 2.0, 0, 0, None
    for it in range(MAX_ITERATIONS):
        currentChi, H, b = build_system(G, S)
        iniChi = currentChi
        if it == 0:
            lam, ni, nBad, chi0 = LAMBDA_INIT, 2.0, 0, currentChi
        qmax, rho = 0, 0.0
        while True:
            ok, x = solve(H, b, lam, perm)
            if G.fix_scale:
                x[6::7] = 0
            trial = apply_update(G, S, x)
            e = edge_errors(G, trial)
            tempChi = float(np.sum(e * e))
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
    return S, done, chi0


def recover_poses(rows):
    """Tiw (n, 16) float32 of Sim3 rows: toRotationMatrix() of the quaternion, t * (1 / s), rounded once to float."""
    S = VSim3.from_rows(rows)
    T = np.zeros((len(S.s), 4, 4))
    T[:, :3, :3] = rotation_matrices(S.q)
    T[:, :3, 3] = S.t * (1. / S.s)[:, None]
    T[:, 3, 3] = 1
    return T.astype(np.float32).reshape(-1, 16)


def correct_points(rows_in, rows_out, Xw, ref):
    """correctedSwr.map(Srw.map(X)) in double, rounded once to float; ref = -1: the point as it is."""
    Xw = np.asarray(Xw, np.float32).reshape(-1, 3)
    ref = np.asarray(ref, np.int64)
    out = Xw.copy()
    k = np.nonzero(ref >= 0)[0]
    if len(k):
        Srw = VSim3.from_rows(rows_in).take(ref[k])
        Swr = VSim3.from_rows(rows_out).take(ref[k]).inverse()
        out[k] = Swr.map(Srw.map(Xw[k].astype(np.float64))).astype(np.float32)
    return out


def optimize_essential_graph(prob, perm=None):
    """The whole function over a flattened problem.  Returns the outputs of eao_optimize_essential_graph: dict(Scw (n, 8), Tiw (n, 16) f32,
    Xw_corrected (p, 3) f32, lm_iterations, trials, lambda, chi2 (per iteration), chi2_initial, n_active)."""
    G = Graph(prob)
    trace = []
    S, its, chi0 = lm_optimize(G, G.S0, trace, perm)
    rows_in = np.asarray(prob["Scw"], np.float64).reshape(-1, 8)
    rows = S.rows()
    untouched = np.ones(G.n, bool)
    untouched[G.free] = False
    rows[untouched] = rows_in[untouched]
    return dict(Scw=rows, Tiw=recover_poses(rows), Xw_corrected=correct_points(rows_in, rows, prob["Xw"], prob["ref"]),
                lm_iterations=its, trials=np.array([t[2] for t in trace], np.int32), **{"lambda": np.array([t[0] for t in trace])},
                chi2=np.array([t[1] for t in trace]), chi2_initial=chi0, n_active=int(G.active.sum()))
