"""PnPsolver (reference src/PnPsolver.cc) restated in numpy: the yardstick of eao_pnp_solver_iterate (csrc/pnp_solver.hip, csrc/pnp_internal.h).

A checking restatement, written for reading beside the reference text, not for speed.  EPnP's own pieces follow the text line by line in float64.  OpenCV's
parts are not in the reference tree; what stands in for them:
  cvSVD of the symmetric 3 x 3 / 12 x 12   an eigen-solve, in one of three VARIANTS: numpy eigh, numpy svd, or the cyclic Jacobi the device runs ("jacobi":
                                           fixed sweeps, S and V rotated as csrc/small_dense.h jacobi_sym does).  Singular values |lambda| descending,
                                           the lower index first among equals.
  cvSVD of ABt                             numpy svd (R = U V^T does not depend on the signs of the pairs).
  cvInvert / cvSolve(CV_SVD)               pinv_rule(): one-sided Jacobi SVD, a singular value counts when it exceeds 2 * DBL_EPSILON * (the sum of all).
                                           The same function in every variant -- the least-squares rule is written down once.
Two deviations from upstream, shared by every variant and by the device:
  1. sign_rows(): each PCA axis (row of UCt) is signed so that its component of largest magnitude is positive (the lowest index wins a tie).
  2. gauss_newton's x starts at zero (upstream's is uninitialised when qr_solve returns through `eta == 0` in the first iteration).
`trace`, when given, counts the special lines a call went through (the eta == 0 return, the det < 0 flip, each branch of find_betas_approx_*)."""
import numpy as np

VARIANTS = ("eigh", "svd", "jacobi")
GN_ITERATIONS = 5                 # iterations_number (:843)
ALPHA_ONE = np.float32(1.0)       # a[0] = 1.0f - ... (:432)
L_TWO = np.float32(2.0)           # 2.0f * dot(...) (:790)
SWEEPS = {3: 10, 12: 16}          # kSweepsPca / kSweepsAbt, kSweepsMtM
SWEEPS_PINV = 12
DBL_EPSILON = float(np.finfo(np.float64).eps)


def _hit(trace, key):
    if trace is not None:
        trace[key] = trace.get(key, 0) + 1


def jacobi_cs(app, aqq, apq):
    if apq == 0.0:
        return 1.0, 0.0
    with np.errstate(all="ignore"):
        theta = (aqq - app) / (2.0 * apq)
        t = (-1.0 if theta < 0.0 else 1.0) / (abs(theta) + np.sqrt(theta * theta + 1.0))
        c = 1.0 / np.sqrt(t * t + 1.0)
    return c, t * c


def jacobi_sym(S, sweeps):
    """dense::jacobi_sym: the rotations in the device's order.  Returns (diagonal, V with the eigenvectors in its columns)."""
    S = np.array(S, np.float64)
    n = len(S)
    V = np.eye(n)
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            for p in range(n - 1):
                for q in range(p + 1, n):
                    c, s = jacobi_cs(S[p, p], S[q, q], S[p, q])
                    a, b = S[:, p].copy(), S[:, q].copy()
                    S[:, p], S[:, q] = c * a - s * b, s * a + c * b
                    a, b = S[p, :].copy(), S[q, :].copy()
                    S[p, :], S[q, :] = c * a - s * b, s * a + c * b
                    a, b = V[:, p].copy(), V[:, q].copy()
                    V[:, p], V[:, q] = c * a - s * b, s * a + c * b
    return np.diag(S).copy(), V


def order_desc(d):
    """Indices of |d| descending, the lower index first among equals (an insertion sort, as the device's: a NaN never moves forward)."""
    order = list(range(len(d)))
    a = np.abs(d)
    for i in range(1, len(d)):
        o, j = order[i], i
        while j > 0 and a[order[j - 1]] < a[o]:
            order[j] = order[j - 1]
            j -= 1
        order[j] = o
    return order


def sym_svd(S, variant):
    """cvSVD(S, D, Ut, 0, CV_SVD_U_T) of a symmetric S: (D descending, Ut with the singular vectors in its rows)."""
    S = np.asarray(S, np.float64)
    if not np.isfinite(S).all():
        variant = "jacobi"      # (numpy's solvers raise on a NaN; the fixed-sweep Jacobi ends like on any other input)
    if variant == "eigh":
        d, V = np.linalg.eigh(S)
    elif variant == "svd":
        U, d, _ = np.linalg.svd(S)
        V = U
    else:
        d, V = jacobi_sym(S, SWEEPS[len(S)])
    order = order_desc(d)
    return np.abs(d)[order], V[:, order].T.copy()


def sign_rows(uct):
    for i in range(3):
        m = 0
        for j in (1, 2):
            if abs(uct[i, j]) > abs(uct[i, m]):
                m = j
        if uct[i, m] < 0.0:
            uct[i] = -uct[i]
    return uct


def pinv_rule(A):
    """cvInvert(CV_SVD) / the matrix cvSolve(CV_SVD) applies: the pseudo-inverse through a one-sided Jacobi SVD (pnp_internal.h pinv)."""
    A = np.array(A, np.float64)
    m, n = A.shape
    V = np.eye(n)
    with np.errstate(all="ignore"):
        for _ in range(SWEEPS_PINV):
            for p in range(n - 1):
                for q in range(p + 1, n):
                    c, s = jacobi_cs(A[:, p] @ A[:, p], A[:, q] @ A[:, q], A[:, p] @ A[:, q])
                    a, b = A[:, p].copy(), A[:, q].copy()
                    A[:, p], A[:, q] = c * a - s * b, s * a + c * b
                    a, b = V[:, p].copy(), V[:, q].copy()
                    V[:, p], V[:, q] = c * a - s * b, s * a + c * b
        w2 = (A * A).sum(axis=0)
        w = np.sqrt(w2)
        thr = 2.0 * DBL_EPSILON * w.sum()
        P = np.zeros((n, m))
        for j in range(n):
            if w[j] > thr:
                P += np.outer(V[:, j], A[:, j]) / w2[j]
    return P


def qr_solve(A, b, x, trace=None):
    """qr_solve (:860-950), line by line, on copies; x is returned unchanged through the eta == 0 return."""
    A = np.array(A, np.float64).reshape(-1)
    b = np.array(b, np.float64)
    nr, nc = 6, 4
    A1, A2 = np.zeros(nc), np.zeros(nc)
    kk = 0
    with np.errstate(all="ignore"):
        for k in range(nc):
            ik = kk
            eta = abs(A[ik])
            for i in range(k + 1, nr):
                elt = abs(A[ik])
                if eta < elt:
                    eta = elt
                ik += nc
            if eta == 0:
                _hit(trace, "eta_zero")
                return x
            ik, s, inv_eta = kk, 0.0, 1.0 / eta
            for i in range(k, nr):
                A[ik] *= inv_eta
                s += A[ik] * A[ik]
                ik += nc
            sigma = np.sqrt(s)
            if A[kk] < 0:
                sigma = -sigma
            A[kk] += sigma
            A1[k] = sigma * A[kk]
            A2[k] = -eta * sigma
            for j in range(k + 1, nc):
                ij, s = kk, 0.0
                for i in range(k, nr):
                    s += A[ij] * A[ij + j - k]
                    ij += nc
                tau = s / A1[k]
                ij = kk
                for i in range(k, nr):
                    A[ij + j - k] -= tau * A[ij]
                    ij += nc
            kk += nc + 1
        jj = 0
        for j in range(nc):
            ij, tau = jj, 0.0
            for i in range(j, nr):
                tau += A[ij] * b[i]
                ij += nc
            tau /= A1[j]
            ij = jj
            for i in range(j, nr):
                b[i] -= tau * A[ij]
                ij += nc
            jj += nc + 1
        x = np.array(x, np.float64)
        x[nc - 1] = b[nc - 1] / A2[nc - 1]
        for i in range(nc - 2, -1, -1):
            ij, s = i * nc + i + 1, 0.0
            for j in range(i + 1, nc):
                s += A[ij] * x[j]
                ij += 1
            x[i] = (b[i] - s) / A2[i]
    return x


def gauss_newton(L, rho, betas, trace=None):
    betas = np.array(betas, np.float64)
    x = np.zeros(4)      # (deviation 2)
    with np.errstate(all="ignore"):
        for _ in range(GN_ITERATIONS):
            A, b = np.zeros((6, 4)), np.zeros(6)
            for i in range(6):
                r = L[i]
                A[i, 0] = 2 * r[0] * betas[0] + r[1] * betas[1] + r[3] * betas[2] + r[6] * betas[3]
                A[i, 1] = r[1] * betas[0] + 2 * r[2] * betas[1] + r[4] * betas[2] + r[7] * betas[3]
                A[i, 2] = r[3] * betas[0] + r[4] * betas[1] + 2 * r[5] * betas[2] + r[8] * betas[3]
                A[i, 3] = r[6] * betas[0] + r[7] * betas[1] + r[8] * betas[2] + 2 * r[9] * betas[3]
                b[i] = rho[i] - (r[0] * betas[0] * betas[0] + r[1] * betas[0] * betas[1] + r[2] * betas[1] * betas[1] + r[3] * betas[0] * betas[2] +
                                 r[4] * betas[1] * betas[2] + r[5] * betas[2] * betas[2] + r[6] * betas[0] * betas[3] + r[7] * betas[1] * betas[3] +
                                 r[8] * betas[2] * betas[3] + r[9] * betas[3] * betas[3])
            x = qr_solve(A, b, x, trace)
            betas = betas + x
    return betas


def find_betas(L, rho, kind, trace=None):
    """find_betas_approx_1 / _2 / _3 (:667-758)."""
    cols = {1: [0, 1, 3, 6], 2: [0, 1, 2], 3: [0, 1, 2, 3, 4]}[kind]
    b = pinv_rule(L[:, cols]) @ rho
    betas = np.zeros(4)
    with np.errstate(all="ignore"):
        if kind == 1:
            if b[0] < 0:
                _hit(trace, "approx1_neg")
                betas[0] = np.sqrt(-b[0])
                betas[1:4] = -b[1:4] / betas[0]
            else:
                _hit(trace, "approx1_pos")
                betas[0] = np.sqrt(b[0])
                betas[1:4] = b[1:4] / betas[0]
            return betas
        if b[0] < 0:
            _hit(trace, "approx%d_neg" % kind)
            betas[0] = np.sqrt(-b[0])
            betas[1] = np.sqrt(-b[2]) if b[2] < 0 else 0.0
        else:
            _hit(trace, "approx%d_pos" % kind)
            betas[0] = np.sqrt(b[0])
            betas[1] = np.sqrt(b[2]) if b[2] > 0 else 0.0
        if b[1] < 0:
            betas[0] = -betas[0]
        if kind == 3:
            betas[2] = b[3] / betas[0]
    return betas


def compute_pose(pws, us, K, variant="jacobi", trace=None):
    """compute_pose (:477-525) over pws (n,3), us (n,2) (float64 copies of the floats).  Returns R (3,3), t (3,), rep_errors (3,), N."""
    pws, us = np.asarray(pws, np.float64), np.asarray(us, np.float64)
    fu, fv, uc, vc = (float(k) for k in K)
    n = len(pws)
    with np.errstate(all="ignore"):
        # choose_control_points
        cws = np.zeros((4, 3))
        for i in range(n):
            cws[0] += pws[i]
        cws[0] /= n
        PW0 = pws - cws[0]
        S3 = np.zeros((3, 3))
        for i in range(n):
            S3 += np.outer(PW0[i], PW0[i])
        dc, uct = sym_svd(S3, variant)
        uct = sign_rows(uct)      # (deviation 1)
        for i in range(1, 4):
            cws[i] = cws[0] + np.sqrt(dc[i - 1] / n) * uct[i - 1]
        # compute_barycentric_coordinates
        CC = (cws[1:4] - cws[0]).T
        ci = pinv_rule(CC)
        alphas = np.zeros((n, 4))
        d = pws - cws[0]
        for j in range(3):
            alphas[:, 1 + j] = ci[j, 0] * d[:, 0] + ci[j, 1] * d[:, 1] + ci[j, 2] * d[:, 2]
        alphas[:, 0] = ALPHA_ONE - alphas[:, 1] - alphas[:, 2] - alphas[:, 3]
        # fill_M, MtM
        MtM = np.zeros((12, 12))
        for i in range(n):
            M1, M2 = np.zeros(12), np.zeros(12)
            M1[0::3] = alphas[i] * fu
            M1[2::3] = alphas[i] * (uc - us[i, 0])
            M2[1::3] = alphas[i] * fv
            M2[2::3] = alphas[i] * (vc - us[i, 1])
            MtM += np.outer(M1, M1)
            MtM += np.outer(M2, M2)
        _, ut = sym_svd(MtM, variant)
        # compute_L_6x10, compute_rho
        v = [ut[11], ut[10], ut[9], ut[8]]
        pairs = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
        L = np.zeros((6, 10))
        for i, (a, b) in enumerate(pairs):
            dv = [v[k][3 * a:3 * a + 3] - v[k][3 * b:3 * b + 3] for k in range(4)]
            dot = lambda x, y: x[0] * y[0] + x[1] * y[1] + x[2] * y[2]
            L[i] = [dot(dv[0], dv[0]), L_TWO * dot(dv[0], dv[1]), dot(dv[1], dv[1]), L_TWO * dot(dv[0], dv[2]), L_TWO * dot(dv[1], dv[2]), dot(dv[2], dv[2]),
                    L_TWO * dot(dv[0], dv[3]), L_TWO * dot(dv[1], dv[3]), L_TWO * dot(dv[2], dv[3]), dot(dv[3], dv[3])]
        rho = np.array([((cws[a] - cws[b]) ** 2).sum() for a, b in pairs])
        Rs, ts, rep = [None] * 4, [None] * 4, [np.nan] * 4
        for kind in (1, 2, 3):
            betas = gauss_newton(L, rho, find_betas(L, rho, kind, trace), trace)
            Rs[kind], ts[kind], rep[kind] = compute_R_and_t(ut, betas, alphas, pws, us, (fu, fv, uc, vc), trace)
        N = 1
        if rep[2] < rep[1]:
            N = 2
        if rep[3] < rep[N]:
            N = 3
    return Rs[N], ts[N], np.array(rep[1:4]), N


def compute_R_and_t(ut, betas, alphas, pws, us, K, trace=None):
    fu, fv, uc, vc = K
    n = len(pws)
    ccs = np.zeros((4, 3))
    for i in range(4):
        ccs += betas[i] * ut[11 - i].reshape(4, 3)
    pcs = alphas[:, 0:1] * ccs[0] + alphas[:, 1:2] * ccs[1] + alphas[:, 2:3] * ccs[2] + alphas[:, 3:4] * ccs[3]
    if n > 0 and pcs[0, 2] < 0.0:      # solve_for_sign
        _hit(trace, "sign_flip")
        pcs = -pcs
    # estimate_R_and_t
    pc0, pw0 = np.zeros(3), np.zeros(3)
    for i in range(n):
        pc0 += pcs[i]
        pw0 += pws[i]
    pc0 /= n
    pw0 /= n
    abt = np.zeros((3, 3))
    for i in range(n):
        abt += np.outer(pcs[i] - pc0, pws[i] - pw0)
    if np.isfinite(abt).all():
        U, _, Vt = np.linalg.svd(abt)
        R = U @ Vt
    else:
        R = np.full((3, 3), np.nan)
    det = np.linalg.det(R)
    if det < 0:
        _hit(trace, "det_flip")
        R[2] = -R[2]
    t = pc0 - R @ pw0
    # reprojection_error
    Xc = pws @ R[0] + t[0]
    Yc = pws @ R[1] + t[1]
    inv = 1.0 / (pws @ R[2] + t[2])
    ue, ve = uc + fu * Xc * inv, vc + fv * Yc * inv
    terms = np.sqrt((us[:, 0] - ue) ** 2 + (us[:, 1] - ve) ** 2)
    s = 0.0
    for i in range(n):
        s += terms[i]
    return R, t, s / n


def max_error(prob):
    return np.asarray(prob["sigma2"], np.float32) * np.float32(prob["th2"])      # mvMaxError (:154-156), float


def check_inliers(R, t, prob, return_error=False):
    """CheckInliers (:308-339) with upstream's widths: exact, so the device's flags can be replayed from ITS OWN poses bit for bit."""
    X = np.asarray(prob["p3d_w"], np.float32).reshape(-1, 3).astype(np.float64)
    uv = np.asarray(prob["p2d"], np.float32).reshape(-1, 2).astype(np.float64)
    fu, fv, uc, vc = (float(np.float32(k)) for k in prob["K"])
    R, t = np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3)
    with np.errstate(all="ignore"):
        Xc = (R[0, 0] * X[:, 0] + R[0, 1] * X[:, 1] + R[0, 2] * X[:, 2] + t[0]).astype(np.float32)
        Yc = (R[1, 0] * X[:, 0] + R[1, 1] * X[:, 1] + R[1, 2] * X[:, 2] + t[1]).astype(np.float32)
        invZc = (1 / (R[2, 0] * X[:, 0] + R[2, 1] * X[:, 1] + R[2, 2] * X[:, 2] + t[2])).astype(np.float32)
        ue = uc + fu * Xc.astype(np.float64) * invZc.astype(np.float64)
        ve = vc + fv * Yc.astype(np.float64) * invZc.astype(np.float64)
        distX = (uv[:, 0] - ue).astype(np.float32)
        distY = (uv[:, 1] - ve).astype(np.float32)
        error2 = distX * distX + distY * distY
        flags = error2 < max_error(prob)
    return (flags, error2) if return_error else flags


def pose_of(prob, idx, variant="jacobi", trace=None):
    """compute_pose over the correspondences idx (add_correspondence widens the floats)."""
    X = np.asarray(prob["p3d_w"], np.float32).reshape(-1, 3).astype(np.float64)[idx]
    uv = np.asarray(prob["p2d"], np.float32).reshape(-1, 2).astype(np.float64)[idx]
    return compute_pose(X, uv, [np.float32(k) for k in prob["K"]], variant, trace)


def to_Tcw(R, t):
    T = np.eye(4, dtype=np.float32)
    with np.errstate(all="ignore"):
        T[:3, :3] = np.asarray(R, np.float64).astype(np.float32)
        T[:3, 3] = np.asarray(t, np.float64).astype(np.float32)
    return T


def new_state(n):
    return dict(iterations=0, best_inliers=0, best_Tcw=np.zeros((4, 4), np.float32), best_inlier=np.zeros(n, np.uint8))


def refine(prob, best_inlier, min_inliers, variant="jacobi", trace=None):
    """Refine (:260-305): (success, R, t, flags)."""
    idx = np.flatnonzero(best_inlier)
    R, t, _, _ = pose_of(prob, idx, variant, trace)
    flags = check_inliers(R, t, prob)
    return int(flags.sum()) > min_inliers, R, t, flags


def sequential_rule(n, counts, hyp_flags, hyp_Tcw, refine_of, state, min_inliers, max_its):
    """The rule of iterate's loop over given counts; refine_of(flags) -> (ok, Tcw, flags, count), called once per distinct best set.  The replay the device tests
    use (over the device's own counts and Refine verdicts) and the once-per-record form of the yardstick."""
    st = dict(iterations=int(state["iterations"]), best_inliers=int(state["best_inliers"]), best_Tcw=np.array(state["best_Tcw"], np.float32),
              best_inlier=np.array(state["best_inlier"], np.uint8))
    out = dict(returned=-1, refined=0, n_inliers=0, Tcw=np.zeros((4, 4), np.float32), inlier=np.zeros(n, np.uint8), no_more=False, records=[])
    if n < min_inliers:
        out.update(no_more=True, state=st)
        return out
    verdict, best_hyp = None, -1      # verdict: Refine of the current best set, computed when first asked for
    for k, c in enumerate(counts):
        st["iterations"] += 1
        if c >= min_inliers:
            if c > st["best_inliers"]:
                st.update(best_inliers=int(c), best_inlier=np.asarray(hyp_flags[k], np.uint8).copy(), best_Tcw=np.array(hyp_Tcw[k], np.float32))
                out["records"].append(k)
                verdict, best_hyp = None, k
            if verdict is None:
                verdict = refine_of(st["best_inlier"])
            if verdict[0]:
                out.update(returned=k, refined=1, n_inliers=int(verdict[3]), Tcw=np.array(verdict[1], np.float32), inlier=np.asarray(verdict[2], np.uint8).copy())
                break
    if out["returned"] < 0 and st["iterations"] >= max_its:
        out["no_more"] = True
        if st["best_inliers"] >= min_inliers:
            out.update(returned=best_hyp if best_hyp >= 0 else len(counts), refined=0, n_inliers=st["best_inliers"], Tcw=st["best_Tcw"].copy(), inlier=st["best_inlier"].copy())
    out["state"] = st
    return out


def hypotheses(prob, sets, variant="jacobi", trace=None):
    """compute_pose + CheckInliers of every set: dict(R, t, rep, choice, inliers, inlier)."""
    sets = np.asarray(sets, np.int64)
    n = len(np.asarray(prob["sigma2"]))
    h = dict(R=np.zeros((len(sets), 3, 3)), t=np.zeros((len(sets), 3)), rep=np.zeros((len(sets), 3)), choice=np.zeros(len(sets), np.int32),
             inliers=np.zeros(len(sets), np.int32), inlier=np.zeros((len(sets), n), np.uint8))
    for k, s in enumerate(sets):
        R, t, rep, N = pose_of(prob, s, variant, trace)
        f = check_inliers(R, t, prob)
        h["R"][k], h["t"][k], h["rep"][k], h["choice"][k], h["inliers"][k], h["inlier"][k] = R, t, rep, N, f.sum(), f
    return h


def iterate(prob, state, sets, min_inliers, max_its, variant="jacobi", hyp=None, trace=None):
    """PnPsolver::iterate in the once-per-record form (what the device computes).  Returns the outcome dict of sequential_rule plus hyp."""
    n = len(np.asarray(prob["sigma2"]))
    state = state or new_state(n)
    if n < min_inliers:
        return sequential_rule(n, [], [], [], None, state, min_inliers, max_its)
    hyp = hyp or hypotheses(prob, sets, variant, trace)

    def refine_of(flags):
        ok, R, t, f = refine(prob, flags, min_inliers, variant, trace)
        return ok, to_Tcw(R, t), f, int(f.sum()), R, t

    out = sequential_rule(n, hyp["inliers"], hyp["inlier"], [to_Tcw(hyp["R"][k], hyp["t"][k]) for k in range(len(hyp["inliers"]))], refine_of, state, min_inliers, max_its)
    out["hyp"] = hyp
    return out


def iterate_literal(prob, state, sets, min_inliers, max_its, variant="jacobi", hyp=None):
    """The loop of :182-255 as written: Refine is called at EVERY hypothesis that passes the >= gate."""
    n = len(np.asarray(prob["sigma2"]))
    state = state or new_state(n)
    st = dict(iterations=int(state["iterations"]), best_inliers=int(state["best_inliers"]), best_Tcw=np.array(state["best_Tcw"], np.float32),
              best_inlier=np.array(state["best_inlier"], np.uint8))
    out = dict(returned=-1, refined=0, n_inliers=0, Tcw=np.zeros((4, 4), np.float32), inlier=np.zeros(n, np.uint8), no_more=False, records=[], refine_calls=0)
    if n < min_inliers:
        out.update(no_more=True, state=st)
        return out
    hyp = hyp or hypotheses(prob, sets, variant)
    best_hyp = -1
    for k in range(len(hyp["inliers"])):
        st["iterations"] += 1
        c = int(hyp["inliers"][k])
        if c >= min_inliers:
            if c > st["best_inliers"]:
                st.update(best_inliers=c, best_inlier=hyp["inlier"][k].copy(), best_Tcw=to_Tcw(hyp["R"][k], hyp["t"][k]))
                out["records"].append(k)
                best_hyp = k
            out["refine_calls"] += 1
            ok, R, t, f = refine(prob, st["best_inlier"], min_inliers, variant)
            if ok:
                out.update(returned=k, refined=1, n_inliers=int(f.sum()), Tcw=to_Tcw(R, t), inlier=f.astype(np.uint8))
                out["state"] = st
                return out
    if st["iterations"] >= max_its:
        out["no_more"] = True
        if st["best_inliers"] >= min_inliers:
            out.update(returned=best_hyp if best_hyp >= 0 else len(hyp["inliers"]), refined=0, n_inliers=st["best_inliers"], Tcw=st["best_Tcw"].copy(), inlier=st["best_inlier"].copy())
    out["state"] = st
    return out


def ransac_parameters(N, probability=0.99, minInliers=8, maxIterations=300, minSet=4, epsilon=0.4, th2=5.991):
    """SetRansacParameters (:121-157) with its float / int conversions: (min_inliers, max_its)."""
    eps = np.float32(epsilon)
    n_min = int(np.float32(N) * eps)      # int nMinInliers = N*mRansacEpsilon (int * float -> float, truncated)
    n_min = max(n_min, minInliers, minSet)
    if eps < np.float32(n_min) / np.float32(N):
        eps = np.float32(n_min) / np.float32(N)
    if n_min == N:
        its = 1
    else:
        with np.errstate(all="ignore"):
            v = np.ceil(np.log(1 - probability) / np.log(1 - float(eps) ** 3))      # pow(float, int) is double
        # N < min_inliers makes epsilon > 1 and the logarithm a NaN; its conversion to int is undefined upstream (INT_MIN on x86).  iterate leaves through
        # N < mRansacMinInliers before the value is read; the adapter and this function take INT_MIN, so max_its becomes 1.
        its = int(v) if np.isfinite(v) and abs(v) < 2 ** 31 else -2 ** 31
    return n_min, max(1, min(its, maxIterations))
