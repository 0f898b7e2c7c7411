"""PnPsolver (reference src/PnPsolver.cc): the EPnP RANSAC of Tracking::Relocalization through eao_pnp_solver_iterate /
eao_pnp_solver_iterate_batch (csrc/pnp_solver.hip).

prob: p3d_w (n,3) f32, p2d (n,2) f32, sigma2 (n,) f32, K (fx, fy, cx, cy), th2.
state: dict(iterations, best_inliers, best_Tcw (4,4), best_inlier (n,) u8) or None for a new solver; never modified, the new state comes back
in the result.  sets: (n_hyp, min_set) indices into 0 .. n-1 in draw order (min_set is the second dimension)."""
import ctypes as C

import numpy as np

from . import _lib


def new_state(n):
    return dict(iterations=0, best_inliers=0, best_Tcw=np.zeros((4, 4), np.float32), best_inlier=np.zeros(n, np.uint8))


def _pack(prob, state, sets, inspect, P, S, R):
    keep = dict(p3d=np.ascontiguousarray(prob["p3d_w"], np.float32).reshape(-1, 3), p2d=np.ascontiguousarray(prob["p2d"], np.float32).reshape(-1, 2),
                sigma2=np.ascontiguousarray(prob["sigma2"], np.float32).reshape(-1), sets=np.ascontiguousarray(sets, np.int32))
    assert keep["sets"].ndim == 2, "sets: (n_hyp, min_set)"
    n, (nh, min_set) = len(keep["p3d"]), keep["sets"].shape
    assert len(keep["p2d"]) == n and len(keep["sigma2"]) == n
    P.n = n
    P.p3d_w, P.p2d, P.sigma2 = _lib.ptr(keep["p3d"]), _lib.ptr(keep["p2d"]), _lib.ptr(keep["sigma2"])
    P.fx, P.fy, P.cx, P.cy = [float(v) for v in prob["K"]]
    P.th2 = float(prob["th2"])
    state = state or new_state(n)
    S.iterations, S.best_inliers = int(state["iterations"]), int(state["best_inliers"])
    S.best_Tcw[:] = [float(v) for v in np.asarray(state["best_Tcw"], np.float32).ravel()]
    keep["best_inlier"] = np.zeros(max(n, 1), np.uint8)
    keep["best_inlier"][:n] = np.asarray(state["best_inlier"], np.uint8)[:n]
    S.best_inlier = _lib.ptr(keep["best_inlier"])
    keep["inlier"] = np.zeros(max(n, 1), np.uint8)
    R.inlier = _lib.ptr(keep["inlier"])
    if inspect:
        h, r, m = max(nh, 1), nh + 1, max(n, 1)
        keep.update(hyp_R=np.zeros((h, 3, 3)), hyp_t=np.zeros((h, 3)), hyp_rep_err=np.zeros((h, 3)), hyp_choice=np.zeros(h, np.int32), hyp_inliers=np.zeros(h, np.int32),
                    hyp_inlier=np.zeros(h * m, np.uint8), rec_hyp=np.zeros(r, np.int32), rec_R=np.zeros((r, 3, 3)), rec_t=np.zeros((r, 3)),
                    rec_inliers=np.zeros(r, np.int32), rec_inlier=np.zeros(r * m, np.uint8))
        for k in ("hyp_R", "hyp_t", "hyp_rep_err", "hyp_choice", "hyp_inliers", "hyp_inlier", "rec_hyp", "rec_R", "rec_t", "rec_inliers", "rec_inlier"):
            setattr(R, k, _lib.ptr(keep[k]))
    return keep, n, nh, min_set


def _out(S, R, keep, n, nh, inspect):
    out = dict(returned=int(R.returned), refined=int(R.refined), n_inliers=int(R.n_inliers), Tcw=np.array(R.Tcw[:], np.float32).reshape(4, 4),
               inlier=keep["inlier"][:n].copy(), no_more=bool(R.no_more), n_records=int(R.n_records),
               state=dict(iterations=int(S.iterations), best_inliers=int(S.best_inliers), best_Tcw=np.array(S.best_Tcw[:], np.float32).reshape(4, 4),
                          best_inlier=keep["best_inlier"][:n].copy()))
    if inspect:
        nr = out["n_records"]
        out.update(hyp_R=keep["hyp_R"][:nh], hyp_t=keep["hyp_t"][:nh], hyp_rep_err=keep["hyp_rep_err"][:nh], hyp_choice=keep["hyp_choice"][:nh],
                   hyp_inliers=keep["hyp_inliers"][:nh], hyp_inlier=keep["hyp_inlier"][:nh * n].reshape(nh, n),
                   rec_hyp=keep["rec_hyp"][:nr], rec_R=keep["rec_R"][:nr], rec_t=keep["rec_t"][:nr], rec_inliers=keep["rec_inliers"][:nr],
                   rec_inlier=keep["rec_inlier"][:nr * n].reshape(nr, n))
    return out


def pnp_solver_iterate(prob, state, sets, min_inliers, max_its, inspect=False):
    """PnPsolver::iterate over len(sets) passes of its loop (eao_pnp_solver_iterate).  Returns dict(returned, refined, n_inliers, Tcw (4,4), inlier (n,), no_more,
    n_records, state) and, with inspect, hyp_R / hyp_t / hyp_rep_err / hyp_choice / hyp_inliers / hyp_inlier and rec_hyp / rec_R / rec_t / rec_inliers / rec_inlier."""
    P, S, R = _lib.PnpSolverProblem(), _lib.PnpSolverState(), _lib.PnpSolverResult()
    keep, n, nh, min_set = _pack(prob, state, sets, inspect, P, S, R)
    _lib.check(_lib.load().eao_pnp_solver_iterate(C.byref(P), int(min_inliers), int(max_its), int(min_set), C.byref(S), _lib.ptr(keep["sets"]), nh, C.byref(R)))
    return _out(S, R, keep, n, nh, inspect)


def pnp_solver_iterate_batch(probs, states, sets, min_inliers, max_its, inspect=False):
    """One iterate call for each of a list of solvers in one launch chain (eao_pnp_solver_iterate_batch): one round of Relocalization's loop over its candidates.
    min_inliers / max_its: one value or one per problem.  Each entry as pnp_solver_iterate returns it."""
    nb = len(probs)
    mi = np.broadcast_to(np.asarray(min_inliers, np.int32), (nb,)).copy()
    mx = np.broadcast_to(np.asarray(max_its, np.int32), (nb,)).copy()
    m = max(nb, 1)
    Ps, Ss, Rs = (_lib.PnpSolverProblem * m)(), (_lib.PnpSolverState * m)(), (_lib.PnpSolverResult * m)()
    sp, nh, ms = (C.c_void_p * m)(), np.zeros(m, np.int32), np.zeros(m, np.int32)
    keeps = []
    for b in range(nb):
        keep, n, h, s = _pack(probs[b], states[b], sets[b], inspect, Ps[b], Ss[b], Rs[b])
        sp[b], nh[b], ms[b] = _lib.ptr(keep["sets"]), h, s
        keeps.append((keep, n, h))
    _lib.check(_lib.load().eao_pnp_solver_iterate_batch(nb, Ps, _lib.ptr(mi), _lib.ptr(mx), _lib.ptr(ms), Ss, sp, _lib.ptr(nh), Rs))
    return [_out(Ss[b], Rs[b], keep, n, h, inspect) for b, (keep, n, h) in enumerate(keeps)]


def last_kernel_ms():
    """Device time of the four kernels of this thread's last call (EAO_PNP_EVENTS=1)."""
    ms = np.zeros(4, np.float32)
    _lib.check(_lib.load().eao_pnp_solver_last_kernel_ms(_lib.ptr(ms)))
    return ms
