"""Sim3Solver (reference src/Sim3Solver.cc): the Horn RANSAC of LoopClosing::ComputeSim3 through eao_sim3_solver_iterate /
eao_sim3_solver_iterate_batch (csrc/sim3_solver.hip).

prob: T1w / T2w (4,4) f32, Xw1 / Xw2 (n,3) f32, sigma2_1 / sigma2_2 (n,) f32, K1 / K2 (fx, fy, cx, cy), fix_scale.
state: dict(iterations, best_inliers, best_T12 (4,4), best_R (3,3), best_t (3,), best_s) or None for a new solver; never modified, the
new state comes back in the result.  triples: (n_hyp, 3) indices into 0 .. n-1 in draw order."""
import ctypes as C

import numpy as np

from . import _lib


def new_state():
    return dict(iterations=0, best_inliers=0, best_T12=np.zeros((4, 4), np.float32), best_R=np.zeros((3, 3), np.float32),
                best_t=np.zeros(3, np.float32), best_s=np.float32(0))


def _state_in(S, state):
    state = state or new_state()
    S.iterations, S.best_inliers = int(state["iterations"]), int(state["best_inliers"])
    S.best_T12[:] = [float(v) for v in np.asarray(state["best_T12"], np.float32).ravel()]
    S.best_R[:] = [float(v) for v in np.asarray(state["best_R"], np.float32).ravel()]
    S.best_t[:] = [float(v) for v in np.asarray(state["best_t"], np.float32).ravel()]
    S.best_s = float(state["best_s"])


def _state_out(S):
    return dict(iterations=int(S.iterations), best_inliers=int(S.best_inliers), best_T12=np.array(S.best_T12[:], np.float32).reshape(4, 4),
                best_R=np.array(S.best_R[:], np.float32).reshape(3, 3), best_t=np.array(S.best_t[:], np.float32), best_s=np.float32(S.best_s))


def _pack(prob, state, triples, inspect, P, S, R):
    keep = dict(T1w=np.ascontiguousarray(prob["T1w"], np.float32), T2w=np.ascontiguousarray(prob["T2w"], np.float32),
                Xw1=np.ascontiguousarray(prob["Xw1"], np.float32).reshape(-1, 3), Xw2=np.ascontiguousarray(prob["Xw2"], np.float32).reshape(-1, 3),
                s1=np.ascontiguousarray(prob["sigma2_1"], np.float32), s2=np.ascontiguousarray(prob["sigma2_2"], np.float32),
                triples=np.ascontiguousarray(triples, np.int32).reshape(-1, 3))
    n, nh = len(keep["Xw1"]), len(keep["triples"])
    assert len(keep["Xw2"]) == n and len(keep["s1"]) == n and len(keep["s2"]) == n
    K1, K2 = [float(v) for v in prob["K1"]], [float(v) for v in prob["K2"]]
    P.n = n
    P.T1w, P.T2w, P.Xw1, P.Xw2 = _lib.ptr(keep["T1w"]), _lib.ptr(keep["T2w"]), _lib.ptr(keep["Xw1"]), _lib.ptr(keep["Xw2"])
    P.sigma2_1, P.sigma2_2 = _lib.ptr(keep["s1"]), _lib.ptr(keep["s2"])
    P.fx1, P.fy1, P.cx1, P.cy1 = K1
    P.fx2, P.fy2, P.cx2, P.cy2 = K2
    P.fix_scale = 1 if prob["fix_scale"] else 0
    _state_in(S, state)
    keep["inlier"] = np.zeros(max(n, 1), np.uint8)
    R.inlier = _lib.ptr(keep["inlier"])
    if inspect:
        keep["hyp_inliers"] = np.zeros(max(nh, 1), np.int32)
        keep["hyp_T12"] = np.zeros((max(nh, 1), 4, 4), np.float32)
        keep["hyp_T21"] = np.zeros((max(nh, 1), 4, 4), np.float32)
        keep["hyp_inlier"] = np.zeros((max(nh, 1), max(n, 1)), np.uint8)
        R.hyp_inliers, R.hyp_T12, R.hyp_T21, R.hyp_inlier = (_lib.ptr(keep[k]) for k in ("hyp_inliers", "hyp_T12", "hyp_T21", "hyp_inlier"))
    return keep, n, nh


def _out(S, R, keep, n, nh, inspect):
    out = dict(returned=int(R.returned), n_inliers=int(R.n_inliers), T12=np.array(R.T12[:], np.float32).reshape(4, 4),
               inlier=keep["inlier"][:n].copy(), no_more=bool(R.no_more), state=_state_out(S))
    if inspect:
        out.update(hyp_inliers=keep["hyp_inliers"][:nh], hyp_T12=keep["hyp_T12"][:nh], hyp_T21=keep["hyp_T21"][:nh],
                   hyp_inlier=keep["hyp_inlier"].reshape(-1)[:nh * n].reshape(nh, n))
    return out


def sim3_solver_iterate(prob, state, triples, min_inliers=20, max_its=300, inspect=False):
    """Sim3Solver::iterate(len(triples), ...) of one solver (eao_sim3_solver_iterate).  Returns dict(returned, n_inliers, T12 (4,4), inlier (n,),
    no_more, state) and, with inspect, hyp_inliers (n_hyp,), hyp_T12 / hyp_T21 (n_hyp,4,4), hyp_inlier (n_hyp,n)."""
    P, S, R = _lib.Sim3SolverProblem(), _lib.Sim3SolverState(), _lib.Sim3SolverResult()
    keep, n, nh = _pack(prob, state, triples, inspect, P, S, R)
    _lib.check(_lib.load().eao_sim3_solver_iterate(C.byref(P), int(min_inliers), int(max_its), C.byref(S), _lib.ptr(keep["triples"]), nh, C.byref(R)))
    return _out(S, R, keep, n, nh, inspect)


def sim3_solver_iterate_batch(probs, states, triples, min_inliers=20, max_its=300, inspect=False):
    """One iterate call for each of a list of solvers in one launch chain (eao_sim3_solver_iterate_batch).  min_inliers / max_its: one value
    or one per problem.  Each entry as sim3_solver_iterate returns it."""
    nb = len(probs)
    mi = np.broadcast_to(np.asarray(min_inliers, np.int32), (nb,)).copy()
    mx = np.broadcast_to(np.asarray(max_its, np.int32), (nb,)).copy()
    Ps, Ss, Rs = (_lib.Sim3SolverProblem * max(nb, 1))(), (_lib.Sim3SolverState * max(nb, 1))(), (_lib.Sim3SolverResult * max(nb, 1))()
    tp, nh = (C.c_void_p * max(nb, 1))(), np.zeros(max(nb, 1), np.int32)
    keeps = []
    for b in range(nb):
        keep, n, h = _pack(probs[b], states[b], triples[b], inspect, Ps[b], Ss[b], Rs[b])
        tp[b], nh[b] = _lib.ptr(keep["triples"]), h
        keeps.append((keep, n, h))
    _lib.check(_lib.load().eao_sim3_solver_iterate_batch(nb, Ps, _lib.ptr(mi), _lib.ptr(mx), Ss, tp, _lib.ptr(nh), Rs))
    return [_out(Ss[b], Rs[b], keep, n, h, inspect) for b, (keep, n, h) in enumerate(keeps)]
