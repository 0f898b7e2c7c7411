"""PnPsolver on the device (eao_pnp_solver_iterate / _batch, csrc/pnp_solver.hip) on the families of tests/pnp_solver_scenes.py.

What is held, and where (the two findings behind it: tests/test_pnp_solver_reference_cpu.py):
  replay        every family, min_set = 4 and the degenerate ones included, no exclusions: CheckInliers restated in numpy with its exact float / double steps on
                the DEVICE'S OWN poses gives the device's flags and counts bit for bit; hyp_choice is the rule of :518-520 on the device's own reprojection
                errors; the records, the outcome and the new state are the sequential rule replayed over the device's counts and Refine verdicts.
  hypotheses    min_set >= 6 families against the recorded yardstick (tests/golden/pnp_solver/*.npz), on the hypotheses the yardstick marks conditioned.
  Refine        every family with a record: the yardstick's compute_pose on the device's own inlier set.
  outcome       min_set = 4, exact inliers: the call returns the true inlier set and the yardstick's refined pose on it.
  plumbing      batch against single calls, determinism, buffer reuse across sizes, four threads, invalid arguments.
Every bound comes from tests/pnp_solver_tolerances.py."""
import os
import threading

import numpy as np
import pytest

import pnp_solver_reference as Y
import pnp_solver_scenes as SC
from pnp_solver_tolerances import MARGIN_REL, REP_BAND, RT_BOUND

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [name for name, _ in SC.all_families()]
GOLDEN = sorted(f[:-4] for f in os.listdir(os.path.join(ROOT, "tests", "golden", "pnp_solver")) if f.endswith(".npz"))
_cache = {}


def _chunks(c):
    sizes = c.get("chunks", (len(c["sets"]),))
    o, out = 0, []
    for s in sizes:
        out.append(c["sets"][o:o + s])
        o += s
    return out


def _case(name):
    """(case, [(state before, sets, device output)] per consecutive call), computed once and left unchanged"""
    if name not in _cache:
        from eao_fusion_amd.pnp_solver import new_state, pnp_solver_iterate
        c = SC.FAMILIES[name]()
        st, calls = new_state(len(c["prob"]["sigma2"])), []
        for sets in _chunks(c):
            dev = pnp_solver_iterate(c["prob"], st, sets, c["min_inliers"], c["max_its"], inspect=True)
            calls.append((st, sets, dev))
            st = dev["state"]
        _cache[name] = (c, calls)
    return _cache[name]


def result_bytes(o):
    keys = ["returned", "refined", "n_inliers", "Tcw", "inlier", "no_more", "n_records"]
    keys += [k for k in sorted(o) if k.startswith("hyp_") or k.startswith("rec_")]
    b = b"".join(np.ascontiguousarray(o[k]).tobytes() for k in keys)
    s = o["state"]
    return b + b"".join(np.ascontiguousarray(s[k]).tobytes() for k in ("iterations", "best_inliers", "best_Tcw", "best_inlier"))


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_replay(name):
    c, calls = _case(name)
    prob, n = c["prob"], len(c["prob"]["sigma2"])
    for st, sets, dev in calls:
        nh = len(sets)
        if n < c["min_inliers"]:
            assert dev["no_more"] and dev["returned"] == -1 and dev["n_records"] == 0 and not dev["hyp_inliers"].any()
            assert all(np.array_equal(dev["state"][k], st[k]) for k in st), "the state is untouched"
            continue
        # CheckInliers on the device's own poses: flags and counts bit for bit
        for k in range(nh):
            f = Y.check_inliers(dev["hyp_R"][k], dev["hyp_t"][k], prob)
            assert np.array_equal(f, dev["hyp_inlier"][k] > 0), (name, k)
            assert int(f.sum()) == int(dev["hyp_inliers"][k])
            rep = dev["hyp_rep_err"][k]
            N = 1
            if rep[1] < rep[0]:
                N = 2
            if rep[2] < rep[N - 1]:
                N = 3
            assert N == int(dev["hyp_choice"][k]), (name, k, rep)
        sources = []
        for j in range(dev["n_records"]):
            f = Y.check_inliers(dev["rec_R"][j], dev["rec_t"][j], prob)
            assert np.array_equal(f, dev["rec_inlier"][j] > 0) and int(f.sum()) == int(dev["rec_inliers"][j]), (name, j)
            h = int(dev["rec_hyp"][j])
            sources.append(np.asarray(st["best_inlier"] if h < 0 else dev["hyp_inlier"][h], np.uint8))

        def refine_of(flags):
            for j, src in enumerate(sources):
                if np.array_equal(src, flags):
                    return int(dev["rec_inliers"][j]) > c["min_inliers"], Y.to_Tcw(dev["rec_R"][j], dev["rec_t"][j]), dev["rec_inlier"][j], int(dev["rec_inliers"][j])
            raise AssertionError("the rule asks for Refine of a set the device did not refine")

        rule = Y.sequential_rule(n, dev["hyp_inliers"], dev["hyp_inlier"], [Y.to_Tcw(dev["hyp_R"][k], dev["hyp_t"][k]) for k in range(nh)], refine_of, st,
                                 c["min_inliers"], c["max_its"])
        assert [int(h) for h in dev["rec_hyp"] if h >= 0] == rule["records"]
        assert int(dev["rec_hyp"][0]) == -1 if (st["best_inliers"] > 0 and dev["n_records"]) else True
        for k in ("returned", "refined", "n_inliers", "no_more"):
            assert int(dev[k]) == int(rule[k]), (name, k, dev[k], rule[k])
        assert dev["Tcw"].tobytes() == rule["Tcw"].tobytes()
        if dev["returned"] >= 0:
            assert np.array_equal(dev["inlier"], np.asarray(rule["inlier"], np.uint8))
        for k in ("iterations", "best_inliers"):
            assert dev["state"][k] == rule["state"][k], (name, k)
        assert dev["state"]["best_Tcw"].tobytes() == rule["state"]["best_Tcw"].tobytes()
        assert np.array_equal(dev["state"]["best_inlier"], rule["state"]["best_inlier"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", [g for g in GOLDEN if g in SC.PARITY])
def test_hypothesis_parity(name):
    """min_set >= 6: poses within RT_BOUND on conditioned hypotheses, flags equal outside MARGIN_REL, the same choice where it is decided, the same outcome."""
    c, calls = _case(name)
    _, _, dev = calls[0]
    z = np.load(os.path.join(ROOT, "tests", "golden", "pnp_solver", name + ".npz"))
    assert np.array_equal(z["sets"], c["sets"]) and np.array_equal(z["p3d_w"], c["prob"]["p3d_w"]), "the golden file is of another scene: tools/gen_golden_pnp_solver.py"
    cond = z["conditioned"] > 0
    assert cond.any()
    gate = Y.max_error(c["prob"]).astype(np.float64)
    for k in np.flatnonzero(cond):
        d = max(np.abs(dev["hyp_R"][k] - z["hyp_R"][k]).max(), np.abs(dev["hyp_t"][k] - z["hyp_t"][k]).max())
        assert d <= RT_BOUND, (name, k, d)
        clear = np.abs(z["hyp_err"][k] - gate) > MARGIN_REL * gate
        assert np.array_equal(dev["hyp_inlier"][k][clear], z["hyp_inlier"][k][clear]), (name, k)
        rep = np.sort(z["hyp_rep_err"][k])
        if rep[1] - rep[0] > REP_BAND:
            assert int(dev["hyp_choice"][k]) == int(z["hyp_choice"][k]), (name, k)
    assert (dev["returned"], dev["refined"], int(dev["no_more"])) == (int(z["returned"]), int(z["refined"]), int(z["no_more"]))
    assert [int(h) for h in dev["rec_hyp"] if h >= 0] == list(z["records"])
    assert dev["state"]["iterations"] == int(z["iterations"])
    if dev["returned"] >= 0:
        assert np.abs(dev["Tcw"].astype(np.float64) - z["Tcw"]).max() <= RT_BOUND
        clear = np.ones(len(gate), bool)
        if dev["refined"] == 0:
            clear = np.abs(z["hyp_err"][dev["returned"]] - gate) > MARGIN_REL * gate
        assert np.array_equal(dev["inlier"][clear], z["inlier"][clear])


def _well_posed(prob, idx):
    """at least six points that do not lie in a plane (the smallest singular value of the centred points against the largest)"""
    if len(idx) < 6:
        return False
    X = np.asarray(prob["p3d_w"], np.float64)[idx]
    s = np.linalg.svd(X - X.mean(axis=0), compute_uv=False)
    return bool(s[2] > 1e-3 * s[0])


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_refine_parity(name):
    """Refine's compute_pose on the device's OWN inlier set against the yardstick's on that set: n is large there and the problem is conditioned, at min_set = 4 too."""
    c, calls = _case(name)
    compared = 0
    for st, sets, dev in calls:
        for j in range(dev["n_records"]):
            h = int(dev["rec_hyp"][j])
            idx = np.flatnonzero(st["best_inlier"] if h < 0 else dev["hyp_inlier"][h])
            if not _well_posed(c["prob"], idx):
                continue
            R, t, _, _ = Y.pose_of(c["prob"], idx, "jacobi")
            d = max(np.abs(dev["rec_R"][j] - R).max(), np.abs(dev["rec_t"][j] - t).max())
            assert d <= RT_BOUND, (name, j, d)
            compared += 1
    expect = {"x6_n63", "n6_n64", "x8_n65", "n8_n257", "x4_n100", "n4_n100", "x4_n257", "n4_n63", "repeat_n65", "fail_then_succeed", "carried", "carried_success"}
    assert compared > 0 or name not in expect, "no record was compared"


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["x4_n100", "x4_n257"])
def test_outcome_min4_exact(name):
    """min_set = 4, exact inliers and gross outliers: whatever basis the eigen-solver hands back, the call returns the true inlier set and its refined pose."""
    c, calls = _case(name)
    _, _, dev = calls[0]
    assert dev["returned"] >= 0 and dev["refined"] == 1
    assert np.array_equal(dev["inlier"] > 0, c["true_inlier"])
    R, t, _, _ = Y.pose_of(c["prob"], np.flatnonzero(c["true_inlier"]), "jacobi")
    assert np.abs(dev["Tcw"].astype(np.float64) - Y.to_Tcw(R, t)).max() <= RT_BOUND
    assert max(np.abs(R - c["R_true"]).max(), np.abs(t - c["t_true"]).max()) <= 1e-4, "the scene's planted pose"


BATCH = ["x6_n63", "x4_n100", "n8_n257", "x6_n6", "n8_n9_below_min", "coplanar_n65", "n4_n63", "fail_then_succeed", "n6_n64", "x8_n65", "zero_depth_n64", "repeat_n65",
         "all_outliers_n64", "x4_n257", "n8_n10_at_min", "n4_n100"]


@pytest.mark.gpu
def test_batch_equals_single_calls():
    """sixteen problems of mixed N and min_set through the batch entry point: byte for byte what the single calls return; and a second call gives the same bytes"""
    from eao_fusion_amd.pnp_solver import pnp_solver_iterate_batch
    cs = [SC.FAMILIES[name]() for name in BATCH]
    first = [_chunks(c)[0] for c in cs]
    args = ([c["prob"] for c in cs], [None] * len(cs), first, [c["min_inliers"] for c in cs], [c["max_its"] for c in cs])
    outs = pnp_solver_iterate_batch(*args, inspect=True)
    again = pnp_solver_iterate_batch(*args, inspect=True)
    for name, o, a in zip(BATCH, outs, again):
        single = _case(name)[1][0][2]
        assert result_bytes(o) == result_bytes(single), name
        assert result_bytes(o) == result_bytes(a), name


def _run(name, out, slot):
    from eao_fusion_amd.pnp_solver import pnp_solver_iterate
    c = SC.FAMILIES[name]()
    out[slot] = result_bytes(pnp_solver_iterate(c["prob"], None, _chunks(c)[0], c["min_inliers"], c["max_its"], inspect=True))


@pytest.mark.gpu
def test_size_sequence_on_one_thread_and_four_threads():
    """257 -> 6 -> 65 -> 257 on one thread (its staging block and device arena are reused across sizes) against fresh threads; then four threads at once"""
    seq = ["n8_n257", "x6_n6", "x8_n65", "n8_n257"]
    expect = [result_bytes(_case(name)[1][0][2]) for name in seq]
    got = [None] * 4

    def one_thread():
        for i, name in enumerate(seq):
            _run(name, got, i)

    t = threading.Thread(target=one_thread)
    t.start()
    t.join()
    assert got == expect
    fresh = [None] * 4
    for i, name in enumerate(seq):
        t = threading.Thread(target=_run, args=(name, fresh, i))
        t.start()
        t.join()
    assert fresh == expect
    par = [None] * 4
    ts = [threading.Thread(target=_run, args=(name, par, i)) for i, name in enumerate(seq)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert par == expect


@pytest.mark.gpu
def test_invalid_arguments_fail_with_nothing_written():
    from eao_fusion_amd import _lib
    from eao_fusion_amd.pnp_solver import new_state, pnp_solver_iterate, pnp_solver_iterate_batch
    c = SC.FAMILIES["x6_n63"]()
    n = 63
    good = c["sets"][:4]

    def fails(prob, sets, state=None, min_inliers=c["min_inliers"]):
        with pytest.raises(_lib.EaoError) as e:
            pnp_solver_iterate(prob, state, sets, min_inliers, c["max_its"])
        assert e.value.status == _lib.EAO_ERR_INVALID

    bad = good.copy()
    bad[2, 3] = n
    fails(c["prob"], bad)
    bad[2, 3] = -1
    fails(c["prob"], bad)
    fails(c["prob"], np.zeros((2, 3), np.int32))        # min_set < 4
    fails(c["prob"], np.zeros((2, 65), np.int32))       # min_set > 64
    for key in ("p3d_w", "p2d", "sigma2"):
        p = dict(c["prob"])
        p[key] = np.array(p[key], np.float32)
        p[key].reshape(-1)[5] = np.nan
        fails(p, good)
    fails(dict(c["prob"], K=(np.inf, 525.0, 320.0, 240.0)), good)
    small = dict(c["prob"], p3d_w=c["prob"]["p3d_w"][:5], p2d=c["prob"]["p2d"][:5], sigma2=c["prob"]["sigma2"][:5])
    fails(small, np.zeros((1, 6), np.int32), min_inliers=4)       # n < min_set
    st = new_state(n)
    st["best_inliers"] = 3                                   # not the size of best_inlier
    fails(c["prob"], good, state=st)
    # a batch with one invalid problem: the call fails
    with pytest.raises(_lib.EaoError):
        pnp_solver_iterate_batch([c["prob"], c["prob"]], [None, None], [good, bad], c["min_inliers"], c["max_its"])
    # nothing written: the C structs of a failing call keep their bytes
    import ctypes as C
    from eao_fusion_amd import pnp_solver as PS
    P, S, R = _lib.PnpSolverProblem(), _lib.PnpSolverState(), _lib.PnpSolverResult()
    keep, _, nh, ms = PS._pack(c["prob"], None, bad, True, P, S, R)
    C.memset(C.byref(R, 0), 0x5A, 12)
    S.iterations = 7
    before = (bytes(R), bytes(S), {k: v.tobytes() for k, v in keep.items()})
    assert _lib.load().eao_pnp_solver_iterate(C.byref(P), c["min_inliers"], c["max_its"], ms, C.byref(S), _lib.ptr(keep["sets"]), nh, C.byref(R)) == _lib.EAO_ERR_INVALID
    assert before == (bytes(R), bytes(S), {k: v.tobytes() for k, v in keep.items()})


@pytest.fixture(scope="module")
def class_driver(tmp_path_factory):
    import subprocess
    exe = str(tmp_path_factory.mktemp("pnp_solver") / "pnp_solver_driver")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-DEAOFUSION_FORCE_CV_COMPAT", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "pnp_solver", "pnp_solver_driver.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "eao_fusion_amd"), "-leaofusion_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "eao_fusion_amd"), "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    return exe


@pytest.mark.gpu
def test_class_surface_relocalizes(class_driver):
    """Relocalization's loop (src/Tracking.cc:2847-2940) over three candidates through include/eaofusion/PnPsolver.h with a seeded stand-in generator: one has fewer
    correspondences than min_inliers (discarded without a draw), one is all outliers (its first iterate(5) runs all 35 hypotheses -- the || -- and ends with bNoMore),
    one returns its refined pose in the first round, which goes on to PoseOptimization over its inliers and ends the search.  Draws, pose and inliers are what the
    Python entry point gives over the same draw stream."""
    import subprocess
    import pnp_solver_frames as FR
    from eao_fusion_amd.pnp_solver import pnp_solver_iterate
    seed = 20240607
    cases = [SC.case(9, 7, 4, 1, noise_px=1.0, outlier_frac=0.0), SC.case(64, 33, 4, 1, outlier_frac=1.0), SC.FAMILIES["x4_n100"]()]
    texts = [FR.candidate_text(c["prob"], seed=50 + i) for i, c in enumerate(cases)]
    out = subprocess.run([class_driver, "loop"], input="3 %d\n" % seed + "".join(t[0] for t in texts), capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().split("\n")
    its = [ln.split() for ln in lines if " iterate " in ln]
    assert [(int(w[1]), int(w[3])) for w in its] == [(1, 0), (1, 1), (1, 2)]
    f = lambda w, key, count=1: w[w.index(key) + 1] if count == 1 else w[w.index(key) + 1:w.index(key) + 1 + count]
    assert (int(f(its[0], "draws")), int(f(its[0], "nomore")), f(its[0], "mat")) == (0, 1, "empty")
    assert (int(f(its[1], "draws")), int(f(its[1], "nomore")), f(its[1], "mat")) == (35 * 4, 1, "empty")
    lcg = FR.Lcg(seed)
    FR.draw_sets(lcg, 64, 4, 35)
    c, (_, index, total) = cases[2], texts[2]
    mi, mx = Y.ransac_parameters(100, *SC.RELOCALIZATION)
    dev = pnp_solver_iterate(c["prob"], None, FR.draw_sets(lcg, 100, 4, 35), mi, mx)
    assert dev["returned"] >= 0 and dev["refined"] == 1
    assert (int(f(its[2], "draws")), int(f(its[2], "nomore")), int(f(its[2], "ninl")), int(f(its[2], "size"))) == (35 * 4, 0, dev["n_inliers"], total)
    assert np.array(f(its[2], "mat", 16), np.float32).tobytes() == dev["Tcw"].tobytes()
    assert [int(v) for v in its[2][its[2].index("inliers") + 1:]] == [index[i] for i in np.flatnonzero(dev["inlier"])]
    pose = [ln.split() for ln in lines if ln.startswith("pose ")]
    assert len(pose) == 1 and int(f(pose[0], "ngood")) >= 50
    T = np.array(f(pose[0], "T", 16), np.float64).reshape(4, 4)
    assert max(np.abs(T[:3, :3] - c["R_true"]).max(), np.abs(T[:3, 3] - c["t_true"]).max()) <= 1e-3
    assert lines[-2] == "match candidate 2" and lines[-1] == "done match 1 rounds 1"
