"""Optimizer::OptimizeEssentialGraph on the device (eao_optimize_essential_graph, csrc/essential_graph.hip) against the numpy restatement
tests/essential_graph_reference.py on the families of essential_graph_scenes.CASES (each with fix_scale 0 and 1), the golden fixtures of the
300-keyframe ring, the map-point pass at several sizes, determinism across calls and host threads, and the argument checks.  Every bound comes
from tests/lm_tolerances.py and tests/essential_graph_tolerances.py."""
import functools
import os
import threading

import numpy as np
import pytest

import essential_graph_reference as R
import essential_graph_scenes as SC
from essential_graph_tolerances import DERIVED_FLOAT_ULPS, chi2_last_rel
from lm_tolerances import CHAOTIC_BANDS_ALLOWED, UPDATE_REL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "essential_graph")


@functools.lru_cache(maxsize=None)
def _case(name, fs):
    return SC.case(name, fs)


@functools.lru_cache(maxsize=None)
def _reference(name, fs):
    """The yardstick's result of a case, computed once; the 300-keyframe ring comes from its golden file (tools/gen_golden_essential_graph.py; the CPU suite
    re-derives it)."""
    fn = os.path.join(GOLDEN, "%s_fs%d.npz" % (name, int(fs)))
    if os.path.exists(fn):
        z = np.load(fn)
        prob = _case(name, fs)
        assert np.array_equal(z["Scw_in"], prob["Scw"]) and np.array_equal(z["edges"], prob["edges"]), "golden file of another scene: " + fn
        rows = z["Scw"]
        return dict(Scw=rows, lm_iterations=int(z["lm_iterations"]), trials=z["trials"], chi2=z["chi2"], chi2_initial=float(z["chi2_initial"]),
                    n_active=int(z["n_active"]))
    return R.optimize_essential_graph(_case(name, fs))


def _quat_aligned(q, qref):
    """q with the sign that brings it closest to qref, per keyframe."""
    sgn = np.where(np.sum(q * qref, axis=1, keepdims=True) < 0, -1.0, 1.0)
    return q * sgn


def _displacement(a, b):
    return max(np.abs(_quat_aligned(a[:, :4], b[:, :4]) - b[:, :4]).max(), np.abs(a[:, 4:] - b[:, 4:]).max())


def _within_float_ulps(a, b, ulps):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return bool(np.all(np.abs(a.astype(np.float64) - b.astype(np.float64)) <= ulps * np.spacing(np.maximum(np.abs(a), np.abs(b))).astype(np.float64)))


def _assert_derived(prob, got):
    """Tiw and Xw_corrected against their recomputation from the device's own Scw; points without a reference bit for bit."""
    assert _within_float_ulps(got["Tiw"], R.recover_poses(got["Scw"]), DERIVED_FLOAT_ULPS)
    want = R.correct_points(np.asarray(prob["Scw"], np.float64), got["Scw"], prob["Xw"], prob["ref"])
    assert got["Xw_corrected"].shape == want.shape
    assert _within_float_ulps(got["Xw_corrected"], want, DERIVED_FLOAT_ULPS)
    none = np.asarray(prob["ref"]) < 0
    assert np.array_equal(got["Xw_corrected"][none].view(np.uint32), np.asarray(prob["Xw"], np.float32)[none].view(np.uint32))


def _assert_parity(prob, ref, got, cid):
    rows_in = np.asarray(prob["Scw"], np.float64)
    upd = float(np.abs(ref["Scw"] - rows_in).max())
    tol = UPDATE_REL * upd
    if cid in SC.BANDED:      # (the rule of test_gpu_sim3.py's banded families; the table is empty today)
        band = max(_displacement(R.optimize_essential_graph(SC.ulp_perturbed(prob, s))["Scw"], ref["Scw"]) for s in range(4))
        assert band > UPDATE_REL * upd, "not a banded case: hold it to UPDATE_REL"
        tol = CHAOTIC_BANDS_ALLOWED * band
    d = _displacement(got["Scw"], ref["Scw"])
    CHI2_LAST_REL = chi2_last_rel(cid)
    chi_rel = abs(got["chi2"][-1] - ref["chi2"][-1]) / ref["chi2"][-1]
    print("\n[essential graph %s] GPU - yardstick %.3e of an update of %.3e (bound %.3e); iterations %d / %d, trials %s / %s; last chi2 off by %.3e (bound %.3e)"
          % (cid, d, upd, tol, got["lm_iterations"], ref["lm_iterations"], list(got["trials"]), list(ref["trials"]), chi_rel, CHI2_LAST_REL))
    assert d <= tol
    G = R.Graph(prob)
    untouched = np.ones(prob["n"], bool)
    untouched[G.free] = False
    assert untouched[prob["fixed"]]
    assert np.array_equal(got["Scw"][untouched].view(np.uint64), rows_in[untouched].view(np.uint64))      # the fixed vertex and those without an edge
    if prob["fix_scale"]:
        assert np.array_equal(got["Scw"][:, 7].view(np.uint64), rows_in[:, 7].view(np.uint64))
    assert got["n_active"] == ref["n_active"] == int(G.active.sum())
    if cid not in SC.ITERS_UNSTABLE:
        assert got["lm_iterations"] == ref["lm_iterations"] and list(got["trials"]) == list(ref["trials"])
    assert got["chi2_initial"] == pytest.approx(ref["chi2_initial"], rel=CHI2_LAST_REL)
    assert chi_rel <= CHI2_LAST_REL
    _assert_derived(prob, got)


@pytest.mark.gpu
@pytest.mark.parametrize("name,fs", SC.CASES, ids=SC.case_ids())
def test_essential_graph_parity(name, fs):
    from eao_fusion_amd.optimizer import essential_graph_plan, optimize_essential_graph
    prob = _case(name, fs)
    got = optimize_essential_graph(prob)
    _assert_parity(prob, _reference(name, fs), got, "%s-fs%d" % (name, int(fs)))
    if name == "isolated":
        v = prob["isolated"]
        assert got["n_active"] == prob["n"] - 1
        assert np.array_equal(got["Scw"][v].view(np.uint64), np.asarray(prob["Scw"], np.float64)[v].view(np.uint64))
        assert prob["ref"][2] == v and np.array_equal(got["Xw_corrected"][2], prob["Xw"][2])      # a point referenced to it is unchanged
    plan = essential_graph_plan(prob)      # (the plan the call above ran on: a pure function of the problem)
    if name == "ring300":      # the solver's multi-segment path ran: several segments, a separator block behind them
        assert plan["segments"] > 1 and plan["separators"] > 0, plan
    if name in ("ring9", "ring10"):
        assert plan["rows"] == 64 and plan["segments"] == 1, plan


@pytest.mark.gpu
@pytest.mark.parametrize("fs", [False, True], ids=["fs0", "fs1"])
@pytest.mark.parametrize("n_points", SC.POINT_COUNTS)
def test_essential_graph_points(n_points, fs):
    """The map-point pass at 0, 1, 63, 65 and 5000 points, references -1 and the fixed keyframe among them; the poses do not depend on the points."""
    from eao_fusion_amd.optimizer import optimize_essential_graph
    base = _case("ring40", fs)
    prob = SC.with_points(base, n_points, seed=500 + n_points)
    got = optimize_essential_graph(prob)
    assert got["Xw_corrected"].shape == (n_points, 3)
    _assert_derived(prob, got)
    if n_points > 1:
        assert prob["ref"][0] == -1 and prob["ref"][1] == prob["fixed"]
        assert np.array_equal(got["Xw_corrected"][1], prob["Xw"][1])      # through the fixed keyframe and back: the same float
    assert got["Scw"].tobytes() == optimize_essential_graph(base)["Scw"].tobytes()


def _bytes(o):
    return b"".join([o["Scw"].tobytes(), o["Tiw"].tobytes(), o["Xw_corrected"].tobytes(), np.int32(o["lm_iterations"]).tobytes(), o["trials"].tobytes(),
                     o["lambda"].tobytes(), o["chi2"].tobytes(), np.float64(o["chi2_initial"]).tobytes()])


@pytest.mark.gpu
def test_essential_graph_same_bytes_twice_and_after_another_problem():
    from eao_fusion_amd.optimizer import optimize_essential_graph
    a, b, c = _case("ring66", False), _case("hub", True), _case("dup2", False)
    first = [_bytes(optimize_essential_graph(p)) for p in (a, a, b, c)]
    assert first[0] == first[1]
    again = [_bytes(optimize_essential_graph(p)) for p in (c, b, a)]      # each after a different problem, larger and smaller, on the same thread
    assert again == [first[3], first[2], first[0]]


@pytest.mark.gpu
def test_essential_graph_two_host_threads():
    """Two host threads (each with its own context and stream) on two different graphs at once: the same bytes as single-threaded."""
    from eao_fusion_amd.optimizer import optimize_essential_graph
    probs = [_case("ring65", True), _case("edges257", False)]
    single = [_bytes(optimize_essential_graph(p)) for p in probs]
    out = [None, None]

    def work(k):
        out[k] = [_bytes(optimize_essential_graph(probs[k])) for _ in range(3)]

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for k in range(2):
        assert out[k] == [single[k]] * 3


@pytest.mark.gpu
def test_essential_graph_bad_arguments():
    """The error code, the message, and nothing written."""
    from eao_fusion_amd import _lib
    from eao_fusion_amd.optimizer import optimize_essential_graph
    good = _case("ring10", False)

    def broken(**kw):
        p = dict(good)
        p.update(kw)
        return p

    nan_scw = np.array(good["Scw"]); nan_scw[3, 5] = np.nan
    inf_snc = np.array(good["Snc"]); inf_snc[9, 0] = np.inf      # (keyframe 9 carries a NonCorrectedSim3)
    nan_x = np.array(good["Xw"]); nan_x[4, 1] = np.nan
    e_range = np.array(good["edges"]); e_range[2, 1] = 10
    e_neg = np.array(good["edges"]); e_neg[0, 0] = -1
    e_self = np.array(good["edges"]); e_self[5, 1] = e_self[5, 0]
    assert good["has_nc"][9]
    cases = [(broken(Scw=nan_scw), "non-finite Scw"), (broken(Snc=inf_snc), "non-finite Snc"), (broken(Xw=nan_x), "non-finite map point"),
             (broken(fixed=10), "fixed = 10"), (broken(fixed=-1), "fixed = -1"), (broken(edges=e_range), "edge 2 links"), (broken(edges=e_neg), "edge 0 links"),
             (broken(edges=e_self), "to itself")]
    for p, msg in cases:
        with pytest.raises(_lib.EaoError) as ei:
            optimize_essential_graph(p)
        assert ei.value.status == _lib.EAO_ERR_INVALID and msg in str(ei.value), str(ei.value)
    # nothing written: the caller's buffers keep their bytes
    import ctypes as C
    Scw, Snc = np.ascontiguousarray(nan_scw), np.ascontiguousarray(good["Snc"])
    has, edges = np.ascontiguousarray(good["has_nc"], np.uint8), np.ascontiguousarray(good["edges"], np.int32)
    Xw, ref = np.ascontiguousarray(good["Xw"], np.float32), np.ascontiguousarray(good["ref"], np.int32)
    P = _lib.EssentialGraphProblem(10, 0, 0, _lib.ptr(Scw), _lib.ptr(has), _lib.ptr(Snc), len(edges), _lib.ptr(edges), len(Xw), _lib.ptr(Xw), _lib.ptr(ref))
    oS, oT, oX = np.full((10, 8), 7.0), np.full((10, 16), 7.0, np.float32), np.full((len(Xw), 3), 7.0, np.float32)
    Rr = _lib.EssentialGraphResult()
    Rr.Scw, Rr.Tiw, Rr.Xw_corrected = _lib.ptr(oS), _lib.ptr(oT), _lib.ptr(oX)
    Rr.lm_iterations = -5
    assert _lib.load().eao_optimize_essential_graph(C.byref(P), C.byref(Rr)) == _lib.EAO_ERR_INVALID
    assert np.all(oS == 7.0) and np.all(oT == 7.0) and np.all(oX == 7.0) and Rr.lm_iterations == -5
    assert optimize_essential_graph(good)["lm_iterations"] > 0      # and the thread's context is as usable as before


@pytest.fixture(scope="module")
def class_driver(tmp_path_factory):
    import subprocess
    exe = str(tmp_path_factory.mktemp("essential_graph") / "essential_graph_driver")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-DESSENTIAL_GRAPH_RUN", "-DEAOFUSION_FORCE_CV_COMPAT", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "essential_graph", "essential_graph_driver.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "eao_fusion_amd"), "-leaofusion_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "eao_fusion_amd"), "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    return exe


@pytest.mark.gpu
@pytest.mark.parametrize("fs", [False, True])
def test_essential_graph_class_surface(class_driver, fs):
    """include/eaofusion/OptimizerEssentialGraph.h over the stand-ins of tests/cpp/essential_graph/, linked against the library, against the Python path on the same
    flattened graph: poses and points byte-equal, SetPose / SetWorldPos / UpdateNormalAndDepth called as often as the reference's loops call them."""
    import subprocess
    from eao_fusion_amd.optimizer import optimize_essential_graph
    m, text, want = SC.hand_built_map(fs)
    walk = subprocess.run([class_driver, "walk"], input=text, capture_output=True, text=True, check=True).stdout
    prob = SC.problem_of_walk(walk)
    assert [tuple(e) for e in prob["edges"]] == want["edges"]
    got = optimize_essential_graph(prob)
    assert got["lm_iterations"] > 0 and np.abs(got["Scw"] - prob["Scw"]).max() > 0
    lines = subprocess.run([class_driver, "run"], input=text, capture_output=True, text=True, check=True).stdout.strip().split("\n")
    kf = [ln.split()[1:] for ln in lines if ln.startswith("kf ")]
    mp = [ln.split()[1:] for ln in lines if ln.startswith("mp ")]
    pl = [ln.split()[1:] for ln in lines if ln.startswith("pl ")]
    assert "lists 3" in lines      # GetAllKeyFrames / GetAllMapPoints / GetAllMapPlanes once each: the write-back uses the vectors of the walk
    assert len(kf) == len(m["kfs"]) and len(mp) == len(m["points"]) and len(pl) == len(m["planes"])
    v = 0
    for rec, k in zip(kf, m["kfs"]):
        T = np.array([float(x) for x in rec[1:]], np.float32)
        if k["bad"]:
            assert int(rec[0]) == 0 and np.array_equal(T, np.asarray(k["T"], np.float32).ravel())      # no vertex: never touched
            continue
        assert int(rec[0]) == 1 and T.tobytes() == got["Tiw"][v].tobytes()
        v += 1
    assert v == prob["n"]
    row = 0
    for rec, (x, bad, _, _, _) in zip(mp, m["points"]):
        X = np.array([float(c) for c in rec[3:]], np.float32)
        if bad:
            assert rec[:2] == ["0", "0"] and np.array_equal(X, np.array(x, np.float32))
            continue
        assert rec[:3] == ["1", "1", "3"] and X.tobytes() == got["Xw_corrected"][row].tobytes()
        row += 1
    for rec, (x, bad, _, _, _) in zip(pl, m["planes"]):
        X = np.array([float(c) for c in rec[2:]], np.float32)
        if bad:
            assert rec[:2] == ["0", "4"] and np.array_equal(X, np.array(x[:3], np.float32))
            continue
        assert rec[:2] == ["1", "3"] and X.tobytes() == got["Xw_corrected"][row].tobytes()      # SetWorldPos with three entries, as the fork wrote it
        row += 1
    assert row == len(prob["ref"])
