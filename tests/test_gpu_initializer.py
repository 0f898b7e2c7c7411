"""Initializer on the device (eao_initializer_initialize, csrc/initializer.hip) against the numpy restatement tests/initializer_reference.py on the families of
tests/initializer_scenes.py and the golden fixtures tests/golden/initializer/*.npz.  Every bound comes from tests/initializer_tolerances.py.

Group A: the yardstick's matrices on conditioned hypotheses.  Group B: the replay, bit for bit, of every later step on the device's OWN values (no tolerance).
Group C: the yardstick's outcome on the friendly families.  The 4 / 8 motion hypotheses are matched as a set: their order follows the SVD's signs.
The yardstick's arithmetic choices (OpenCV's own arithmetic is not in the reference tree): see the docstring of tests/initializer_reference.py."""
import ctypes as C
import glob
import os
import subprocess
import threading

import numpy as np
import pytest

import initializer_reference as R
import initializer_scenes as SC
from initializer_tolerances import GAP_MIN, HF_REL, MARGIN_REL, RT_REL, X3D_REL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRIENDLY = list(SC.FRIENDLY)
ALL = FRIENDLY + list(SC.IRREGULAR)
_cache = {}


def _problem(name):
    return SC.workload() if name == "workload" else SC.friendly(name) if name in SC.FRIENDLY else SC.irregular(name)


def _case(name):
    """(problem, packed pairs, yardstick, device with everything inspected), computed once and left unchanged"""
    if name not in _cache:
        from eao_fusion_amd.initializer import initialize
        prob = _problem(name)
        ref = R.initialize(prob, prob["sets"], "f64jacobi")
        dev = initialize(prob, prob["sets"], inspect=True)
        _cache[name] = (prob, ref["pk"], ref, dev)
    return _cache[name]


def _eq(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def _hf_dist(a, b):
    ua, ub = R.unit(a).reshape(len(a), -1), R.unit(b).reshape(len(b), -1)
    return np.minimum(np.abs(ua - ub).max(1), np.abs(ua + ub).max(1))


def _motion_dist(Ra, ta, Rb, tb):
    return max(float(np.abs(np.asarray(Ra, np.float64) - Rb).max()), float(np.abs(np.asarray(ta, np.float64) - tb).max()))


# ---------------------------------------------------------------------- Group A
@pytest.mark.gpu
@pytest.mark.parametrize("name", FRIENDLY)
def test_conditioned_matrices(name):
    """H21i / F21i of conditioned hypotheses within HF_REL of the yardstick's (unit Frobenius norm, the sign free)."""
    prob, pk, ref, dev = _case(name)
    for key, gap in (("H21", "gap_h"), ("F21", "gap_f")):
        cond = ref["hyp"][gap] >= GAP_MIN
        d = _hf_dist(dev["hyp_" + key][cond], ref["hyp"][key][cond])
        print(name, key, "conditioned %d of %d, largest distance %.3e (HF_REL %.3e)" % (cond.sum(), len(cond), d.max() if len(d) else 0.0, HF_REL))
        assert np.isfinite(dev["hyp_" + key][cond]).all() and (d <= HF_REL).all()


# ---------------------------------------------------------------------- Group B
@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL)
def test_replay_scores_and_selection(name):
    """Flags and double-sum scores of every hypothesis equal CheckHomography / CheckFundamental on the device's own H21 / H12 / F21; H12 is the inverse rule applied to
    the device's H21; the winners are the first argmax of the device's scores; RH and the branch follow from its SH and SF."""
    prob, pk, ref, dev = _case(name)
    sigma = prob["sigma"]
    assert _eq(dev["hyp_H12"], R.inv3(dev["hyp_H21"]))
    for b in range(len(prob["sets"])):
        fl, sc, _ = R.check_homography(dev["hyp_H21"][b], dev["hyp_H12"][b], pk["raw"], sigma)
        assert _eq(fl, dev["hyp_inlier_H"][b] > 0) and _eq(sc, dev["hyp_SH"][b]), (b, sc, dev["hyp_SH"][b])
        fl, sc, _ = R.check_fundamental(dev["hyp_F21"][b], pk["raw"], sigma)
        assert _eq(fl, dev["hyp_inlier_F"][b] > 0) and _eq(sc, dev["hyp_SF"][b]), (b, sc, dev["hyp_SF"][b])
    bh, SH = R.first_argmax(dev["hyp_SH"])
    bf, SF = R.first_argmax(dev["hyp_SF"])
    assert (dev["best_h"], dev["best_f"]) == (bh, bf) and _eq(dev["SH"], SH) and _eq(dev["SF"], SF)
    RH, branch = R.choose(SH, SF)
    assert _eq(dev["RH"], RH) and dev["branch"] == branch
    win = bh if branch == R.BRANCH_H else bf
    assert dev["no_model"] == (win < 0)
    if win >= 0:
        assert _eq(dev["H21"], dev["hyp_H21"][bh] if bh >= 0 else np.zeros((3, 3))) and _eq(dev["F21"], dev["hyp_F21"][bf] if bf >= 0 else np.zeros((3, 3)))
        flags = (dev["hyp_inlier_H"] if branch == R.BRANCH_H else dev["hyp_inlier_F"])[win]
        assert _eq(dev["inlier"], flags) and dev["n_inliers"] == int(flags.sum())
    else:
        assert not dev["returned"] and dev["n_motions"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL)
def test_replay_check_rt_and_final_rule(name):
    """CheckRT's good / n_good / selected cosine equal the yardstick's gates applied to the device's own R, t and p3d; pairs the device rejects are rejected by the
    yardstick's own triangulation unless they lie inside MARGIN_REL of a gate; the final rule on the device's own counts and cosines gives its returned, R21, t21."""
    prob, pk, ref, dev = _case(name)
    n1, first, inl = pk["n1"], pk["first"], dev["inlier"] > 0
    assert dev["n_motions"] == (0 if dev["no_model"] or dev["degenerate"] else 8 if dev["branch"] == R.BRANCH_H else 4)
    pars = []
    for m in range(dev["n_motions"]):
        Rm, tm = dev["mot_R"][m], dev["mot_t"][m]
        X = dev["mot_p3d"][m][first]
        acc = (X != 0).any(1)
        assert not (acc & ~inl).any()
        own = R.check_rt(pk["raw"], first, inl, Rm, tm, prob["K"], prob["sigma"], n1, "f64jacobi")
        differ = acc != own["accepted"]
        assert (own["margin"][differ] < MARGIN_REL).all(), (m, np.nonzero(differ)[0], own["margin"][differ])
        th2 = np.float32(R.REPROJ_FACTOR * np.float64(np.float32(prob["sigma"]) * np.float32(prob["sigma"])))
        ok, good, cosp, _ = R.check_rt_gates(X, pk["raw"], Rm, tm, prob["K"], th2)
        assert ok[acc].all(), (m, np.nonzero(acc & ~ok)[0])
        vg = np.zeros(n1, np.uint8)
        vg[first[acc & good]] = 1
        assert _eq(vg, dev["mot_good"][m]) and dev["mot_n_good"][m] == int(acc.sum())
        untouched = np.ones(n1, bool)
        untouched[first[acc]] = False
        assert not dev["mot_p3d"][m][untouched].any()
        n = int(acc.sum())
        want = np.sort(cosp[acc])[min(R.PARALLAX_RANK, n - 1)] if n else np.float32(1)
        assert _eq(dev["mot_cos"][m], want), (m, dev["mot_cos"][m], want)
        pars.append(R.parallax_of(dev["mot_cos"][m]) if n else np.float32(0))
    if dev["n_motions"] == 0:
        assert not dev["returned"] and dev["motion"] == -1
        return
    rule = R.rule_h if dev["branch"] == R.BRANCH_H else R.rule_f
    ret, best = rule(dev["mot_n_good"][:dev["n_motions"]], pars, dev["n_inliers"], prob["min_parallax"], prob["min_triangulated"])
    assert (dev["returned"], dev["motion"]) == (ret, best), (dev["returned"], dev["motion"], ret, best, dev["mot_n_good"], pars)
    if best >= 0:
        assert dev["n_good"] == dev["mot_n_good"][best] and _eq(dev["cos_parallax"], dev["mot_cos"][best]) and _eq(dev["parallax"], R.parallax_of(dev["mot_cos"][best]))
    if ret:
        assert _eq(dev["R21"], dev["mot_R"][best]) and _eq(dev["t21"], dev["mot_t"][best])
        assert _eq(dev["p3d"], dev["mot_p3d"][best]) and _eq(dev["triangulated"], dev["mot_good"][best])
    else:
        assert not dev["R21"].any() and not dev["t21"].any() and not dev["p3d"].any() and not dev["triangulated"].any()


# ---------------------------------------------------------------------- Group C
@pytest.mark.gpu
@pytest.mark.parametrize("name", FRIENDLY + ["workload"])
def test_yardstick_outcome(name):
    """branch, both winners, returned and the motion hypothesis (as a set, by nearest (R, t)) equal the yardstick's; R21 / t21 within RT_REL, p3d within X3D_REL of the
    point's norm, triangulated equal outside MARGIN_REL of a gate."""
    prob, pk, ref, dev = _case(name)
    assert (dev["branch"], dev["best_h"], dev["best_f"], dev["returned"]) == (ref["branch"], ref["best_h"], ref["best_f"], ref["returned"])
    assert ref["returned"] and dev["n_motions"] == len(ref["motions"])
    d = [_motion_dist(dev["mot_R"][dev["motion"]], dev["mot_t"][dev["motion"]], Rr, tr) for Rr, tr in ref["motions"]]
    assert int(np.argmin(d)) == ref["motion"]
    print(name, "motion distance %.3e (RT_REL %.3e)" % (d[ref["motion"]], RT_REL))
    assert _motion_dist(dev["R21"], dev["t21"], ref["R21"], ref["t21"]) <= RT_REL
    rt = ref["rt"][ref["motion"]]
    near = np.zeros(pk["n1"], bool)
    near[pk["first"][rt["margin"] < MARGIN_REL]] = True
    assert _eq(dev["triangulated"][~near], ref["triangulated"][~near])
    both = (dev["triangulated"] > 0) & (ref["triangulated"] > 0)
    X, Y = dev["p3d"][both].astype(np.float64), ref["p3d"][both].astype(np.float64)
    rel = np.linalg.norm(X - Y, axis=1) / np.linalg.norm(Y, axis=1)
    print(name, "%d points, largest |dX| / |X| %.3e (X3D_REL %.3e)" % (both.sum(), rel.max(), X3D_REL))
    assert both.sum() >= prob["min_triangulated"] and (rel <= X3D_REL).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SC.IRREGULAR))
def test_irregular_outcome(name):
    """Every irregular family ends as the yardstick says."""
    prob, pk, ref, dev = _case(name)
    assert (dev["returned"], dev["no_model"], dev["degenerate"], dev["branch"]) == (ref["returned"], ref["no_model"], ref["degenerate"], ref["branch"]), SC.IRREGULAR[name][1]


@pytest.mark.gpu
def test_singular_homography_on_device():
    """The scene `singular`: hypothesis 0 has an exactly singular H21i -- the zero inverse, NaN chi-squares, a NaN score that never wins -- and a zero third row, so
    every transfer denominator of :368 is exactly zero and its chi-square not finite; a NaN chi-square fails `> th`, so the flags stay set as upstream leaves them
    (Group B replays all of it bit for bit)."""
    prob, pk, ref, dev = _case("singular")
    H, Hi = dev["hyp_H21"][0], dev["hyp_H12"][0]
    assert R.det3(H) == 0 and not Hi.any() and not H[2].any() and H[0].any()
    assert np.isnan(dev["hyp_SH"][0]) and dev["best_h"] > 0 and np.isfinite(dev["SH"]) and dev["SH"] > 0
    flags, score, chi = R.check_homography(H, Hi, pk["raw"], prob["sigma"])
    assert np.isnan(chi[:, 0]).all() and not np.isfinite(chi[:, 1]).any() and _eq(dev["hyp_inlier_H"][0] > 0, flags)
    assert (dev["best_h"], dev["best_f"], dev["branch"], dev["returned"]) == (ref["best_h"], ref["best_f"], ref["branch"], ref["returned"])


# ---------------------------------------------------------------------- the entry point
def _raw_call(prob, sets):
    """the C call with sentinel-filled outputs: (status, result struct, p3d, triangulated)"""
    from eao_fusion_amd import _lib
    k1, k2 = np.ascontiguousarray(prob["keys1"], np.float32), np.ascontiguousarray(prob["keys2"], np.float32)
    m12, sets = np.ascontiguousarray(prob["matches12"], np.int32), np.ascontiguousarray(sets, np.int32)
    P, Rs = _lib.InitializerProblem(), _lib.InitializerResult()
    P.n1, P.n2, P.keys1_xy, P.keys2_xy, P.n_matches, P.matches12 = len(k1), len(k2), _lib.ptr(k1), _lib.ptr(k2), len(m12), _lib.ptr(m12)
    P.fx, P.fy, P.cx, P.cy = [float(v) for v in prob["K"]]
    P.sigma, P.min_parallax, P.min_triangulated = float(prob["sigma"]), float(prob["min_parallax"]), int(prob["min_triangulated"])
    C.memset(C.byref(Rs), 0x5A, C.sizeof(Rs))
    p3d, tri = np.full((len(k1), 3), 7.5, np.float32), np.full(len(k1), 9, np.uint8)
    for f, _t in Rs._fields_:
        if _t is C.c_void_p:
            setattr(Rs, f, None)
    Rs.p3d, Rs.triangulated = _lib.ptr(p3d), _lib.ptr(tri)
    before = bytes(Rs)
    st = _lib.load().eao_initializer_initialize(C.byref(P), _lib.ptr(sets), len(sets), C.byref(Rs))
    return st, bytes(Rs) == before, p3d, tri


@pytest.mark.gpu
def test_invalid_problems_write_nothing():
    from eao_fusion_amd import _lib
    good = SC.irregular("n63")
    st, same, p3d, tri = _raw_call(good, good["sets"])
    assert st == 0 and not same

    def bad(**kw):
        p = dict(good)
        p.update({k: np.array(v) if isinstance(v, np.ndarray) else v for k, v in kw.items()})
        return p
    k_nan, k_inf = good["keys1"].copy(), good["keys2"].copy()
    k_nan[5, 1], k_inf[0, 0] = np.nan, np.inf
    m_hi, m_neg, m_desc = good["matches12"].copy(), good["matches12"].copy(), good["matches12"].copy()
    m_hi[3, 1], m_neg[0, 0] = len(good["keys2"]), -1
    m_desc[[4, 5]] = m_desc[[5, 4]]
    s_hi = good["sets"].copy()
    s_hi[-1, -1] = len(good["matches12"])
    cases = [(bad(matches12=good["matches12"][:7]), good["sets"] % 7), (good, s_hi), (bad(matches12=m_hi), good["sets"]), (bad(matches12=m_neg), good["sets"]),
             (bad(matches12=m_desc), good["sets"]), (bad(keys1=k_nan), good["sets"]), (bad(keys2=k_inf), good["sets"]),
             (bad(K=(500.0, np.inf, 320.0, 240.0)), good["sets"]), (bad(K=(np.nan, 500.0, 320.0, 240.0)), good["sets"])]
    for p, s in cases:
        st, same, p3d, tri = _raw_call(p, s)
        assert st == _lib.EAO_ERR_INVALID and same and (p3d == 7.5).all() and (tri == 9).all()


def _bits(r):
    return b"".join(np.ascontiguousarray(r[k]).tobytes() for k in sorted(r))


@pytest.mark.gpu
def test_two_calls_are_bit_identical():
    from eao_fusion_amd.initializer import initialize
    for name in ("general_96", "planar_96", "duplicated"):
        prob = _problem(name)
        assert _bits(initialize(prob, prob["sets"], inspect=True)) == _bits(initialize(prob, prob["sets"], inspect=True)) == _bits(_case(name)[3])


@pytest.mark.gpu
def test_four_host_threads():
    """Four host threads, each its own scene (its own stream and staging block): the single-call bits."""
    from eao_fusion_amd.initializer import initialize
    names = ["general_96", "planar_96", "n257", "sigma_2"]
    want = [_bits(_case(n)[3]) for n in names]
    got, probs = [None] * 4, [_problem(n) for n in names]

    def work(k):
        for _ in range(3):
            got[k] = _bits(initialize(probs[k], probs[k]["sets"], inspect=True))
    ts = [threading.Thread(target=work, args=(k,)) for k in range(4)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert got == want


@pytest.mark.gpu
def test_normal_path_equals_inspected():
    from eao_fusion_amd.initializer import initialize
    for name in ("general_96", "planar_96", "pure_rotation"):
        prob, pk, ref, dev = _case(name)
        r = initialize(prob, prob["sets"])
        assert all(_eq(r[k], dev[k]) for k in r)


@pytest.mark.gpu
@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "initializer", "*.npz"))))
def test_golden(path):
    """The recorded yardstick results: outcome exact, the motion and the points within the bands."""
    from eao_fusion_amd.initializer import initialize
    z = np.load(path)
    prob = dict(keys1=z["keys1"], keys2=z["keys2"], matches12=z["matches12"], K=tuple(z["K"]), sigma=float(z["sigma"]), min_parallax=float(z["min_parallax"]),
                min_triangulated=int(z["min_triangulated"]))
    r = initialize(prob, z["sets"])
    assert (r["returned"], r["branch"], r["best_h"], r["best_f"], r["degenerate"], r["no_model"]) == (bool(z["returned"]), int(z["branch"]), int(z["best_h"]), int(z["best_f"]),
                                                                                                      bool(z["degenerate"]), bool(z["no_model"]))
    if r["returned"]:
        assert _motion_dist(r["R21"], r["t21"], z["R21"], z["t21"]) <= RT_REL
        both = (r["triangulated"] > 0) & (z["triangulated"] > 0)
        X, Y = r["p3d"][both].astype(np.float64), z["p3d"][both].astype(np.float64)
        assert both.sum() >= int(z["min_triangulated"]) and (np.linalg.norm(X - Y, axis=1) <= X3D_REL * np.linalg.norm(Y, axis=1)).all()


def test_golden_files_exist():
    assert len(glob.glob(os.path.join(ROOT, "tests", "golden", "initializer", "*.npz"))) == 3


@pytest.mark.gpu
def test_class_surface_on_device(tmp_path):
    """include/eaofusion/Initializer.h through InitializerT with stand-in frames and a RandomT fed the recorded sets: what the Python mirror returns for that problem."""
    from eao_fusion_amd import _lib
    from eao_fusion_amd.initializer import initialize
    exe = str(tmp_path / "initializer_driver")
    src = os.path.join(ROOT, "tests", "cpp", "initializer")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-DEAOFUSION_FORCE_CV_COMPAT", "-I", os.path.join(ROOT, "include"), os.path.join(src, "initializer_driver.cpp"),
                           _lib.LIB_PATH, "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    import initializer_frames as FR
    for name in ("general_96", "planar_96", "pure_rotation"):
        prob = _problem(name)
        txt, v12 = FR.frames_text(prob)
        out = subprocess.run([exe], input=txt, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout + out.stderr
        got = FR.parse_result(out.stdout)
        r = initialize(prob, prob["sets"])
        assert got["returned"] == r["returned"]
        if r["returned"]:
            assert _eq(got["R21"], r["R21"]) and _eq(got["t21"], r["t21"]) and _eq(got["p3d"], r["p3d"]) and _eq(got["triangulated"], r["triangulated"] > 0)
