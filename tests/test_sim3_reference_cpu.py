"""CPU checks of the OptimizeSim3 yardstick (tests/sim3_reference.py) and of the class surface's host walk
(include/eaofusion/OptimizerSim3.h, compiled with g++ against the stand-ins in tests/cpp/sim3/)."""
import math
import os
import subprocess

import numpy as np
import pytest

import sim3_reference as R
import sim3_scenes as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sim3_close(a, b, tol):
    return np.abs(a.q - b.q).max() <= tol and np.abs(a.t - b.t).max() <= tol and abs(a.s - b.s) <= tol


def _as_matrix(S):
    M = np.eye(4)
    M[:3, :3] = S.s * R.quat_to_R(S.q)
    M[:3, 3] = S.t
    return M


# ---------------------------------------------------------------------- exp map
# The branch formulas divide rounding noise by sigma^2 or theta^2 (~1e-10 at the boundary): upstream's exp map is continuous across
# its eps boundaries to a few 1e-6, not to the last bit.
EXP_BOUNDARY_TOL = 1e-5

@pytest.mark.parametrize("omega_dir,sigma", [((1, 0, 0), 0.0), ((0.3, -0.5, 0.8), 0.0), ((0.3, -0.5, 0.8), 0.2), ((0, 1, 0), -0.3)])
def test_exp_continuous_across_theta_eps(omega_dir, sigma):
    d = np.asarray(omega_dir, np.float64) / np.linalg.norm(omega_dir)
    ups = np.array([0.1, -0.2, 0.3])
    lo = R.sim3_exp(np.r_[d * (R.EPS * (1 - 1e-6)), ups, sigma])
    hi = R.sim3_exp(np.r_[d * (R.EPS * (1 + 1e-6)), ups, sigma])
    assert _sim3_close(lo, hi, EXP_BOUNDARY_TOL)


@pytest.mark.parametrize("theta", [0.0, 0.4])
def test_exp_continuous_across_sigma_eps(theta):
    w = np.array([theta, 0.0, 0.0])
    ups = np.array([0.5, 0.1, -0.7])
    lo = R.sim3_exp(np.r_[w, ups, R.EPS * (1 - 1e-6)])
    hi = R.sim3_exp(np.r_[w, ups, R.EPS * (1 + 1e-6)])
    assert _sim3_close(lo, hi, EXP_BOUNDARY_TOL)
    lo = R.sim3_exp(np.r_[w, ups, -R.EPS * (1 - 1e-6)])
    hi = R.sim3_exp(np.r_[w, ups, -R.EPS * (1 + 1e-6)])
    assert _sim3_close(lo, hi, EXP_BOUNDARY_TOL)


def test_exp_small_angle_scaled_branch_as_upstream_writes_it():
    """theta < eps <= |sigma|: upstream's B = ((sigma^2 / 2 - sigma + 1) s) / sigma^3 lacks the '- 1' of the series, so with 0 < theta < eps the
    translation jumps by ~ B theta^2 |upsilon| at the sigma boundary.  Restated as written (the device does the same); never reached by
    OptimizeSim3's own updates, whose rotation part is either 0 (Jacobian perturbations of sigma) or far above eps."""
    w, ups = np.array([3e-6, 0.0, 0.0]), np.array([0.5, 0.1, -0.7])
    hi = R.sim3_exp(np.r_[w, ups, R.EPS * (1 + 1e-6)])
    sigma = R.EPS * (1 + 1e-6)
    B = ((0.5 * sigma * sigma - sigma + 1) * math.exp(sigma)) / (sigma * sigma * sigma)
    assert B > 1e14 and np.abs(hi.t).max() > 1e3


def test_exp_of_zero_is_identity():
    S = R.sim3_exp(np.zeros(7))
    assert np.array_equal(S.q, [0, 0, 0, 1]) and np.array_equal(S.t, [0, 0, 0]) and S.s == 1.0


def test_exp_matches_matrix_exponential():
    """The large-angle branch against a series matrix exponential of the 4 x 4 generator (independent formulation)."""
    u = np.array([0.3, -0.2, 0.5, 0.4, -0.1, 0.2, 0.25])
    G = np.zeros((4, 4))
    w, v, sg = u[:3], u[3:6], u[6]
    G[:3, :3] = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) + sg * np.eye(3)
    G[:3, 3] = v
    E, term = np.eye(4), np.eye(4)
    for k in range(1, 40):
        term = term @ G / k
        E = E + term
    assert np.abs(_as_matrix(R.sim3_exp(u)) - E).max() < 1e-12


# ---------------------------------------------------------------------- Sim3 algebra
def test_inverse_round_trip():
    rng = np.random.default_rng(3)
    for _ in range(20):
        S = R.sim3_exp(rng.normal(size=7) * [1, 1, 1, 1, 1, 1, 0.3])
        X = rng.normal(size=(50, 3)) * 4
        assert np.abs(S.inverse().map(S.map(X)) - X).max() < 1e-12
        assert np.abs(_as_matrix(S * S.inverse()) - np.eye(4)).max() < 1e-12


def test_composition_is_matrix_product():
    rng = np.random.default_rng(4)
    A, B = R.sim3_exp(rng.normal(size=7) * 0.4), R.sim3_exp(rng.normal(size=7) * 0.4)
    assert np.abs(_as_matrix(A * B) - _as_matrix(A) @ _as_matrix(B)).max() < 1e-12


def _random_q(rng):
    q = rng.normal(size=4)
    return q / np.linalg.norm(q)


def test_quaternion_from_R_random_rotations():
    rng = np.random.default_rng(5)
    for _ in range(200):
        q = _random_q(rng)
        r = R.quat_from_R(R.quat_to_R(q))
        assert min(np.abs(r - q).max(), np.abs(r + q).max()) < 1e-12


@pytest.mark.parametrize("axis", [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0.3, -0.4, 0.866)])
def test_quaternion_from_R_half_turns(axis):
    """180-degree rotations: trace -1, so the largest-diagonal branches decide."""
    q = SC.axis_angle_q(axis, math.pi)
    r = R.quat_from_R(R.quat_to_R(q))
    assert min(np.abs(r - q).max(), np.abs(r + q).max()) < 1e-12


# ---------------------------------------------------------------------- Jacobians, LM
def test_numeric_jacobian_against_coarse_difference():
    p = SC.scene(n=40, seed=8)
    E = R.Edges(p)
    S = R.Sim3(p["q"], p["t"], p["s"])
    idx = np.arange(40)
    J12, J21 = R.numeric_jacobians(E, S, idx)
    h = 1e-5
    for d in range(6):     # fix_scale: the 7th column is exactly zero
        u = np.zeros(7)
        u[d] = h
        ep12, ep21 = R.errors(E, R.sim3_exp(u) * S, idx)
        u[d] = -h
        em12, em21 = R.errors(E, R.sim3_exp(u) * S, idx)
        for J, ep, em in ((J12, ep12, em12), (J21, ep21, em21)):
            coarse = (ep - em) / (2 * h)
            assert np.abs(J[:, :, d] - coarse).max() <= 1e-4 * max(1.0, np.abs(coarse).max())
    assert not J12[:, :, 6].any() and not J21[:, :, 6].any()


def test_ldlt_pivot_solves_and_rejects_indefinite():
    rng = np.random.default_rng(9)
    A = rng.normal(size=(7, 7))
    A = A @ A.T + 0.1 * np.eye(7)
    b = rng.normal(size=7)
    ok, x = R.ldlt_pivot_solve(A, b)
    assert ok and np.abs(A @ x - b).max() < 1e-10
    A[3, 3] = -5.0
    ok, _ = R.ldlt_pivot_solve(A, b)
    assert not ok


@pytest.mark.parametrize("fix_scale", [True, False])
def test_recovers_planted_sim3(fix_scale):
    p = SC.scene(n=300, seed=10 + fix_scale, fix_scale=fix_scale, off_deg=5.0, off_m=0.1)
    o = R.optimize_sim3(p)
    pl = p["planted"]
    start = max(np.abs(np.abs(p["q"]) - np.abs(pl["q"])).max(), np.abs(p["t"] - pl["t"]).max())
    err = max(np.abs(np.abs(o["q"]) - np.abs(pl["q"])).max(), np.abs(o["t"] - pl["t"]).max())
    assert not o["early_exit"] and err < 0.1 * start
    if fix_scale:
        assert o["s"] == float(p["s"])      # bit-identical: exp(0) * s
    else:
        assert abs(o["s"] - pl["s"]) < 0.1 * abs(p["s"] - pl["s"]) + 5e-3


def test_early_exit_leaves_S_and_nulls_pass_one_outliers():
    p = SC.scene(n=14, seed=51, fix_scale=True, outlier_frac=0.6)
    o = R.optimize_sim3(p)
    assert o["early_exit"] and o["n_inliers"] == 0 and o["iters"][1] == 0
    assert np.array_equal(o["q"], p["q"]) and np.array_equal(o["t"], p["t"]) and o["s"] == p["s"]
    # exactly the correspondences the first inlier pass rejects, on the stale chi2 of the last trial of optimize(5)
    E = R.Edges(p)
    S, it0, stale = R.lm_optimize(E, R.Sim3(p["q"], p["t"], p["s"]), np.arange(14), 5, [])
    assert np.array_equal(o["removed"].astype(bool), stale) and 14 - int(stale.sum()) < 10


def test_no_correspondences():
    o = R.optimize_sim3(SC.scene(n=0, seed=1))
    assert o["early_exit"] and list(o["iters"]) == [0, 0] and o["n_inliers"] == 0


def test_reference_is_fast_enough_for_the_suite():
    import time
    p = SC.scene(n=2000, seed=12)
    t0 = time.perf_counter()
    R.optimize_sim3(p)
    assert time.perf_counter() - t0 < 1.0


# ---------------------------------------------------------------------- the parity families
def test_families_cover_the_cases():
    """The GPU parity families reach what they are named for: the early exit (with and without correspondences), a first pass that
    rejects correspondences so that the second optimize() gets 10 iterations, clean problems that get 5, both scale modes."""
    outs = [(name, kw, R.optimize_sim3(SC.scene(**kw))) for name, kw in SC.FAMILIES]
    for name, kw, o in outs:
        if name in ("early_exit", "empty"):
            assert o["early_exit"] and o["budget"] == (5, 0), (name, kw)
        else:
            assert not o["early_exit"], (name, kw)
        if name == "outliers":
            assert o["budget"] == (5, 10) and o["removed"].sum() > 0, (name, kw)
    assert any(o["budget"] == (5, 5) for _, _, o in outs)
    assert {kw["fix_scale"] for name, kw, o in outs if not o["early_exit"]} == {True, False}


def _update_norm(p, a):
    return max(np.abs(a["q"] - p["q"]).max(), np.abs(a["t"] - p["t"]).max(), abs(a["s"] - p["s"]))


def _displacement(a, b):
    return max(np.abs(a["q"] - b["q"]).max(), np.abs(a["t"] - b["t"]).max(), abs(a["s"] - b["s"]))


@pytest.fixture(scope="module")
def irregular():
    """Every IRREGULAR family through the yardstick, as generated and under ulp_perturbed seeds 0..3 (what tools/sim3_chaotic_seeds.py
    --irregular logs): {id: (name, kw, problem, result, [results of the four one-ulp copies])}."""
    out = {}
    for (name, kw, edit), fid in zip(SC.IRREGULAR, SC.irregular_ids()):
        p = SC.irregular_scene(kw, edit)
        out[fid] = (name, kw, p, R.optimize_sim3(p), [R.optimize_sim3(SC.ulp_perturbed(p, s)) for s in range(4)])
    assert len(out) == len(SC.IRREGULAR), "IRREGULAR ids are not unique"
    return out


def _only(irregular, name):
    hits = [v for v in irregular.values() if v[0] == name]
    assert len(hits) == 1, name
    return hits[0][2], hits[0][3]


def test_iteration_unstable_table_matches_the_one_ulp_probe(irregular):
    """sim3_scenes.ITERS_UNSTABLE lists exactly the families whose reference iteration counts move under a one-ulp change of the
    observations, and on those only the counts move (the GPU test still compares everything else).  Likewise IRREGULAR_ITERS_UNSTABLE and
    IRREGULAR_BANDED over IRREGULAR and ulp_perturbed seeds 0..3 (profiles/sim3_irregular_bands.txt), within their caps."""
    found = set()
    for name, kw in SC.FAMILIES:
        p = SC.scene(**kw)
        a, b = R.optimize_sim3(p), R.optimize_sim3(SC.ulp_perturbed(p))
        assert np.array_equal(a["removed"], b["removed"]) and a["n_inliers"] == b["n_inliers"] and a["early_exit"] == b["early_exit"], (name, kw)
        if list(a["iters"]) != list(b["iters"]):
            found.add(SC.family_key(name, kw))
            upd = max(np.abs(a["q"] - p["q"]).max(), np.abs(a["t"] - p["t"]).max(), abs(a["s"] - p["s"]))
            disp = max(np.abs(a["q"] - b["q"]).max(), np.abs(a["t"] - b["t"]).max(), abs(a["s"] - b["s"]))
            assert disp <= 2e-5 * upd, (name, kw, disp / upd)
    assert found == SC.ITERS_UNSTABLE
    from lm_tolerances import UPDATE_REL
    unstable, banded = set(), set()
    for fid, (name, kw, p, a, bs) in irregular.items():
        if any(list(a["iters"]) != list(b["iters"]) for b in bs):
            unstable.add(SC.family_key(name, kw))
        upd = _update_norm(p, a)
        if upd and max(_displacement(a, b) for b in bs) > UPDATE_REL * upd:
            banded.add(SC.family_key(name, kw))
    assert unstable == SC.IRREGULAR_ITERS_UNSTABLE and banded == SC.IRREGULAR_BANDED
    assert len(banded) <= SC.IRREGULAR_BANDED_MAX == 1
    early = {SC.family_key(name, kw) for name, kw, p, a, bs in irregular.values() if a["early_exit"]}
    assert len(unstable - early) <= SC.IRREGULAR_ITERS_UNSTABLE_MAX == 3
    assert all(_displacement(a, b) <= UPDATE_REL / 2 * _update_norm(p, a) for name, kw, p, a, bs in irregular.values() for b in bs
               if name in ("scale_small", "scale_large"))      # the extreme-scale pair that is held to UPDATE_REL


def test_irregular_schedules_hold_under_one_ulp(irregular):
    """No IRREGULAR family's removed / n_inliers / early_exit moves when every observation moves by one ulp (seeds 0..3)."""
    for fid, (name, kw, p, a, bs) in irregular.items():
        for b in bs:
            assert np.array_equal(a["removed"], b["removed"]) and a["n_inliers"] == b["n_inliers"] and a["early_exit"] == b["early_exit"], fid


@pytest.mark.parametrize("which", [1, 2])
def test_irregular_behind_camera_rows_are_behind_and_removed(irregular, which):
    """The mirrored map points have z < 0 in their own camera frame as the library forms it, the edge that maps them divides by a negative
    z at the start, and every one of them ends in removed."""
    p, o = _only(irregular, "behind_cam%d" % which)
    rows = p["planted_rows"]["behind%d" % which]
    assert len(rows) >= 10
    Xc = R.camera_points(p["T%dw" % which], p["Xw%d" % which])
    assert (Xc[rows, 2] < 0).all() and (np.delete(Xc[:, 2], rows) > 0).all()
    S0 = R.Sim3(p["q"], p["t"], p["s"])
    mapped = S0.map(Xc) if which == 2 else S0.inverse().map(Xc)      # camera-2 points go through S12 (the direct edge), camera-1 points through S21
    assert (mapped[rows, 2] < 0).all()
    assert not o["early_exit"] and o["removed"][rows].all()
    assert {kw["fix_scale"] for name, kw, *_ in irregular.values() if name.startswith("behind_cam")} == {True, False}


def test_irregular_ten_and_nine_survivors(irregular):
    """The nCorr - nBad < 10 gate from both sides: exactly 10 survivors go on, exactly 9 return early; with and without removals."""
    for name, survivors, early in (("ten_survive", 10, False), ("nine_survive", 9, True), ("ten_clean", 10, False), ("nine_clean", 9, True)):
        p, o = _only(irregular, name)
        n = len(p["Xw1"])
        assert n - int(o["removed"].sum()) == survivors and bool(o["early_exit"]) == early, name
        planted = p.get("planted_rows", {}).get("gross", np.zeros(0, np.int64))
        assert np.array_equal(np.nonzero(o["removed"])[0], planted), name
        assert o["n_inliers"] == (0 if early else 10) and o["budget"] == ((5, 0) if early else (5, 10) if len(planted) else (5, 5)), name


def test_irregular_strided_removes_exactly_the_planted_rows(irregular):
    p, o = _only(irregular, "strided")
    rows = p["planted_rows"]["gross"]
    m = np.arange(len(p["Xw1"]))
    assert np.array_equal(rows, m[(m % 256 == 7) | ((m >= 64) & (m < 128))]) and len(rows) == 70     # one thread's stride and one whole wave
    assert np.array_equal(np.nonzero(o["removed"])[0], rows) and not o["early_exit"]


def test_irregular_zero_information_rows_are_never_removed(irregular):
    p, o = _only(irregular, "zero_info")
    rows = p["planted_rows"]["zero_info"]
    assert len(rows) >= 10 and not p["inv_sigma2_1"][rows].any() and not p["inv_sigma2_2"][rows].any()
    assert (p["inv_sigma2_1"] == 0).sum() >= 40 and (p["inv_sigma2_2"] == 0).sum() >= 40
    assert not o["removed"][rows].any() and o["removed"].sum() > 0
    # ... although some of them are gross: with the smallest information any pyramid level carries, the gate would have removed them
    E = R.Edges(p)
    hit = np.intersect1d(rows, p["planted_rows"]["gross"])
    e12, _ = R.errors(E, R.Sim3(o["q"], o["t"], o["s"]), hit)
    assert len(hit) >= 3 and (R.chi2(e12, np.full(len(hit), 1.0 / 1.2 ** 14)) > E.th2).all()


def test_irregular_families_are_what_they_are_named_for(irregular):
    by_name = {}
    for name, kw, p, o, bs in irregular.values():
        by_name.setdefault(name, []).append((kw, p, o))
    # near-zero depth: the collapse returns early, the milder one does not; both really moved the points
    for name, z, early in (("depth_collapse", 1e-4, True), ("depth_near", 0.1, False)):
        (kw, p, o), = by_name[name]
        rows = p["planted_rows"]["depth1"]
        assert np.abs(R.camera_points(p["T1w"], p["Xw1"])[rows, 2] - z).max() < 1e-5 and len(rows) == 4 and bool(o["early_exit"]) == early, name
    # the second optimize() of a pass that removed nothing gets 5 iterations, uses all of them, and would go on with 10
    (kw, p, o), = by_name["budget_five"]
    assert o["budget"] == (5, 5) and list(o["iters"]) == [5, 5] and not o["removed"].any()
    E, idx = R.Edges(p), np.arange(len(p["Xw1"]))
    S, _, _ = R.lm_optimize(E, R.Sim3(p["q"], p["t"], p["s"]), idx, 5, [])
    assert R.lm_optimize(E, S, idx, 10, [])[1] > 5
    # extreme scales, planted and kept
    for name, s in (("scale_small", 0.05), ("scale_large", 20.0), ("scale_large_banded", 20.0)):
        (kw, p, o), = by_name[name]
        assert p["planted"]["s"] == s and not p["fix_scale"] and abs(o["s"] / s - 1) < 0.02, name
    for name in ("all_outliers", "far_start_lost"):
        for kw, p, o in by_name[name]:
            assert o["early_exit"] and o["removed"].sum() >= len(p["Xw1"]) - 9, name
    assert {kw["fix_scale"] for kw, p, o in by_name["far_start_lost"]} == {True, False}
    # a far start that survives, through rejected trials
    (kw, p, o), = by_name["far_start"]
    assert not o["early_exit"] and max(t[2] for t in o["trace"]) >= 3
    # Huber widths whose float square root does not square back to th2
    for name, th2 in (("th2_narrow", 2.0), ("th2_wide", 40.0)):
        (kw, p, o), = by_name[name]
        E = R.Edges(p)
        assert E.th2 == th2 and E.delta * E.delta != th2 and not o["early_exit"], name
    (kw, p, o), = by_name["non_unit_q"]
    assert abs(np.linalg.norm(p["q"]) - 1.003) < 1e-12 and not o["early_exit"]
    (kw, p, o), = by_name["duplicates"]
    rows = p["planted_rows"]["duplicates"]
    assert len(rows) == 50 and all((p[k][rows] == p[k][7]).all() for k in ("Xw1", "Xw2", "obs1", "obs2", "inv_sigma2_1", "inv_sigma2_2"))
    assert len(set(o["removed"][rows])) == 1
    # wave and workgroup edges, and far above one stride
    assert [kw["n"] for kw, p, o in by_name["edge_n"]] == [63, 64, 65, 255, 256, 257, 513, 1025]
    assert all(not o["early_exit"] and o["removed"].any() for kw, p, o in by_name["edge_n"])
    (kw, p, o), = by_name["large"]
    assert len(p["Xw1"]) == 20000 and not o["early_exit"]


# ---------------------------------------------------------------------- the class surface's walk
@pytest.fixture(scope="module")
def walk_driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sim3walk") / "sim3_walk")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-DEAOFUSION_FORCE_CV_COMPAT", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "sim3", "sim3_driver.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("n,seed", [(25, 1), (60, 2), (0, 3)])
def test_adapter_walk(walk_driver, n, seed):
    p = SC.scene(n=n, seed=100 + seed, fix_scale=bool(seed % 2))
    txt, expected = SC.keyframe_scene(p, seed=seed)
    out = subprocess.run([walk_driver, "walk"], input=txt, capture_output=True, text=True, check=True).stdout.strip().split("\n")
    rows = {}
    corr = []
    for line in out:
        k, *v = line.split()
        if k == "c":
            corr.append([float(x) for x in v])
        else:
            rows[k] = v
    assert int(rows["n"][0]) == n
    assert [int(v) for v in rows["index"]] == expected      # skipped entries (no match, no point, bad, i2 < 0) and index order
    assert np.array_equal(np.array(rows["T1w"], np.float32), np.asarray(p["T1w"], np.float32).ravel())
    assert np.array_equal(np.array(rows["T2w"], np.float32), np.asarray(p["T2w"], np.float32).ravel())
    assert np.array_equal(np.array(rows["K"], np.float32), np.r_[p["K1"], p["K2"]].astype(np.float32))
    S = [float(v) for v in rows["S"]]
    assert S[:4] == list(map(float, p["q"])) and S[4:7] == list(map(float, p["t"])) and S[7] == float(p["s"])   # x, y, z, w read back as set
    assert np.float32(S[8]) == np.float32(p["th2"]) and int(S[9]) == int(p["fix_scale"])
    if n:
        c = np.array(corr, np.float32)
        assert np.array_equal(c[:, 0:3], p["Xw1"]) and np.array_equal(c[:, 3:6], p["Xw2"])
        assert np.array_equal(c[:, 6:8], p["obs1"]) and np.array_equal(c[:, 8:10], p["obs2"])
        assert np.array_equal(c[:, 10], p["inv_sigma2_1"]) and np.array_equal(c[:, 11], p["inv_sigma2_2"])
        # the camera-frame points the library forms from what the walk hands over: float products, one rounding, + t in float
        Xc = R.camera_points(np.array(rows["T1w"], np.float32), c[:, 0:3])
        manual = np.array([[np.float32(np.float32(sum(np.float64(p["T1w"][i][j]) * np.float64(c[k, j]) for j in range(3))) + p["T1w"][i][3])
                            for i in range(3)] for k in range(min(n, 10))], np.float64)
        assert np.array_equal(Xc[:len(manual)], manual)
    # the write-back: Sim3T(QuatT(w, x, y, z), ...) reads back as (x, y, z, w)
    assert [float(v) for v in rows["written"]] == [0.1, -0.2, 0.3, 0.9, 1.5, -2.5, 3.5, 1.25]
