"""Holds the OptimizeEssentialGraph yardstick (tests/essential_graph_reference.py) and its scenes (tests/essential_graph_scenes.py) to what they claim -- the GPU
parity tests (tests/test_gpu_essential_graph.py) are only as good as these two -- and the tables written from profiles/essential_graph_bands.txt to that file.
CPU only."""
import importlib.util
import os
import re

import numpy as np
import pytest

import essential_graph_reference as R
import essential_graph_scenes as SC
import essential_graph_tolerances as TOL
from lm_tolerances import UPDATE_REL
from sim3_reference import sim3_exp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _log_exp(u):
    S = sim3_exp(np.asarray(u, np.float64))
    V = R.VSim3(S.q[:, None], S.t[None, :], np.array([S.s]))
    return R.sim3_log(V)[0], int(R.log_branches(V)[0])


# (omega direction scaled to theta, upsilon, sigma) -> the branch of log: 2 * (|sigma| >= eps) + (d <= 1 - eps)
AXIS = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
UPS = np.array([0.4, -0.2, 0.7])


def _u(theta, sigma):
    return np.concatenate([AXIS * theta, UPS, [sigma]])


@pytest.mark.parametrize("theta,sigma,branch", [(3e-6, 2e-6, 0), (0.0, 0.0, 0), (0.3, 2e-6, 1), (2.5, 0.0, 1), (3e-6, 0.05, 2), (3e-6, -0.3, 2), (0.3, 0.05, 3), (1.2, -0.4, 3)])
def test_log_inverts_exp_in_each_branch(theta, sigma, branch):
    u = _u(theta, sigma)
    got, br = _log_exp(u)
    assert br == branch
    assert np.abs(got - u).max() <= 1e-9


@pytest.mark.parametrize("theta", [0.3, 3e-6])
def test_log_across_the_sigma_boundary(theta):
    """|sigma| just below and just above 1e-5: both branches are taken and both invert exp (exp switches its own formulas at the same sigma)."""
    lo, hi = _log_exp(_u(theta, 0.99e-5)), _log_exp(_u(theta, 1.01e-5))
    assert lo[1] // 2 == 0 and hi[1] // 2 == 1
    assert np.abs(lo[0] - _u(theta, 0.99e-5)).max() <= 1e-9 and np.abs(hi[0] - _u(theta, 1.01e-5)).max() <= 1e-9


def test_log_across_the_angle_boundary():
    """d = cos(theta) crosses 1 - 1e-5 at theta = 4.4721e-3.  Below it log takes omega = deltaR / 2 (sin(theta) / theta short of theta: theta^3 / 6 = 1.5e-8) and
    A = 1 / 2, B = 1 / 6 where exp, whose own switch is at theta = 1e-5, used the full formulas (theta^2 / 24 = 8e-7 of upsilon)."""
    t_lo, t_hi = 4.46e-3, 4.48e-3
    lo, hi = _log_exp(_u(t_lo, 0.0)), _log_exp(_u(t_hi, 0.0))
    assert lo[1] == 0 and hi[1] == 1
    assert np.abs(hi[0] - _u(t_hi, 0.0)).max() <= 1e-9
    assert np.abs(lo[0][:3] - _u(t_lo, 0.0)[:3]).max() <= 2e-8 and np.abs(lo[0][3:] - _u(t_lo, 0.0)[3:]).max() <= 2e-6


def test_log_small_angle_branch_with_scale_is_upstreams():
    """1e-5 <= theta < 4.47e-3 with |sigma| >= 1e-5: log takes upstream's small-angle B = ((sigma^2 / 2 - sigma + 1) s) / sigma^3 (types/sim3.h:199, no "- 1" in the
    numerator: about 1 / sigma^3) where exp took the general formula, so upsilon does NOT come back -- omega and sigma do.  The restatement keeps that: it is what
    the reference computes on a nearly converged monocular graph."""
    u = _u(2e-3, 0.05)
    got, br = _log_exp(u)
    assert br == 2
    assert np.abs(got[:3] - u[:3]).max() <= 1e-8 and abs(got[6] - u[6]) <= 1e-12
    assert np.abs(got[3:6] - u[3:6]).max() > 1e-3


def test_lu3_solve_pivots():
    rng = np.random.default_rng(5)
    W = rng.normal(size=(50, 3, 3))
    W[:10, 0, 0] = 1e-14       # forces a row exchange in the first column
    W[10:20, 1, 1] = W[10:20, 1, 0] * W[10:20, 0, 1] / W[10:20, 0, 0]      # a zero second pivot without the exchange
    b = rng.normal(size=(50, 3))
    x = R.lu3_solve(W, b)
    assert np.abs(np.einsum("mij,mj->mi", W, x) - b).max() <= 1e-9


def test_numeric_jacobian_against_a_wider_step():
    prob = SC.case("ring9", False)
    G = R.Graph(prob)
    Ji, Jj = R.numeric_jacobians(G, G.S0)
    wide = 1e-6
    P = []
    for d in range(7):
        for sgn in (1.0, -1.0):
            u = np.zeros(7)
            u[d] = sgn * wide
            P.append(sim3_exp(u))
    Wi, Wj = R.numeric_jacobians(G, G.S0, delta_pert=(P, wide))
    # delta = 1e-9 carries ~1e-16 * |t| / 1e-9 of rounding noise per entry; the wide step's truncation error is delta^2
    assert np.abs(Ji - Wi).max() <= 5e-6 and np.abs(Jj - Wj).max() <= 5e-6
    assert np.abs(Ji).max() > 0.5 and np.abs(Jj).max() > 0.5
    fixed_i, fixed_j = G.ei == G.fixed, G.ej == G.fixed
    assert fixed_j.any() and not np.any(Ji[fixed_i]) and not np.any(Jj[fixed_j])      # a fixed vertex's Jacobian is not formed
    Gs = R.Graph(SC.case("ring9", True))
    Jis, Jjs = R.numeric_jacobians(Gs, Gs.S0)
    assert not np.any(Jis[:, :, 6]) and not np.any(Jjs[:, :, 6])      # _fix_scale: the 7th column is exactly zero


@pytest.mark.parametrize("fs", [False, True])
def test_planted_graph_comes_back(fs):
    prob = SC.planted(n=12, seed=3)
    prob["fix_scale"] = fs
    out = R.optimize_essential_graph(prob)
    assert out["chi2_initial"] <= 1e-24 and out["chi2"][-1] <= 1e-24
    assert np.abs(out["Scw"] - prob["Scw"]).max() <= 1e-10
    assert np.array_equal(out["Xw_corrected"][prob["ref"] < 0], prob["Xw"][prob["ref"] < 0])
    assert np.abs(out["Xw_corrected"] - prob["Xw"]).max() <= 1e-5


def _initial_branches(prob):
    G = R.Graph(prob)
    return R.log_branches((G.C * G.S0.take(G.ei)) * G.S0.take(G.ej).inverse()), G


def _final_branches(prob):
    G = R.Graph(prob)
    S = R.VSim3.from_rows(R.optimize_essential_graph(prob)["Scw"])
    return R.log_branches((G.C * S.take(G.ei)) * S.take(G.ej).inverse())


@pytest.mark.parametrize("fs", [False, True])
def test_families_exercise_what_they_say(fs):
    case = lambda name: SC.case(name, fs)
    # the smallest system, two edges between the same pair, one of each kind
    p = case("dup2")
    assert p["n"] == 2 and sorted(map(tuple, p["edges"])) == [(1, 0, 0), (1, 0, 1)] and len(R.Graph(p).free) == 1
    # rows at the 64-row tile edge: 56, 63, and exactly seven tiles / one block past them
    assert [7 * len(R.Graph(case(n)).free) for n in ("ring9", "ring10", "ring65", "ring66")] == [56, 63, 448, 455]
    ring40 = case("ring40")
    assert ring40["n"] == 40 and len(ring40["edges"]) > 40 and ring40["fixed"] == 0
    assert np.all(ring40["edges"][ring40["edges"][:, 1] == 0][:, 0] != 0) and not np.any(ring40["edges"][:, 0] == 0)      # the fixed vertex is vertex 1 of its edges ...
    rev = case("reversed")
    assert np.any(rev["edges"][:, 0] == 0) and not np.any(rev["edges"][:, 1] == 0)                                        # ... and vertex 0 of them here
    Cf, Cr = R.measurements(ring40), R.measurements(rev)
    assert np.abs((Cf * Cr).rows() - np.array([0, 0, 0, 1, 0, 0, 0, 1.0])).max() <= 1e-12                                 # C and C^-1
    assert case("fixed_middle")["fixed"] == 20 and case("fixed_last")["fixed"] == 39
    h = case("hub")
    deg = np.bincount(np.concatenate([h["edges"][:, 0], h["edges"][:, 1]]), minlength=40)
    assert deg[11] >= 35 + 2 and np.sort(deg)[-2] <= deg[11] // 3
    assert [len(case("edges%d" % m)["edges"]) for m in (63, 64, 65, 257)] == [63, 64, 65, 257]
    iso = case("isolated")
    Gi = R.Graph(iso)
    assert not Gi.active[17] and Gi.block[17] < 0 and Gi.active.sum() == 39 and iso["ref"][2] == 17
    out = R.optimize_essential_graph(iso)
    assert np.array_equal(out["Scw"][17], iso["Scw"][17]) and out["n_active"] == 39 and np.array_equal(out["Xw_corrected"][2], iso["Xw"][2])
    # the branches of log
    small = case("drift_small")
    assert np.all(_initial_branches(small)[0] % 2 == 0) and np.all(_final_branches(small) % 2 == 0)      # every edge error in the d > 1 - eps branch, before and after
    large, _ = _initial_branches(case("drift_large"))
    assert np.any(large % 2 == 1) and np.any(large % 2 == 0)                                              # the loop-side edges leave it, the others do not
    unit = case("unit_scale")
    assert np.all(unit["Scw"][:, 7] == 1.0) and np.all(unit["Snc"][:, 7] == 1.0) and np.all(_initial_branches(unit)[0] // 2 == 0)
    drift = case("scale_drift")
    s_c = drift["Scw"][39, 7]
    assert abs(s_c - 0.996 ** 39) < 1e-3 and np.any(_initial_branches(drift)[0] // 2 == 1)
    if not fs:
        assert np.any(_final_branches(drift) // 2 == 1) and np.any(_final_branches(ring40) == 2)         # a freed scale leaves sigma >= eps on nearly converged edges
    big = case("ring300")
    assert big["n"] == 300 and len(R.Graph(big).free) == 299
    # points: no reference, the fixed keyframe
    assert ring40["ref"][0] == -1 and ring40["ref"][1] == ring40["fixed"] and np.sum(ring40["ref"] < 0) >= 3
    for n_points in SC.POINT_COUNTS:
        q = SC.with_points(ring40, n_points)
        assert q["Xw"].shape == (n_points, 3) and q["ref"].shape == (n_points,)


def test_ulp_perturbed_moves_every_entry_by_one_ulp():
    p = SC.case("ring10", False)
    q = SC.ulp_perturbed(p, 1)
    for k in ("Scw", "Snc"):
        assert np.all(q[k] != p[k]) and np.all(np.abs(q[k] - p[k]) <= np.spacing(np.abs(p[k])))
    assert np.array_equal(q["edges"], p["edges"])


def test_elimination_order_is_rounding_only():
    p = SC.case("ring10", False)
    a, b = R.optimize_essential_graph(p), R.optimize_essential_graph(p, perm=SC.permutation(p, 0))
    upd = np.abs(a["Scw"] - p["Scw"]).max()
    assert 0 < np.abs(a["Scw"] - b["Scw"]).max() <= UPDATE_REL * upd


def test_tables_are_the_bands_file():
    """ITERS_UNSTABLE, BANDED and CHI2_LAST_SPREAD are written from profiles/essential_graph_bands.txt (tools/essential_graph_bands.py) and list exactly what it measured;
    two small cases are measured again here."""
    bands = _tool("essential_graph_bands")
    rows = bands.parse(os.path.join(ROOT, "profiles", "essential_graph_bands.txt"))
    assert list(rows) == SC.case_ids()
    assert SC.ITERS_UNSTABLE == {k for k, r in rows.items() if r[1]}
    assert SC.BANDED == {k for k, r in rows.items() if r[0] > UPDATE_REL} and len(SC.BANDED) <= SC.BANDED_MAX
    assert TOL.CHI2_LAST_SPREAD == {k: r[2] for k, r in rows.items()}
    for name, fs in (("ring9", False), ("ring10", False)):
        band, moved, spread, _ = bands.probe(name, fs)
        assert band <= UPDATE_REL and not moved and spread <= TOL.chi2_last_rel("%s-fs%d" % (name, int(fs)))


def test_golden_files_are_the_yardsticks():
    gen = _tool("gen_golden_essential_graph")
    for name, fs in gen.GOLDEN_CASES:
        fn = os.path.join(ROOT, "tests", "golden", "essential_graph", "%s_fs%d.npz" % (name, int(fs)))
        assert os.path.getsize(fn) < (1 << 20)
        z = np.load(fn)
        prob = SC.case(name, fs)
        out = R.optimize_essential_graph(prob)
        assert np.array_equal(z["Scw_in"], prob["Scw"]) and np.array_equal(z["edges"], prob["edges"])
        upd = np.abs(out["Scw"] - prob["Scw"]).max()
        assert np.abs(z["Scw"] - out["Scw"]).max() <= UPDATE_REL * upd and int(z["n_active"]) == out["n_active"]
        if "%s-fs%d" % (name, int(fs)) not in SC.ITERS_UNSTABLE:
            assert int(z["lm_iterations"]) == out["lm_iterations"] and list(z["trials"]) == list(out["trials"])


def test_gpu_test_file_carries_no_literal_tolerance():
    src = open(os.path.join(ROOT, "tests", "test_gpu_essential_graph.py")).read()
    src = re.sub(r'""".*?"""', "", src, flags=re.S)
    assert not re.search(r"\b\d+(\.\d+)?e-\d+\b", src), "a literal tolerance in the GPU test: it belongs in essential_graph_tolerances.py"


def test_abi_declares_the_entry_point():
    hdr = open(os.path.join(ROOT, "include", "eao_fusion.h")).read()
    assert re.search(r"eao_status\s+eao_optimize_essential_graph\s*\(\s*const eao_essential_graph_problem\s*\*\s*\w+\s*,\s*eao_essential_graph_result\s*\*\s*\w+\s*\)", hdr)
    assert "#define EAO_ABI_VERSION 6" in hdr
    from eao_fusion_amd import _lib
    assert "eao_optimize_essential_graph" in _lib.SYMBOLS
    import ctypes as C
    assert C.sizeof(_lib.EssentialGraphProblem) == 80 and C.sizeof(_lib.EssentialGraphResult) == 24 + 4 + 80 + 4 + 160 + 160 + 8 + 8


# ---------------------------------------------------------------------- the class surface's walk against stand-ins (no GPU, no library)
@pytest.fixture(scope="module")
def walk_driver(tmp_path_factory):
    import subprocess
    exe = str(tmp_path_factory.mktemp("essential_graph") / "essential_graph_driver")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-DEAOFUSION_FORCE_CV_COMPAT", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "essential_graph", "essential_graph_driver.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("fs", [False, True])
def test_walk_flattens_a_hand_built_map(walk_driver, fs):
    import subprocess
    from sim3_reference import quat_from_R
    m, text, want = SC.hand_built_map(fs)
    out = subprocess.run([walk_driver, "walk"], input=text, capture_output=True, text=True, check=True).stdout
    p = SC.problem_of_walk(out)
    assert p["ids"] == want["ids"] and p["fixed"] == want["fixed"] and p["fix_scale"] == fs
    assert [tuple(e) for e in p["edges"]] == want["edges"]      # vertex, edge and kind lists: one entry per filter (hand_built_map says which)
    assert list(p["has_nc"]) == want["has_nc"]
    assert list(p["ref"]) == want["refs"] and p["n_map_points"] == want["n_points"] and p["n_planes"] == want["n_planes"]
    good = [k for k in m["kfs"] if not k["bad"]]
    corrected, non_corrected = dict(m["corrected"]), dict(m["non_corrected"])
    pool_of = [i for i, k in enumerate(m["kfs"]) if not k["bad"]]
    for v, kf in enumerate(good):
        T = np.asarray(kf["T"], np.float32)
        pose = np.concatenate([quat_from_R(T[:3, :3].astype(np.float64)), T[:3, 3].astype(np.float64), [1.0]])      # g2o::Sim3(Rcw, tcw, 1.0)
        want_scw = corrected.get(pool_of[v], pose)
        assert np.array_equal(p["Scw"][v], want_scw), v
        assert np.array_equal(p["Snc"][v], non_corrected.get(pool_of[v], want_scw)), v
    xs = [x for x, bad, _, _, _ in m["points"] if not bad] + [x[:3] for x, bad, _, _, _ in m["planes"] if not bad]
    assert np.array_equal(p["Xw"], np.array(xs, np.float32))
    # the flattened graph is one the yardstick can run: every vertex but none is active, the fixed one is the loop keyframe
    G = R.Graph(p)
    assert G.active.all() and len(G.free) == 6


# ---------------------------------------------------------------------- the library's host side (no device): elimination plan, capacity
@pytest.fixture(scope="module")
def built():
    import subprocess
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "eao_fusion_amd", "csrc")])
    from eao_fusion_amd import optimizer
    return optimizer


def _assert_blocks_live(prob, plan):
    """Every tile that k_eg_scatter writes exists: the four corners of each free vertex's own 7 x 7 block and of each pair with an edge, and the right-hand side row."""
    row, tm = plan["row_of"], plan["tile_map"]
    live = lambda r, c: tm[max(r, c) >> 6, min(r, c) >> 6] >= 0
    free = np.nonzero(row >= 0)[0]
    assert len(free) == len(R.Graph(prob).free) and len(set(row[free])) == len(free) and row[free].max() + 7 <= plan["rows"]
    for v in free:
        assert live(row[v], row[v]) and live(row[v] + 6, row[v]) and live(row[v] + 6, row[v] + 6), v
        assert tm[plan["rows"] >> 6, row[v] >> 6] >= 0 and tm[plan["rows"] >> 6, (row[v] + 6) >> 6] >= 0
    for i, j, _ in np.asarray(prob["edges"]).reshape(-1, 3):
        if row[i] >= 0 and row[j] >= 0:
            assert all(live(row[i] + a, row[j] + b) for a in (0, 6) for b in (0, 6)), (i, j)
    return free, row


@pytest.mark.parametrize("name,fs", [c for c in SC.CASES if not c[1]], ids=[i for i, c in zip(SC.case_ids(), SC.CASES) if not c[1]])
def test_plan_keeps_every_block_live(built, name, fs):
    prob = SC.case(name, fs)
    plan = built.essential_graph_plan(prob)
    free, row = _assert_blocks_live(prob, plan)
    straddling = [v for v in free if (row[v] >> 6) != ((row[v] + 6) >> 6)]
    if name == "star":          # no pair of free vertices has an edge: only the vertex's own block keeps the tile below the diagonal alive
        assert len(free) == 11 and plan["rows"] == 128 and [row[v] for v in straddling] == [63] and plan["tile_map"][1, 0] >= 0
        assert not any(row[i] >= 0 and row[j] >= 0 for i, j, _ in prob["edges"])
    if name == "straddle_far":  # the straddling vertex's neighbours lie two and three tiles further down
        e = prob["edges"]
        nb = sorted(set(e[e[:, 1] == 10][:, 0]) | set(e[e[:, 0] == 10][:, 1]))
        assert row[10] == 63 and nb == [25, 30] and all((row[w] >> 6) >= 2 for w in nb)
    if name == "ring300":
        assert plan["segments"] > 1 and plan["separators"] > 0
    if name in ("ring40", "ring66", "hub"):
        assert straddling


def test_plan_of_a_star_around_the_fixed_keyframe(built):
    """n = 12, fixed = 0, edges (k, 0) for k = 1 .. 11: eleven free vertices, no pair; block 9 sits on rows 63 .. 69."""
    prob = SC.ring(n=12, seed=5)
    prob = SC.with_edges(prob, [(k, 0, 1) for k in range(1, 12)])
    plan = built.essential_graph_plan(prob)
    _assert_blocks_live(prob, plan)
    assert plan["row_of"][10] == 63 and plan["rows"] == 128 and plan["tile_rows"] == 3 and plan["tile_map"][1, 0] >= 0


def test_capacity_error_before_anything_is_written(built):
    """8193 free keyframes on a path: EAO_ERR_INVALID with a message, on the host (no device is touched), the result struct and its arrays untouched."""
    import ctypes as C
    from eao_fusion_amd import _lib
    n = 8194
    Scw = np.tile(np.array([0, 0, 0, 1, 0, 0, 0, 1.0]), (n, 1))
    Scw[:, 4] = np.arange(n)
    has = np.zeros(n, np.uint8)
    edges = np.ascontiguousarray(np.stack([np.arange(1, n), np.arange(0, n - 1), np.ones(n - 1)], axis=1).astype(np.int32))
    P = _lib.EssentialGraphProblem(n, 0, 0, _lib.ptr(Scw), _lib.ptr(has), _lib.ptr(Scw), n - 1, _lib.ptr(edges), 0, None, None)
    oS, oT = np.full((n, 8), 7.0), np.full((n, 16), 7.0, np.float32)
    Rr = _lib.EssentialGraphResult()
    Rr.Scw, Rr.Tiw = _lib.ptr(oS), _lib.ptr(oT)
    Rr.n_active, Rr.lm_iterations = -5, -5
    assert _lib.load().eao_optimize_essential_graph(C.byref(P), C.byref(Rr)) == _lib.EAO_ERR_INVALID
    msg = _lib.load().eao_last_error().decode()
    assert "at most 8192 free keyframes" in msg and "8193" in msg
    assert Rr.n_active == -5 and Rr.lm_iterations == -5 and np.all(oS == 7.0) and np.all(oT == 7.0)
    info = (C.c_int32 * 17)()
    assert _lib.load().eao_essential_graph_plan(C.byref(P), info, None, None, 0) == _lib.EAO_ERR_INVALID
