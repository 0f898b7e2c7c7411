"""The PnPsolver yardstick (tests/pnp_solver_reference.py) held to the conditions the device tests rest on, without a device.

Two findings shape those tests, and this file keeps them true:
  1. With min_set = 4 (what Relocalization passes) M^T M has a four-dimensional null space and the pose EPnP returns depends on the basis the eigen-solver hands
     back: the yardstick's own variants disagree by O(1) on most hypotheses (test_min4_is_not_pinned_per_hypothesis).  So per-hypothesis parity is asked for
     min_set >= 6 only; at 4 the device tests hold the replay, the sequential rule, Refine on the device's own set, and the outcome on exact-inlier scenes.
  2. From six points up the variants agree to 1e-9 or better ONCE the sign of the PCA axes is fixed (sign_rows); one ulp on the inputs then moves a pose by about 1e-6.
Also: tests/pnp_solver_tolerances.py equals profiles/pnp_solver_bands.txt; the literal upstream loop (Refine at every gate-passing hypothesis) and the once-per-record
form the device computes give identical results; the special lines are reached; the constants fixture (held to the reference text by tests/test_reference_literals.py) equals kernel, yardstick and adapter."""
import os
import re
import sys

import numpy as np
import pytest

import pnp_solver_reference as Y
import pnp_solver_scenes as SC
import pnp_solver_tolerances as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from reference_literals import literals  # noqa: E402

NAMES = [name for name, _ in SC.all_families()]
_runs = {}


def _yardstick_runs(name):
    if name not in _runs:
        _runs[name] = SC.yardstick_runs(SC.FAMILIES[name]())
    return _runs[name]


def test_tolerances_equal_the_bands_file():
    text = open(os.path.join(ROOT, "profiles", "pnp_solver_bands.txt")).read()
    consts = dict(re.findall(r"^constant (\w+) = ([0-9.e+-]+)", text, re.M))
    assert set(consts) == {"RT_BOUND", "MARGIN_REL", "REP_BAND"}
    for k, v in consts.items():
        assert float(v) == getattr(T, k), k
    assert (T.UNCONDITIONED_MAX_SHARE, T.IN_MARGIN_MAX_SHARE, T.MIN4_DISAGREE_MIN_SHARE) == (0.05, 0.01, 0.25)      # set by the issue


@pytest.mark.parametrize("name", SC.PARITY)
def test_parity_family_is_conditioned(name):
    """At most 5 % of the hypotheses unconditioned, at most 1 % of the pairs inside MARGIN_REL, the same outcome under every variant and perturbation; the golden
    file holds exactly these marks and the jacobi variant's results."""
    c = SC.FAMILIES[name]()
    rs = _yardstick_runs(name)
    cond = SC.pose_spread(rs) <= T.RT_BOUND
    assert (~cond).mean() <= T.UNCONDITIONED_MAX_SHARE, (name, int((~cond).sum()), len(cond))
    gate = Y.max_error(c["prob"]).astype(np.float64)
    assert (np.abs(rs[0]["err"] - gate) <= T.MARGIN_REL * gate).mean() <= T.IN_MARGIN_MAX_SHARE
    probs = [c["prob"]] * 3 + [SC.ulp_perturbed(c["prob"], s) for s in SC.ULP_SEEDS]
    variants = ["eigh", "svd", "jacobi"] + ["eigh"] * len(SC.ULP_SEEDS)
    outcomes = []
    for prob, variant, h in zip(probs, variants, rs):
        o = Y.iterate(prob, None, c["sets"], c["min_inliers"], c["max_its"], variant, hyp=h)
        outcomes.append((o["returned"], o["refined"], o["no_more"], tuple(o["records"]), o["state"]["iterations"]))
    assert len(set(outcomes)) == 1, outcomes
    z = np.load(os.path.join(ROOT, "tests", "golden", "pnp_solver", name + ".npz"))
    assert np.array_equal(z["sets"], c["sets"]) and np.array_equal(z["p2d"], c["prob"]["p2d"]) and np.array_equal(z["conditioned"] > 0, cond)
    assert np.abs(z["hyp_R"] - rs[2]["R"]).max() <= 1e-9 and np.abs(z["hyp_t"] - rs[2]["t"]).max() <= 1e-9 and np.array_equal(z["hyp_inliers"], rs[2]["inliers"])
    assert (int(z["returned"]), int(z["refined"]), bool(z["no_more"]), tuple(z["records"]), int(z["iterations"])) == outcomes[2]


@pytest.mark.parametrize("name", SC.MIN4)
def test_min4_is_not_pinned_per_hypothesis(name):
    """The stated reason no per-hypothesis parity is asked at min_set = 4: the yardstick's own eigen-solve variants disagree beyond the band on more than a quarter
    of the hypotheses (on nearly all of them, in fact)."""
    c = SC.FAMILIES[name]()
    base = Y.hypotheses(c["prob"], c["sets"], "eigh")
    spread = SC.pose_spread([base, Y.hypotheses(c["prob"], c["sets"], "svd"), Y.hypotheses(c["prob"], c["sets"], "jacobi")])
    assert (spread > T.RT_BOUND).mean() > T.MIN4_DISAGREE_MIN_SHARE, (name, float((spread > T.RT_BOUND).mean()))


@pytest.mark.parametrize("name", NAMES)
def test_literal_loop_equals_once_per_record(name):
    """Upstream calls Refine on mvbBestInliers at every hypothesis that passes the >= gate; the device refines each best set once.  Refine is deterministic and the
    set changes only at a record, so the two give identical results -- also across calls, where the state carries the set in."""
    c = SC.FAMILIES[name]()
    n = len(c["prob"]["sigma2"])
    st, o = None, 0
    for size in c.get("chunks", (len(c["sets"]),)):
        sets = c["sets"][o:o + size]
        a = Y.iterate(c["prob"], st, sets, c["min_inliers"], c["max_its"], "eigh")
        b = Y.iterate_literal(c["prob"], st, sets, c["min_inliers"], c["max_its"], "eigh", hyp=a.get("hyp"))
        for k in ("returned", "refined", "n_inliers", "no_more", "records"):
            assert a[k] == b[k], (name, k)
        assert np.array_equal(a["Tcw"], b["Tcw"], equal_nan=True) and np.array_equal(a["inlier"], b["inlier"])
        for k in ("iterations", "best_inliers"):
            assert a["state"][k] == b["state"][k]
        assert np.array_equal(a["state"]["best_Tcw"], b["state"]["best_Tcw"], equal_nan=True) and np.array_equal(a["state"]["best_inlier"], b["state"]["best_inlier"])
        st, o = a["state"], o + size
        assert len(st["best_inlier"]) == n


def test_sequencing_scenes_are_what_they_say():
    c = SC.FAMILIES["fail_then_succeed"]()
    o = Y.iterate_literal(c["prob"], None, c["sets"], c["min_inliers"], c["max_its"], "eigh")
    assert o["records"] == [1, 4] and o["returned"] == 4 and o["refined"] == 1 and o["refine_calls"] == 3      # Refine failed at 1 and again at 3
    assert np.array_equal(o["inlier"] > 0, c["true_inlier"])
    c = SC.FAMILIES["carried"]()
    a = Y.iterate(c["prob"], None, c["sets"][:4], c["min_inliers"], c["max_its"], "eigh")
    assert a["returned"] == -1 and a["records"] == [1] and a["state"]["best_inliers"] == 12
    b = Y.iterate_literal(c["prob"], a["state"], c["sets"][4:], c["min_inliers"], c["max_its"], "eigh")
    assert b["records"] == [2] and b["returned"] == 2 and b["refine_calls"] == 2      # hypothesis 0 passed the gate as a non-record: Refine of the carried set
    c = SC.FAMILIES["carried_success"]()
    a = Y.iterate(c["prob"], None, c["sets"][:2], c["min_inliers"], c["max_its"], "eigh")
    b = Y.iterate(c["prob"], a["state"], c["sets"][2:], c["min_inliers"], c["max_its"], "eigh")
    assert a["returned"] == 1 and b["records"] == [] and b["returned"] == 2 and b["refined"] == 1 and np.array_equal(a["Tcw"], b["Tcw"])
    c = SC.FAMILIES["all_outliers_n64"]()
    o = Y.iterate(c["prob"], None, c["sets"], c["min_inliers"], c["max_its"], "eigh")
    assert o["no_more"] and o["returned"] == -1
    c = SC.FAMILIES["n8_n9_below_min"]()
    o = Y.iterate(c["prob"], None, c["sets"], c["min_inliers"], c["max_its"], "eigh")
    assert o["no_more"] and o["returned"] == -1 and o["state"]["iterations"] == 0
    c = SC.FAMILIES["repeat_n65"]()
    assert len(set(c["sets"][0])) < 6
    for name in ("x4_n100", "x4_n257"):      # what test_gpu_pnp_solver.test_outcome_min4_exact rests on
        c = SC.FAMILIES[name]()
        assert (c["min_set"], c["min_inliers"], c["max_its"], len(c["sets"])) == (4, len(c["true_inlier"]) // 2, 35, 35)
        for variant in Y.VARIANTS:
            o = Y.iterate(c["prob"], None, c["sets"], c["min_inliers"], c["max_its"], variant)
            assert o["returned"] >= 0 and o["refined"] == 1 and np.array_equal(o["inlier"] > 0, c["true_inlier"]), (name, variant)


def test_draw_quirk_repeats_an_index():
    """vAvailableIndices[idx] = vAvailableIndices.back() uses the drawn VALUE as the position (:199): sets with a repeated index come out of the sampling loop."""
    sets = SC.draw_sets(np.random.default_rng(0), 12, 6, 400)
    assert sets.min() >= 0 and sets.max() < 12
    assert any(len(set(s)) < 6 for s in sets)


def test_special_lines_are_reached():
    trace = {}
    x = Y.qr_solve(np.zeros((6, 4)), np.ones(6), np.array([1.0, 2.0, 3.0, 4.0]), trace)      # the eta == 0 return leaves X as it was
    assert trace == {"eta_zero": 1} and list(x) == [1.0, 2.0, 3.0, 4.0]
    A = np.arange(24, dtype=np.float64).reshape(6, 4) ** 1.5 + np.eye(6, 4)
    assert np.abs(Y.qr_solve(A, A @ np.array([1.0, -2.0, 0.5, 3.0]), np.zeros(4)) - [1.0, -2.0, 0.5, 3.0]).max() < 1e-9
    rng = np.random.default_rng(5)
    for kind in (1, 2, 3):
        L = rng.normal(size=(6, 10)) * 0.05
        L[:, 0] = 1.0
        Y.find_betas(L, np.ones(6), kind, trace)
        L[:, 0] = -1.0
        Y.find_betas(L, np.ones(6), kind, trace)
        assert trace["approx%d_pos" % kind] >= 1 and trace["approx%d_neg" % kind] >= 1
    c = SC.FAMILIES["x4_n100"]()      # the det < 0 flip and both signs of solve_for_sign inside whole poses
    Y.hypotheses(c["prob"], c["sets"][:12], "jacobi", trace)
    assert trace.get("det_flip", 0) >= 1 and trace.get("sign_flip", 0) >= 1
    # least squares: the stated rank rule drops a vanishing singular value (minimum-norm solution)
    A = np.array([[1.0, 1.0], [1.0, 1.0], [2.0, 2.0]])
    assert np.abs(Y.pinv_rule(A) - np.linalg.pinv(A)).max() < 1e-12
    B = rng.normal(size=(6, 5))
    assert np.abs(Y.pinv_rule(B) - np.linalg.pinv(B)).max() < 1e-10


def test_sign_rule_and_variants_from_six_points():
    """Finding 2: with the sign rule the three variants agree far inside the band on six or more consistent points, on 1 px of noise too."""
    for name in ("n6_n64", "n8_n257"):
        c = SC.FAMILIES[name]()
        idx = np.flatnonzero(c["true_inlier"])[:30]
        poses = [Y.pose_of(c["prob"], idx, v) for v in Y.VARIANTS]
        for R, t, _, _ in poses[1:]:
            assert max(np.abs(R - poses[0][0]).max(), np.abs(t - poses[0][1]).max()) <= 1e-9
    u = Y.sign_rows(np.array([[-0.1, -0.9, 0.3], [0.5, -0.5, 0.1], [0.2, 0.3, -0.9]]))
    assert u[0, 1] > 0 and u[1, 0] > 0 and u[2, 2] > 0      # the largest component positive; the lowest index wins the tie of row 1


RANSAC_TABLE = [      # (N, arguments) -> (min_inliers, max_its), worked by hand from :134-152
    ((100, 0.99, 10, 300, 4, 0.5, 5.991), (50, 35)),
    ((100, 0.99, 8, 300, 4, 0.4, 5.991), (40, 70)),
    ((15, 0.99, 10, 300, 4, 0.5, 5.991), (10, 14)),
    ((10, 0.99, 10, 300, 4, 0.5, 5.991), (10, 1)),
    ((9, 0.99, 10, 300, 4, 0.5, 5.991), (10, 1)),
    ((1000, 0.99, 10, 20, 6, 0.3, 5.991), (300, 20)),
    ((3, 0.99, 2, 300, 4, 0.5, 5.991), (4, 1)),
]


@pytest.mark.parametrize("args, want", RANSAC_TABLE)
def test_ransac_parameters(args, want):
    assert Y.ransac_parameters(*args) == want


def test_kernel_yardstick_and_adapter_spell_the_fixture():
    c = literals("pnp_solver")      # (held to the reference text by tests/test_reference_literals.py)
    src = open(os.path.join(ROOT, "eao_fusion_amd", "csrc", "pnp_internal.h")).read()
    block = src[src.index("// pnp-constants-begin"):src.index("// pnp-constants-end")]
    got = dict(re.findall(r"constexpr \w+ (k\w+) = ([0-9.]+f?);", block))
    assert got == dict(kGaussNewtonIterations=c["GN_ITERATIONS"], kAlphaOne=c["ALPHA_ONE"], kLTwo=c["L_TWO"])
    rest = src.replace(block, "")
    assert "1.0f" not in rest and "2.0f" not in rest
    assert Y.GN_ITERATIONS == int(c["GN_ITERATIONS"]) and Y.ALPHA_ONE.dtype == np.float32 and Y.L_TWO.dtype == np.float32
    assert float(Y.ALPHA_ONE) == float(c["ALPHA_ONE"].rstrip("f")) and float(Y.L_TWO) == float(c["L_TWO"].rstrip("f"))
    reloc = tuple(float(c["RELOC_" + k]) for k in ("PROBABILITY", "MIN_INLIERS", "MAX_ITERATIONS", "MIN_SET", "EPSILON", "TH2"))
    assert SC.RELOCALIZATION == reloc and SC.TH2 == float(c["DEFAULT_TH2"])
    import inspect
    defaults = [p.default for p in list(inspect.signature(Y.ransac_parameters).parameters.values())[1:]]
    assert defaults == [float(c["DEFAULT_PROBABILITY"]), int(c["DEFAULT_MIN_INLIERS"]), int(c["DEFAULT_MAX_ITERATIONS"]), int(c["DEFAULT_MIN_SET"]),
                        float(c["DEFAULT_EPSILON"]), float(c["DEFAULT_TH2"])]
    hdr = open(os.path.join(ROOT, "include", "eaofusion", "PnPsolver.h")).read()
    want = "double probability = %s, int minInliers = %s, int maxIterations = %s, int minSet = %s, float epsilon = %s, float th2 = %s" % tuple(
        c["DEFAULT_" + k] for k in ("PROBABILITY", "MIN_INLIERS", "MAX_ITERATIONS", "MIN_SET", "EPSILON", "TH2"))
    assert want in hdr
