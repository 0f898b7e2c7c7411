"""The yardstick of the Sim3Solver parity tests (tests/sim3_solver_reference.py) held on its own, without a device: against an independent formulation
(the true transform of noise-free scenes, an SVD solution), the sampling loop's quirk, the iteration formula, what each irregular family claims, and the
two conditions the scenes are held to.  tests/sim3_solver_tolerances.py is kept equal to profiles/sim3_solver_bands.txt."""
import importlib.util
import os
import re

import numpy as np
import pytest

import sim3_solver_reference as R
import sim3_solver_scenes as SC
import sim3_solver_tolerances as TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def bands():
    return _tool("sim3_solver_bands")


def _umeyama(P1, P2, fix_scale):
    """X1 = s R X2 + t by SVD, in float64 (columns are points)"""
    P1, P2 = P1.astype(np.float64), P2.astype(np.float64)
    c1, c2 = P1.mean(axis=1, keepdims=True), P2.mean(axis=1, keepdims=True)
    A, B = P1 - c1, P2 - c2
    U, S, Vt = np.linalg.svd(A @ B.T)
    D = np.diag([1, 1, np.sign(np.linalg.det(U @ Vt))])
    Rm = U @ D @ Vt
    # Horn's asymmetric scale, as upstream computes it: <Pr1, R Pr2> / |R Pr2|^2
    s = 1.0 if fix_scale else float((A * (Rm @ B)).sum() / ((Rm @ B) ** 2).sum())
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = s * Rm, (c1 - s * Rm @ c2)[:, 0]
    return T


@pytest.mark.parametrize("fix_scale", [True, False])
@pytest.mark.parametrize("eigen", ["f64", "f32jacobi", "f64jacobi"])
def test_compute_sim3_recovers_the_true_transform(fix_scale, eigen):
    """noise-free scene, well-spread triples: the true Sim3 to float accuracy, T21 its inverse, and agreement with the SVD solution"""
    prob = SC.scene(n=64, seed=77, fix_scale=fix_scale, noise_px=0.0, outlier_frac=0.0)
    pre = R.prepare(prob)
    true = prob["true_T12"]
    tested = 0
    for tr in SC.drawn_triples(64, 40, 5):
        h = R.compute_sim3(pre["X1c"][tr].T, pre["X2c"][tr].T, fix_scale, eigen)
        ev = h["eigenvalues"]
        if (ev[0] - ev[1]) / (abs(ev[0]) + abs(ev[3])) < 0.05:
            continue
        tested += 1
        scale = np.abs(true).max()
        # float32 points at depth up to 8 carry 5e-7; a triple spanning a metre or more turns that into a few 1e-6 of rotation
        assert np.abs(h["T12"] - true).max() <= 2e-4 * scale, (tr, h["T12"], true)
        assert np.abs(h["T12"].astype(np.float64) @ h["T21"].astype(np.float64) - np.eye(4)).max() <= 1e-5
        um = _umeyama(pre["X1c"][tr].T, pre["X2c"][tr].T, fix_scale)
        assert np.abs(h["T12"] - um).max() <= 2e-4 * scale
        assert h["s"] == 1.0 if fix_scale else abs(float(h["s"]) - np.cbrt(np.linalg.det(true[:3, :3]))) <= 1e-4
    assert tested >= 15


def test_eigen_variants_agree_on_conditioned_hypotheses():
    prob, triples = SC.friendly("n64-fs0")
    pre = R.prepare(prob)
    for tr in triples:
        a, b, c = (R.compute_sim3(pre["X1c"][tr].T, pre["X2c"][tr].T, False, e) for e in ("f64", "f32jacobi", "f64jacobi"))
        ev = a["eigenvalues"]
        assert np.allclose(ev, c["eigenvalues"], rtol=0, atol=1e-9 * abs(ev[0])) and np.allclose(ev, b["eigenvalues"], rtol=0, atol=1e-5 * abs(ev[0]))
        if (ev[0] - ev[1]) / (abs(ev[0]) + abs(ev[3])) >= TOL.GAP_MIN:
            scale = np.abs(a["T12"]).max()
            assert np.abs(a["T12"] - b["T12"]).max() <= TOL.T12_REL * scale and np.abs(a["T12"] - c["T12"]).max() <= TOL.T12_REL * scale


def test_draw_triple_hand_traced():
    """N = 10, positions drawn 4, 4, 4: the first draw yields 4 and writes avail[4] = 9 (size 9); the second reads avail[4] = 9, writes avail[9] = avail[8] = 8 --
    one past the shrunken size -- (size 8); the third reads avail[4] = 9 again: (4, 9, 9)."""
    seq = iter([4, 4, 4])
    asked = []

    def rnd(lo, hi):
        asked.append((lo, hi))
        return next(seq)
    assert R.draw_triple(10, rnd) == (4, 9, 9)
    assert asked == [(0, 9), (0, 8), (0, 7)]
    # drawing the last value first is the one case without a repeat at that position: (9, x, ...) writes avail[9] = avail[9]
    seq = iter([9, 3, 3])
    assert R.draw_triple(10, lambda lo, hi: next(seq)) == (9, 3, 8)


def test_draw_triple_stays_in_range():
    for N in (3, 4, 20, 65):
        rnd = SC.counting_stream(N)
        seen_repeat = False
        for _ in range(3000):
            t = R.draw_triple(N, rnd)
            assert all(0 <= v < N for v in t)
            seen_repeat = seen_repeat or len(set(t)) < 3
        assert seen_repeat or N > 20       # small N: the quirk shows within 3000 draws


def test_ransac_max_iterations_table():
    f = R.ransac_max_iterations
    assert f(20, 0.99, 20, 300) == 1                     # N == min_inliers
    assert f(40, 0.99, 20, 300) == 35                    # epsilon = 0.5: log(0.01) / log(0.875) = 34.49
    assert f(100, 0.99, 20, 300) == 300                  # 573 clamped
    assert f(25, 0.99, 20, 300) == 7                     # epsilon = 0.8: log(0.01) / log(0.488) = 6.42
    assert f(21, 0.99, 20, 300) == 3
    assert f(100, 0.99, 20, 5) == 5
    assert f(1000, 0.99, 6, 300) == 300
    assert f(19, 0.99, 20, 300) == 300 and f(0, 0.99, 6, 300) == 300      # N < min_inliers: the argument, the formula is skipped
    assert f(6, 0.99, 6, 300) == 1


def test_sequential_rule():
    f = R.sequential_rule
    assert f([5, 30, 40], 0, 0, 20, 300, 64) == (1, 1, 2, 30, False)            # returns at the first count above 20; 40 is never seen
    assert f([5, 5, 3], 0, 0, 20, 300, 64) == (-1, 1, 3, 5, False)              # a tie goes to the later one
    assert f([20, 3], 0, 0, 20, 300, 64) == (-1, 0, 2, 20, False)               # 20 is not > 20
    assert f([3, 3, 3, 3, 3], 298, 7, 20, 300, 64) == (-1, -1, 300, 7, True)    # cut by max_its
    assert f([30], 300, 0, 20, 300, 64) == (-1, -1, 300, 0, True)
    assert f([30], 5, 2, 20, 300, 19) == (-1, -1, 5, 2, True)                   # n < min_inliers: untouched


# ---------------------------------------------------------------------- each irregular family does what it claims
def test_small_families_return_no_more():
    for name, n in (("n0", 0), ("n3", 3), ("n19", 19)):
        prob, triples = SC.irregular(name)
        assert len(prob["Xw1"]) == n
        out = R.iterate(prob, None, triples)
        assert out["no_more"] and out["returned"] == -1 and out["state"]["iterations"] == 0 and not out["hyp_inliers"].any()


def test_n_equals_min_inliers():
    prob, triples = SC.irregular("n_equals_min")
    n = len(prob["Xw1"])
    assert n == SC.MIN_INLIERS and R.ransac_max_iterations(n, 0.99, SC.MIN_INLIERS, 300) == 1
    out = R.iterate(prob, None, triples, max_its=1)
    assert out["state"]["iterations"] == 1 and out["no_more"] and out["returned"] == -1      # 20 inliers at most: never > 20


def test_depth_edge_family():
    prob, triples = SC.irregular("depth_edge")
    pre = R.prepare(prob)
    assert pre["X1c"][5, 2] == 0 and not np.isfinite(pre["im1"][5]).all()
    assert pre["X1c"][6, 2] < 0 and pre["X2c"][7, 2] < 0
    out = R.iterate(prob, None, triples, min_inliers=64, max_its=len(triples))
    assert not out["hyp_inlier"][:, 5].any()                   # every comparison with its NaN / inf error is false
    assert out["hyp_inliers"].max() > 20                       # the rest of the scene still closes
    assert any(5 in t for t in triples) and any(6 in t for t in triples)


def test_truncation_family():
    prob, triples = SC.irregular("truncation")
    pre = R.prepare(prob)
    j = SC.TRUNCATION_INDEX
    untruncated = 9.210 * float(prob["sigma2_1"][j])
    assert pre["max1"][j] == 13 and 13.2 < untruncated < 13.3
    out = R.iterate(prob, None, triples, min_inliers=64, max_its=len(triples))
    planted = 0
    for h in range(len(triples)):
        e1, e2 = R.errors(pre, out["hyp_T12"][h], out["hyp_T21"][h])
        if pre["max1"][j] < e1[j] < untruncated and e2[j] < pre["max2"][j]:
            planted += 1
            assert out["hyp_inlier"][h, j] == 0 and out["hyp_inliers"][h] == 63      # an inlier under 9.21 sigma^2, an outlier under the size_t gate
    assert planted >= 1 and pre["max1"][j] < R.errors(pre, out["hyp_T12"][0], out["hyp_T21"][0])[0][j] < untruncated


@pytest.mark.parametrize("eigen", ["f64", "f32jacobi", "f64jacobi"])
def test_pure_translation_family(eigen):
    prob, triples = SC.irregular("pure_translation")
    out = R.iterate(prob, None, triples, eigen=eigen)
    assert np.isnan(out["hyp_T12"][:, :3, :]).all() and np.isnan(out["hyp_T21"][:, :3, :]).all()
    assert not out["hyp_inliers"].any() and out["returned"] == -1
    assert out["state"]["best_inliers"] == 0 and np.isnan(out["state"]["best_T12"][:3]).all()      # 0 >= 0: the NaN transform becomes the best


def test_degenerate_triples_family(bands):
    prob, triples = SC.irregular("degenerate_triples")
    pre = R.prepare(prob)
    assert [len(set(t)) for t in triples[:4]] == [1, 2, 2, 1] and tuple(triples[2][1:]) == (63, 63)
    mid = (pre["X1c"][0].astype(np.float64) + pre["X1c"][2]) / 2
    assert np.abs(pre["X1c"][1] - mid).max() <= 1e-6
    out = R.iterate(prob, None, triples, min_inliers=64, max_its=len(triples))
    cond = bands.conditioned(out["hyp_eigenvalues"])
    assert not cond[:7].any() and cond[7:].all()


def test_scaled_families():
    for name, s in (("scale_1e-3", 1e-3), ("scale_1e3", 1e3)):
        prob, triples = SC.irregular(name)
        out = R.iterate(prob, None, triples, min_inliers=65, max_its=len(triples))
        best = int(np.argmax(out["hyp_inliers"]))
        assert out["hyp_inliers"][best] > 20
        got = np.cbrt(np.linalg.det(out["hyp_T12"][best][:3, :3].astype(np.float64)))
        assert abs(got / s - 1) < 0.05


# ---------------------------------------------------------------------- the bands file, the tolerance file, the two conditions
def test_tolerances_are_the_bands_file(bands):
    fams, consts = bands.parse(os.path.join(ROOT, "profiles", "sim3_solver_bands.txt"))
    assert consts == {"GAP_MIN": TOL.GAP_MIN, "T12_REL": TOL.T12_REL, "MARGIN_REL": TOL.MARGIN_REL}
    assert set(fams) == {name for name, _ in SC.all_families()}
    assert bands.GAP_MIN == TOL.GAP_MIN
    # the file is current: re-measured here on three families, and the constants follow from its rows
    for name in ("n64-fs1", "n2000-fs0", "scale_1e3"):
        line = bands.line_of(name, bands.probe(dict(SC.all_families())[name]), TOL.MARGIN_REL)
        f = line.split()
        assert {f[k]: float(f[k + 1]) for k in range(2, len(f), 2)} == fams[name], name
    t12 = max(max(r["t12_eigen"], r["t12_ulp"]) for r in fams.values())
    err = max(max(r["err_eigen"], r["err_ulp"]) for r in fams.values())
    assert TOL.T12_REL == pytest.approx(4 * t12, rel=2e-3) and TOL.MARGIN_REL == pytest.approx(4 * err, rel=2e-3)
    src = open(os.path.join(ROOT, "tests", "test_gpu_sim3_solver.py")).read()
    assert not re.search(r"\b\d+(\.\d+)?e-\d+\b", src), "a literal tolerance in the GPU test: it belongs in sim3_solver_tolerances.py"


def test_the_two_conditions_hold_on_the_friendly_families(bands):
    fams, _ = bands.parse(os.path.join(ROOT, "profiles", "sim3_solver_bands.txt"))
    for name, _ in SC.FRIENDLY:
        r = fams[name]
        assert r["conditioned"] >= TOL.CONDITIONED_MIN_SHARE * r["hyp"], name
        assert r["in_margin"] <= TOL.IN_MARGIN_MAX_SHARE, name
    assert {int(fams[name]["n"]) for name, _ in SC.FRIENDLY} == {20, 21, 63, 64, 65, 257, 2000}
