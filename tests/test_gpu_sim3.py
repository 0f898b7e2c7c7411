"""Optimizer::OptimizeSim3 on the device (eao_optimize_sim3, csrc/sim3.hip) against the numpy restatement tests/sim3_reference.py,
the golden fixtures tests/golden/sim3/*.npz, the batched entry point against single calls, and the class surface
include/eaofusion/OptimizerSim3.h against stand-ins."""
import glob
import os
import subprocess

import numpy as np
import pytest

import sim3_reference as R
import sim3_scenes as SC
from lm_tolerances import UPDATE_REL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FAMILIES = SC.FAMILIES


def _update_norm(prob, ref):
    return max(np.abs(ref["q"] - prob["q"]).max(), np.abs(ref["t"] - prob["t"]).max(), abs(ref["s"] - prob["s"]))


def _displacement(a, b):
    return max(np.abs(a["q"] - b["q"]).max(), np.abs(a["t"] - b["t"]).max(), abs(a["s"] - b["s"]))


def _schedule(o):
    return (tuple(int(v) for v in o["iters"]), int(o["n_inliers"]), bool(o["early_exit"]), o["removed"].tobytes())


@pytest.mark.gpu
@pytest.mark.parametrize("name,kw", FAMILIES, ids=["%s-%d-%d" % (f, k["n"], k["seed"]) for f, k in FAMILIES])
def test_sim3_parity(name, kw):
    from eao_fusion_amd.optimizer import optimize_sim3
    prob = SC.scene(**kw)
    ref = R.optimize_sim3(prob)
    got = optimize_sim3(prob)
    upd = _update_norm(prob, ref)
    assert int(got["n_inliers"]) == int(ref["n_inliers"])
    assert bool(got["early_exit"]) == bool(ref["early_exit"])
    if SC.family_key(name, kw) not in SC.ITERS_UNSTABLE:     # (there the reference's own iteration counts are rounding: sim3_scenes.py)
        assert list(got["iters"]) == list(ref["iters"])
    assert np.array_equal(got["removed"], ref["removed"])
    if ref["early_exit"]:
        # nothing is written back: the initial S12, bit for bit
        assert np.array_equal(got["q"], np.asarray(prob["q"], np.float64)) and np.array_equal(got["t"], np.asarray(prob["t"], np.float64))
        assert got["s"] == float(prob["s"])
        return
    tol = UPDATE_REL * upd + 1e-15
    assert np.abs(got["q"] - ref["q"]).max() <= tol, (got["q"], ref["q"], upd)
    assert np.abs(got["t"] - ref["t"]).max() <= tol, (got["t"], ref["t"], upd)
    assert abs(got["s"] - ref["s"]) <= tol
    if prob["fix_scale"]:
        assert got["s"] == float(prob["s"])


def _golden_files():
    return sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "sim3", "sim3_*.npz")))


@pytest.mark.gpu
def test_sim3_golden():
    from eao_fusion_amd.optimizer import optimize_sim3
    files = _golden_files()
    assert files, "tests/golden/sim3/sim3_*.npz missing (tools/gen_golden_sim3.py)"
    for fn in files:
        z = np.load(fn)
        prob = dict(T1w=z["T1w"], T2w=z["T2w"], Xw1=z["Xw1"], Xw2=z["Xw2"], obs1=z["obs1"], obs2=z["obs2"], inv_sigma2_1=z["inv_sigma2_1"],
                    inv_sigma2_2=z["inv_sigma2_2"], K1=z["K1"], K2=z["K2"], q=z["q0"], t=z["t0"], s=float(z["s0"]), th2=float(z["th2"]),
                    fix_scale=bool(z["fix_scale"]))
        got = optimize_sim3(prob)
        assert int(got["n_inliers"]) == int(z["n_inliers"]), fn
        assert list(got["iters"]) == list(z["iters"]), fn
        assert bool(got["early_exit"]) == bool(z["early_exit"]), fn
        assert np.array_equal(got["removed"], z["removed"]), fn
        upd = max(np.abs(z["q"] - z["q0"]).max(), np.abs(z["t"] - z["t0"]).max(), abs(float(z["s"]) - float(z["s0"])))
        tol = UPDATE_REL * upd + 1e-15
        assert np.abs(got["q"] - z["q"]).max() <= tol and np.abs(got["t"] - z["t"]).max() <= tol and abs(got["s"] - float(z["s"])) <= tol, fn


@pytest.mark.gpu
def test_sim3_batch_bit_identical_to_single_calls():
    from eao_fusion_amd.optimizer import optimize_sim3, optimize_sim3_batch
    kws = [dict(n=20 + 37 * k, seed=900 + k, fix_scale=(k % 2 == 0), outlier_frac=0.15 * (k % 3 == 0)) for k in range(13)]
    kws += [dict(n=0, seed=950, fix_scale=True), dict(n=14, seed=51, fix_scale=True, outlier_frac=0.6), dict(n=2000, seed=951, fix_scale=False)]
    probs = [SC.scene(**kw) for kw in kws]
    assert len(probs) == 16
    batch = optimize_sim3_batch(probs)
    for p, b in zip(probs, batch):
        s = optimize_sim3(p)
        assert np.array_equal(s["q"], b["q"]) and np.array_equal(s["t"], b["t"]) and s["s"] == b["s"]
        assert np.array_equal(s["removed"], b["removed"]) and s["n_inliers"] == b["n_inliers"]
        assert np.array_equal(s["iters"], b["iters"]) and s["early_exit"] == b["early_exit"]


@pytest.fixture(scope="module")
def class_driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sim3") / "sim3_driver")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-DSIM3_RUN", "-DEAOFUSION_FORCE_CV_COMPAT", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "sim3", "sim3_driver.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "eao_fusion_amd"), "-leaofusion_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "eao_fusion_amd"), "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    return exe


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(n=120, seed=71, fix_scale=True, outlier_frac=0.2), dict(n=80, seed=72, fix_scale=False),
                                dict(n=14, seed=51, fix_scale=True, outlier_frac=0.6)], ids=["rgbd-outliers", "mono", "early-exit"])
def test_sim3_class_surface(class_driver, kw):
    prob = SC.scene(**kw)
    txt, index = SC.keyframe_scene(prob, seed=kw["seed"])
    out = subprocess.run([class_driver, "run"], input=txt, capture_output=True, text=True, check=True).stdout.split("\n")
    ret = int(out[0].split()[1])
    nulled = [int(v) for v in out[1].split()[1:]]
    S = [float(v) for v in out[2].split()[1:]]
    ref = R.optimize_sim3(prob)
    assert ret == ref["n_inliers"]
    assert nulled == [index[k] for k in np.nonzero(ref["removed"])[0]]      # only walked entries, exactly the removed ones
    q, t, s = np.array(S[:4]), np.array(S[4:7]), S[7]
    if ref["early_exit"]:
        assert np.array_equal(q, prob["q"]) and np.array_equal(t, prob["t"]) and s == float(prob["s"])
    else:
        tol = UPDATE_REL * _update_norm(prob, ref) + 1e-15
        assert np.abs(q - ref["q"]).max() <= tol and np.abs(t - ref["t"]).max() <= tol and abs(s - ref["s"]) <= tol
        assert not np.array_equal(q, prob["q"])
