"""Optimizer::OptimizeSim3 on the device (eao_optimize_sim3, csrc/sim3.hip) against the numpy restatement tests/sim3_reference.py -- on
the friendly families and on the irregular correspondence sets of sim3_scenes.IRREGULAR --, the golden fixtures tests/golden/sim3/*.npz,
the batched entry point against single calls (16 problems, and 600: more workgroups than CUs), independence of what the calling thread ran
before, and the class surface include/eaofusion/OptimizerSim3.h against stand-ins."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

import sim3_reference as R
import sim3_scenes as SC
from lm_tolerances import CHAOTIC_BANDS_ALLOWED, UPDATE_REL
from sim3_child import result_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FAMILIES = SC.FAMILIES


def _update_norm(prob, ref):
    return max(np.abs(ref["q"] - prob["q"]).max(), np.abs(ref["t"] - prob["t"]).max(), abs(ref["s"] - prob["s"]))


def _displacement(a, b):
    return max(np.abs(a["q"] - b["q"]).max(), np.abs(a["t"] - b["t"]).max(), abs(a["s"] - b["s"]))


def _schedule(o):
    return (tuple(int(v) for v in o["iters"]), int(o["n_inliers"]), bool(o["early_exit"]), o["removed"].tobytes())


def _assert_parity(prob, ref, got, iters_unstable=False, banded=False):
    """The bar of every parity test here: removed bit-equal, n_inliers and early_exit equal, the iteration counts equal unless the family is in
    an instability table, q / t / s within UPDATE_REL of the update, the initial S12 bit for bit on early exit, s untouched under fix_scale.
    banded: the yardstick itself moves by more than UPDATE_REL of its update under one ulp on this family; the bound is then
    CHAOTIC_BANDS_ALLOWED of that band, measured here from ulp_perturbed seeds 0..3 (the pattern of test_gpu_lm_conditioning.py)."""
    upd = _update_norm(prob, ref)
    assert int(got["n_inliers"]) == int(ref["n_inliers"])
    assert bool(got["early_exit"]) == bool(ref["early_exit"])
    if not iters_unstable:     # (there the reference's own iteration counts are rounding: sim3_scenes.py)
        assert list(got["iters"]) == list(ref["iters"])
    assert np.array_equal(got["removed"], ref["removed"])
    if ref["early_exit"]:
        # nothing is written back: the initial S12, bit for bit
        assert np.array_equal(got["q"], np.asarray(prob["q"], np.float64)) and np.array_equal(got["t"], np.asarray(prob["t"], np.float64))
        assert got["s"] == float(prob["s"])
        return
    tol = UPDATE_REL * upd + 1e-15
    if banded:
        band = max(_displacement(ref, R.optimize_sim3(SC.ulp_perturbed(prob, s))) for s in range(4))
        print("\n[sim3 banded] GPU - yardstick %.3e, update %.3e, the yardstick's own one-ulp band %.3e" % (_displacement(got, ref), upd, band))
        assert band > UPDATE_REL * upd, "not a banded family: hold it to UPDATE_REL"
        tol = CHAOTIC_BANDS_ALLOWED * band
    assert np.abs(got["q"] - ref["q"]).max() <= tol, (got["q"], ref["q"], upd)
    assert np.abs(got["t"] - ref["t"]).max() <= tol, (got["t"], ref["t"], upd)
    assert abs(got["s"] - ref["s"]) <= tol
    if prob["fix_scale"]:
        assert got["s"] == float(prob["s"])


@pytest.mark.gpu
@pytest.mark.parametrize("name,kw", FAMILIES, ids=["%s-%d-%d" % (f, k["n"], k["seed"]) for f, k in FAMILIES])
def test_sim3_parity(name, kw):
    from eao_fusion_amd.optimizer import optimize_sim3
    prob = SC.scene(**kw)
    _assert_parity(prob, R.optimize_sim3(prob), optimize_sim3(prob), iters_unstable=SC.family_key(name, kw) in SC.ITERS_UNSTABLE)


@pytest.mark.gpu
@pytest.mark.parametrize("name,kw,edit", SC.IRREGULAR, ids=SC.irregular_ids())
def test_sim3_parity_irregular(name, kw, edit):
    """The same bar on the irregular correspondence sets: points behind either camera, exactly ten and nine survivors, the 5-iteration
    budget used up, zero information, near-zero depth, extreme scales, other th2, a non-unit start, duplicates, removed sets on one
    thread's stride and one whole wave, n at wave and workgroup edges and at 20000 (tests/test_sim3_reference_cpu.py holds each family to
    what it claims)."""
    from eao_fusion_amd.optimizer import optimize_sim3
    prob = SC.irregular_scene(kw, edit)
    key = SC.family_key(name, kw)
    _assert_parity(prob, R.optimize_sim3(prob), optimize_sim3(prob), iters_unstable=key in SC.IRREGULAR_ITERS_UNSTABLE, banded=key in SC.IRREGULAR_BANDED)


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


def _same_result(a, b):
    return result_bytes(a) == result_bytes(b)


def _pool():
    """IRREGULAR + FAMILIES as (problem, iteration counts unstable, banded), the 20000-correspondence family apart."""
    pool, large = [], None
    for name, kw, edit in list(SC.IRREGULAR) + [(n, k, None) for n, k in FAMILIES]:
        key = SC.family_key(name, kw)
        entry = (SC.irregular_scene(kw, edit), key in SC.IRREGULAR_ITERS_UNSTABLE or key in SC.ITERS_UNSTABLE, key in SC.IRREGULAR_BANDED)
        if kw["n"] > 2000:
            large = entry
        else:
            pool.append(entry)
    return pool, large


@pytest.mark.gpu
def test_sim3_large_mixed_batch_bit_identical_to_single_calls():
    """600 problems in one launch -- more workgroups than the device has CUs, so they queue behind one another --, drawn cyclically from
    IRREGULAR + FAMILIES (empty and early-exit problems in between, one of 20000 correspondences in the middle): every result bit-identical
    to a single call of the same problem, one in ten also held to the yardstick."""
    from eao_fusion_amd.optimizer import optimize_sim3, optimize_sim3_batch
    pool, large = _pool()
    nb = 600
    assert nb > 2 * 256      # an MI355X has 256 CUs
    which = [(k + k // len(pool)) % len(pool) for k in range(nb)]     # cyclic, each round starting one further on
    which[nb // 2 + 1] = -1
    entries = [large if w < 0 else pool[w] for w in which]
    ns = [len(e[0]["Xw1"]) for e in entries]
    assert max(ns) == 20000 and sorted(ns)[-2] <= 2000 and ns.count(0) >= 5
    batch = optimize_sim3_batch([e[0] for e in entries])
    single, refs = {}, {}
    for k, (w, e, b) in enumerate(zip(which, entries, batch)):
        if w not in single:
            single[w] = optimize_sim3(e[0])
        assert _same_result(single[w], b), (k, w)
        if k % 10 == 0:
            if w not in refs:
                refs[w] = R.optimize_sim3(e[0])
            _assert_parity(e[0], refs[w], b, iters_unstable=e[1], banded=e[2])
    assert any(r["early_exit"] for r in refs.values()) and len(refs) >= 20


@pytest.mark.gpu
def test_sim3_result_does_not_depend_on_what_the_thread_ran_before():
    """One thread's stream and staging buffers (thread_local in csrc/sim3.hip) grow with the largest problem seen and are reused: 20000 -> 0 ->
    11 -> 2000 -> 20000 -> an early exit of 14, then the same problems in reverse order.  Every problem's result is bit-identical both times,
    and equal to that of a process that has run nothing else."""
    from eao_fusion_amd.optimizer import optimize_sim3
    probs = [SC.irregular_scene(kw, edit) for kw, edit in SC.CALL_ORDER]
    assert [len(p["Xw1"]) for p in probs] == [20000, 0, 11, 2000, 20000, 14]
    forward = [result_bytes(optimize_sim3(p)) for p in probs]
    backward = [result_bytes(optimize_sim3(p)) for p in reversed(probs)][::-1]
    assert forward == backward
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT] + [v for v in [os.environ.get("PYTHONPATH")] if v]))
    for k in range(len(probs)):     # one child at a time, each a fresh process (never an exec over this one, which holds the GPU)
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "sim3_child.py"), str(k)], capture_output=True, text=True, env=env, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        assert bytes.fromhex(out.stdout.strip().split("\n")[-1]) == forward[k], k
    early = optimize_sim3(probs[5])
    assert early["early_exit"] and not optimize_sim3(probs[2])["early_exit"]


@pytest.fixture(scope="module")
def class_driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sim3") / "sim3_driver")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-DSIM3_RUN", "-DEAOFUSION_FORCE_CV_COMPAT", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "sim3", "sim3_driver.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "eao_fusion_amd"), "-leaofusion_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "eao_fusion_amd"), "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    return exe


def _irregular_entry(name):
    (kw, edit), = [(kw, edit) for n, kw, edit in SC.IRREGULAR if n == name]
    return kw, edit


# (scene() arguments, edit, skipped entries among the keyframe's matches or None for keyframe_scene's default)
CLASS_CASES = [(dict(n=120, seed=71, fix_scale=True, outlier_frac=0.2), None, None), (dict(n=80, seed=72, fix_scale=False), None, None),
               (dict(n=14, seed=51, fix_scale=True, outlier_frac=0.6), None, None),
               _irregular_entry("behind_cam2") + (None,), _irregular_entry("behind_cam1") + (None,),
               _irregular_entry("ten_survive") + (75,)]      # 15 correspondences among 75 entries the walk skips: 5 : 1


@pytest.mark.gpu
@pytest.mark.parametrize("kw,edit,n_extra", CLASS_CASES, ids=["rgbd-outliers", "mono", "early-exit", "behind-camera-2", "behind-camera-1", "ten-survivors"])
def test_sim3_class_surface(class_driver, kw, edit, n_extra):
    prob = SC.irregular_scene(kw, edit)
    txt, index = SC.keyframe_scene(prob, seed=kw["seed"], n_extra=n_extra)
    out = subprocess.run([class_driver, "run"], input=txt, capture_output=True, text=True, check=True).stdout.split("\n")
    ret = int(out[0].split()[1])
    nulled = [int(v) for v in out[1].split()[1:]]
    S = [float(v) for v in out[2].split()[1:]]
    ref = R.optimize_sim3(prob)
    if n_extra is not None:
        assert n_extra >= 5 * len(prob["Xw1"]) and ref["n_inliers"] == 10 and ref["removed"].sum() == 5
    assert ret == ref["n_inliers"]
    assert nulled == [index[k] for k in np.nonzero(ref["removed"])[0]]      # only walked entries, exactly the removed ones
    q, t, s = np.array(S[:4]), np.array(S[4:7]), S[7]
    if ref["early_exit"]:
        assert np.array_equal(q, prob["q"]) and np.array_equal(t, prob["t"]) and s == float(prob["s"])
    else:
        tol = UPDATE_REL * _update_norm(prob, ref) + 1e-15
        assert np.abs(q - ref["q"]).max() <= tol and np.abs(t - ref["t"]).max() <= tol and abs(s - ref["s"]) <= tol
        assert not np.array_equal(q, prob["q"])
