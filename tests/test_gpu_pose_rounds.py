"""GPU parity of Optimizer::PoseOptimization round by round, trial by trial, on the scenes of tests/pose_scenes.py: far-off starts whose LM rejects trials in every round,
observation sets that leave rounds 2 - 4 with 0, 1 or 2 level-0 edges, problem sizes on either side of the `< 10` break, a map point in the camera's plane.  The oracle
is run thirteen times per scene (as built + twelve one-ulp perturbations of the inputs); an iteration whose trial count is the same in all of them is DECIDED, and on the
decided prefix of EVERY round the device must make the oracle's decisions.  What the scenes hold is pinned on the CPU by tests/test_pose_scenes_cpu.py, the bounds come
from tools/pose_round_bands.py (profiles/pose_round_bands.txt) through tests/lm_tolerances.py."""
import numpy as np
import pytest

import pose_scenes as S
from lm_tolerances import CHAOTIC_BANDS_ALLOWED, POSE_ROUNDS_CHAOTIC_BAND, POSE_ROUNDS_CHI2_REL, POSE_ROUNDS_LAMBDA_REL, UPDATE_REL

pytestmark = pytest.mark.gpu
SCENES = S.all_scenes()


@pytest.fixture(scope="module")
def gpu():
    import eao_fusion_amd as E
    assert E.load().eao_device_check() == 0, E.load().eao_last_error()
    return E


@pytest.fixture(scope="module")
def reference(oracle):
    """per scene: the problem, the oracle's base run and its decided iterations -- computed once, shared by the tests below, never written to"""
    out = {}
    with np.errstate(all="ignore"):
        for name, (family, fn, args) in SCENES.items():
            p = fn(*args)
            runs = S.oracle_runs(oracle, p)
            out[name] = (p, runs[0], S.decided(runs))
    return out


def check_scene(name, p, r, o, dec):
    bad, worst_c, worst_l = S.compare_rounds(r["trace"], o["trace"], dec, POSE_ROUNDS_CHI2_REL, POSE_ROUNDS_LAMBDA_REL)
    print("%s: decided %s  |chi2| %.2e  |lambda| %.2e  pose %.2e of the update" % (name, dec, worst_c, worst_l, S.pose_excess(r["Tcw"], o["Tcw"], p["Tcw"])))
    assert not bad, "%s: %s" % (name, "; ".join(bad))
    assert r["n_inliers"] == o["n_inliers"], name
    assert np.array_equal(r["outlier"], o["outlier"]), name
    if "plane_outlier" in o:
        assert np.array_equal(r["plane_outlier"], o["plane_outlier"]), name
    bound = CHAOTIC_BANDS_ALLOWED * POSE_ROUNDS_CHAOTIC_BAND[name] if name in POSE_ROUNDS_CHAOTIC_BAND else UPDATE_REL
    assert S.pose_excess(r["Tcw"], o["Tcw"], p["Tcw"]) <= bound, "%s: Tcw is %.3e of the update off the oracle's (bound %.3e)" % (name, S.pose_excess(r["Tcw"], o["Tcw"], p["Tcw"]), bound)


@pytest.mark.parametrize("name", list(SCENES))
def test_every_round_against_the_oracle(gpu, reference, name):
    p, o, dec = reference[name]
    check_scene(name, p, gpu.Optimizer.PoseOptimization(p), o, dec)


@pytest.mark.parametrize("a", S.ALL_EXCLUDED)
def test_no_iteration_without_a_level_0_edge(gpu, reference, a):
    """every edge excluded after round 1: g2o's optimize() returns at once in rounds 2 - 4 (no vertex is active), and the frame keeps the pose it came with"""
    p, o, dec = reference["scattered n=%d seed=%d" % a]
    r = gpu.Optimizer.PoseOptimization(p)
    rs = r["trace"]["round_start"]
    assert len(rs) == 4 and len(r["trace"]["trials"]) == rs[1] == rs[2] == rs[3] == o["trace"]["round_start"][1]
    assert r["lm_iterations"] == rs[1]
    assert np.array_equal(r["Tcw"].view(np.uint32), np.ascontiguousarray(p["Tcw"], np.float32).view(np.uint32)), "the input pose does not come back bit for bit"
    assert r["n_inliers"] == 0 and r["outlier"].all()


def test_the_batch_runs_the_same_rounds(gpu, reference):
    """one eao_pose_optimization_batch call over all scenes (the global-memory sizes go through the single call inside it): every frame's own trace, held like the single call's"""
    names = list(SCENES)
    outs = gpu.Optimizer.PoseOptimizationBatch([reference[k][0] for k in names], traces=True)
    for name, r in zip(names, outs):
        p, o, dec = reference[name]
        check_scene(name, p, r, o, dec)
