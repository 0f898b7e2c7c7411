"""The class surface include/eaofusion/Initializer.h without a device: compiled with g++ against the stand-ins of tests/cpp/initializer/initializer_driver.cpp and
linked with tests/cpp/initializer/initializer_stub.cpp, which prints the library call and answers by a made-up rule.  Checked against the yardstick's host part
(tests/initializer_reference.py): the pair list, the sets of the draw loop over the same generator (one SeedRandOnce(0), 8 * iterations draws, each over the shrinking
range), the arguments passed, and the shapes of R21 / t21 / vP3D / vbTriangulated on true and on false."""
import os
import subprocess

import numpy as np
import pytest

import initializer_frames as FR
import initializer_reference as R
import initializer_scenes as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("initializer") / "initializer_surface")
    src = os.path.join(ROOT, "tests", "cpp", "initializer")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-DEAOFUSION_FORCE_CV_COMPAT", "-I", os.path.join(ROOT, "include"),
                           os.path.join(src, "initializer_driver.cpp"), os.path.join(src, "initializer_stub.cpp"), "-o", exe])
    return exe


def _run(driver, prob, sigma, randi):
    txt, v12 = FR.frames_text(prob, sigma=sigma, randi=randi)
    out = subprocess.run([driver], input=txt, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    return FR.parse_result(out.stdout), v12


def _randi(n, iterations, seed):
    rng = np.random.default_rng(seed)
    return [int(rng.integers(0, n - j)) for _ in range(iterations) for j in range(8)]


def test_pair_list_sets_and_arguments(driver):
    prob = SC.scene(n=30, seed=41, iterations=1)
    n, iterations = 30, 5
    randi = _randi(n, iterations, 7)
    got, v12 = _run(driver, prob, 1.0, randi)
    assert (got["seeds"], got["draws"], got["bad"]) == (1, 8 * iterations, 0)      # one SeedRandOnce(0); every draw over 0 .. size-1 of the shrinking list
    call = got["call"]
    val = lambda k, cnt=1: call[call.index(k) + 1:call.index(k) + 1 + cnt]      # noqa: E731
    assert [int(v) for v in val("n1") + val("n2") + val("N")] == [len(prob["keys1"]), len(prob["keys2"]), n]
    assert [np.float32(v) for v in val("K", 4)] == [np.float32(v) for v in prob["K"]]
    assert (np.float32(val("sigma")[0]), np.float32(val("minparallax")[0]), int(val("mintri")[0]), int(val("iterations")[0])) == (1.0, R.MIN_PARALLAX, R.MIN_TRIANGULATED, iterations)
    assert np.array_equal(np.array(val("keys1", 2 * len(prob["keys1"])), np.float32), prob["keys1"].reshape(-1))
    assert np.array_equal(np.array(val("keys2", 2 * len(prob["keys2"])), np.float32), prob["keys2"].reshape(-1))
    from eao_fusion_amd.initializer import pairs_of
    pairs = pairs_of(v12)
    assert np.array_equal(pairs, prob["matches12"]) and [int(v) for v in val("matches", 2 * n)] == list(pairs.reshape(-1))
    it = iter(randi)
    want = R.draw_sets(n, iterations, lambda lo, hi: next(it))
    assert [int(v) for v in val("sets", 8 * iterations)] == list(want.reshape(-1))
    assert all(len(set(row)) == 8 for row in want)


def test_outputs_on_true_and_false(driver):
    prob = SC.scene(n=30, seed=42, iterations=1)
    n1, randi = len(prob["keys1"]), _randi(30, 2, 8)
    got, _ = _run(driver, prob, 1.0, randi)                 # returned
    assert got["returned"] and got["R21"].shape == (3, 3) and got["t21"].shape == (3,)
    assert np.array_equal(got["R21"].reshape(-1), np.arange(1, 10, dtype=np.float32)) and np.array_equal(got["t21"], np.arange(10, 13, dtype=np.float32))
    assert got["p3d"].shape == (n1, 3) and np.array_equal(got["p3d"], np.arange(n1, dtype=np.float32)[:, None] * np.array([1, 2, 3], np.float32))
    assert np.array_equal(got["triangulated"], np.arange(n1) % 3 == 0)
    got, _ = _run(driver, prob, 2.0, randi)                 # ReconstructF returns false: R21 / t21 empty (:501-502), the vectors untouched
    assert not got["returned"] and got["R21"].size == 0 and got["t21"].size == 0
    assert np.array_equal(got["p3d"], [[-1, -2, -3]]) and list(got["triangulated"]) == [True]
    for sigma in (3.0, 4.0):                                # ReconstructH returns false, and no model: everything as the caller left it
        got, _ = _run(driver, prob, sigma, randi)
        assert not got["returned"] and got["R21"].shape == (2, 2) and got["t21"].shape == (2, 2)
        assert np.array_equal(got["p3d"], [[-1, -2, -3]]) and list(got["triangulated"]) == [True]


def test_fewer_than_eight_matches_throw(driver):
    prob = SC.scene(n=30, seed=43, iterations=1)
    prob["matches12"] = prob["matches12"][:7]
    txt, _ = FR.frames_text(prob, sigma=1.0, randi=[])
    out = subprocess.run([driver], input=txt, capture_output=True, text=True)
    assert out.returncode != 0 and "call" not in out.stdout
