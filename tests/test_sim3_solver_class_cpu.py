"""The class surface include/eaofusion/Sim3Solver.h without a device: compiled with g++ against the stand-ins of tests/cpp/sim3_solver/sim3_solver_driver.cpp
and linked with tests/cpp/sim3_solver/sim3_solver_stub.cpp, which prints every library call and answers by a made-up rule.  Checked: the constructor's
filters and the mvnIndices1 mapping, SetRansacParameters, the draws each iterate call consumes (3 * min(n, remaining), none when N < minInliers) and that
they are the reference's sampling loop over the same generator, bNoMore both ways, vbInliers of length mN1 filled through mvnIndices1."""
import os
import subprocess

import numpy as np
import pytest

import sim3_solver_keyframes as KF
import sim3_solver_reference as R
import sim3_solver_scenes as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 424242


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sim3_solver") / "sim3_solver_surface")
    src = os.path.join(ROOT, "tests", "cpp", "sim3_solver")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-DEAOFUSION_FORCE_CV_COMPAT", "-I", os.path.join(ROOT, "include"),
                           os.path.join(src, "sim3_solver_driver.cpp"), os.path.join(src, "sim3_solver_stub.cpp"), "-o", exe])
    return exe


def _run(driver, prob, script, seed=7):
    txt, index, N1 = KF.candidate_text(prob, seed=seed)
    out = subprocess.run([driver, "surface"], input=txt + "%d\n" % SEED + script, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout.strip().split("\n"), index, N1


def _stub(n, triples, state, min_inliers, max_its):
    """the stub's answer (tests/cpp/sim3_solver/sim3_solver_stub.cpp) restated: counts, then the sequential rule"""
    counts = [(7 * a + 3 * b + c) % (n + 1) for a, b, c in triples]
    return counts, R.sequential_rule(counts, state[0], state[1], min_inliers, max_its, n)


def test_constructor_filters_and_mapping(driver):
    prob = SC.scene(n=30, seed=31, fix_scale=False)
    lines, index, N1 = _run(driver, prob, "iterate 2\n")
    head = lines[0].split()
    assert head[:3] == ["constructed", "n", "30"] and [int(v) for v in head[head.index("indices") + 1:]] == index
    assert N1 > 30 + 6 and index != list(range(30))
    # the default SetRansacParameters(0.99, 6, 300) of the constructor: epsilon = 6 / 30
    assert int(head[head.index("maxits") + 1]) == R.ransac_max_iterations(30, 0.99, 6, 300)
    call = lines[1].split()
    assert call[:6] == ["call", "n", "30", "fix", "0", "min"]
    sig = call[call.index("sigma") + 1:call.index("xw1")]
    assert [tuple(np.float32(v) for v in s.split("/")) for s in sig] == list(zip(prob["sigma2_1"], prob["sigma2_2"]))      # mvLevelSigma2[octave], in index order
    xw = call[call.index("xw1") + 1:call.index("triples")]
    assert np.array_equal(np.array(xw, np.float32), prob["Xw1"][:, 0])


def test_draws_returns_and_no_more(driver):
    prob = SC.scene(n=30, seed=32, fix_scale=True)
    n = 30
    script = "params 0.99 20 12\niterate 5\niterate 5\niterate 5\niterate 5\nparams 0.99 28 7\nfind\n"
    lines, index, N1 = _run(driver, prob, script)
    rnd = KF.CountingRandom(SEED)
    max_its = R.ransac_max_iterations(n, 0.99, 20, 12)
    assert lines[1] == "params maxits %d iterations 0" % max_its and max_its == 12
    state, pos = (0, 0), 2
    seen_return = seen_no_more = False
    for want_n in (5, 5, 5, 5):
        n_hyp = min(want_n, max_its - state[0])
        triples = [R.draw_triple(n, rnd) for _ in range(n_hyp)]
        call = lines[pos].split()
        assert call[0] == "call" and int(call[call.index("nhyp") + 1]) == n_hyp and int(call[call.index("iterations") + 1]) == state[0]
        assert [int(v) for v in call[call.index("triples") + 1:]] == [v for t in triples for v in t]       # the reference's sampling loop over the same generator
        counts, (ret, bk, it, best, no_more) = _stub(n, triples, state, 20, max_its)
        res = lines[pos + 1].split()
        get = lambda k: res[res.index(k) + 1]       # noqa: E731
        assert res[0] == "iterate" and int(get("draws")) == rnd.calls and int(get("iterations")) == it and int(get("size")) == N1
        assert int(get("nomore")) == int(no_more) and int(get("empty")) == int(ret < 0)
        vb = [int(v) for v in res[res.index("vb") + 1:]]
        pos += 2
        if ret >= 0:
            seen_return = True
            assert int(get("ninliers")) == counts[ret] and vb == [index[i] for i in range(counts[ret])]      # filled through mvnIndices1
            T = [float(v) for v in lines[pos].split()[1:]]
            assert T == [100.0 * ret + k for k in range(16)]
            b = lines[pos + 1].split()
            assert (float(b[2]), float(b[4]), float(b[6]), b[8], b[9]) == (10.0 * ret, 1000.0 * ret + 2, 1.0 + ret, "3", "3")
            pos += 2
        else:
            assert int(get("ninliers")) == 0 and vb == []
        seen_no_more = seen_no_more or no_more
        state = (it, best)
    assert state[0] == 12 and seen_no_more and seen_return
    # SetRansacParameters resets mnIterations and restates the formula; find = iterate(mRansacMaxIts)
    max_its = R.ransac_max_iterations(n, 0.99, 28, 7)
    assert lines[pos] == "params maxits %d iterations 0" % max_its
    call = lines[pos + 1].split()
    assert int(call[call.index("nhyp") + 1]) == max_its and int(call[call.index("min") + 1]) == 28


def test_too_few_correspondences_draw_nothing(driver):
    prob = SC.scene(n=19, seed=33, fix_scale=True)
    lines, index, N1 = _run(driver, prob, "params 0.99 20 300\niterate 5\nfind\n")
    assert lines[1] == "params maxits 300 iterations 0"          # N < minInliers: the formula is skipped
    assert not any(l.startswith("call") for l in lines)        # iterate returns before it draws or calls
    for l in lines[2:]:
        f = l.split()
        assert f[f.index("draws") + 1] == "0" and f[f.index("empty") + 1] == "1" and f[f.index("size") + 1] == str(N1)
    assert lines[2].split()[4] == "1"                             # bNoMore
