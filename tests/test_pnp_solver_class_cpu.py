"""The class surface include/eaofusion/PnPsolver.h without a device: compiled with g++ against the stand-ins of tests/cpp/pnp_solver/pnp_solver_driver.cpp and
linked with tests/cpp/pnp_solver/pnp_solver_stub.cpp, which prints every library call and answers by a made-up rule.  Checked: the constructor's two filters and
the mvKeyPointIndices mapping, SetRansacParameters' arithmetic on a table of (N, arguments), the || of the loop count, the draws (the reference's sampling loop with
its quirk over the same generator, all of a call's draws before the call), vbInliers sized to the match vector and filled through mvKeyPointIndices, cleared otherwise."""
import os
import subprocess

import numpy as np
import pytest

import pnp_solver_frames as FR
import pnp_solver_reference as Y
import pnp_solver_scenes as SC
from test_pnp_solver_reference_cpu import RANSAC_TABLE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 424242


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pnp_solver") / "pnp_solver_surface")
    src = os.path.join(ROOT, "tests", "cpp", "pnp_solver")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-DEAOFUSION_FORCE_CV_COMPAT", "-I", os.path.join(ROOT, "include"),
                           os.path.join(src, "pnp_solver_driver.cpp"), os.path.join(src, "pnp_solver_stub.cpp"), "-o", exe])
    return exe


def _run(driver, prob, script, seed=7):
    txt, index, total = FR.candidate_text(prob, seed=seed)
    out = subprocess.run([driver, "surface"], input=txt + "%d\n" % SEED + script, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout.strip().split("\n"), index, total


def _field(words, key, count=1):
    i = words.index(key)
    return words[i + 1] if count == 1 else words[i + 1:i + 1 + count]


def _stub(n, sets, state, min_inliers, max_its):
    """the stub's answer (tests/cpp/pnp_solver/pnp_solver_stub.cpp) restated: counts, flags, its Refine, then the sequential rule"""
    counts = [int(sum((i + 1) * int(v) for i, v in enumerate(s)) % (n + 1)) for s in sets]
    flags = [(np.arange(n) < c).astype(np.uint8) for c in counts]
    Tcw = [(100.0 * c + np.arange(16)).astype(np.float32).reshape(4, 4) for c in counts]

    def refine_of(f):
        c = int(f.sum())
        r = min(n, c + (1 if c % 3 == 0 else 0))
        return r > min_inliers, (-(100.0 * c + np.arange(16))).astype(np.float32).reshape(4, 4), (np.arange(n) < r).astype(np.uint8), r

    return Y.sequential_rule(n, counts, flags, Tcw, refine_of, state, min_inliers, max_its)


def test_constructor_filters_and_mapping(driver):
    c = SC.FAMILIES["n6_n64"]()
    prob = c["prob"]
    lines, index, total = _run(driver, prob, "iterate 2\n")
    head = lines[0].split()
    assert head[:3] == ["constructed", "n", "64"] and [int(v) for v in head[head.index("indices") + 1:]] == index
    assert total > 64 + 6 and index != list(range(64))      # entries without a map point and with a bad one were filtered
    # the default SetRansacParameters() of the constructor
    mi, mx = Y.ransac_parameters(64)
    assert (int(_field(head, "min")), int(_field(head, "maxits")), int(_field(head, "set"))) == (mi, mx, 4)
    call = lines[1].split()
    assert call[:3] == ["call", "n", "64"]
    assert np.array_equal(np.array(call[call.index("sigma") + 1:call.index("x")], np.float32), prob["sigma2"])      # mvLevelSigma2[octave], in index order
    assert np.array_equal(np.array(call[call.index("x") + 1:call.index("u")], np.float32), prob["p3d_w"][:, 0])
    assert np.array_equal(np.array(call[call.index("u") + 1:call.index("sets")], np.float32), prob["p2d"][:, 0])
    assert np.array_equal(np.array(_field(call, "K", 4), np.float32), np.asarray(prob["K"], np.float32)) and np.float32(_field(call, "th2")) == np.float32(5.991)


@pytest.mark.parametrize("args, want", RANSAC_TABLE)
def test_set_ransac_parameters(driver, args, want):
    N, p, mi, mx, ms, eps, th2 = args
    c = SC.case(N, 90 + N, min(4, N), 1, outlier_frac=0.0)      # (its own sets are not used)
    lines, _, _ = _run(driver, c["prob"], "params %r %d %d %d %r %r\n" % (p, mi, mx, ms, eps, th2))
    w = lines[1].split()
    assert w[0] == "params" and (int(_field(w, "n")), int(_field(w, "min")), int(_field(w, "maxits")), int(_field(w, "set"))) == (N, want[0], want[1], ms)
    e = np.float32(eps)
    if e < np.float32(want[0]) / np.float32(N):
        e = np.float32(want[0]) / np.float32(N)
    assert np.float32(_field(w, "eps")) == e


def test_loop_count_draws_and_inlier_mapping(driver):
    c = SC.FAMILIES["x4_n100"]()
    n = 100
    script = "params 0.99 10 300 4 0.5 5.991\niterate 5\niterate 5\niterate 5\niterate 40\nfind\n"
    lines, index, total = _run(driver, c["prob"], script)
    mi, mx = Y.ransac_parameters(n, *SC.RELOCALIZATION)
    assert (mi, mx) == (50, 35)
    lcg = FR.Lcg(SEED)
    state = Y.new_state(n)
    calls = [ln.split() for ln in lines if ln.startswith("call ")]
    outs = [ln.split() for ln in lines if ln.startswith("iterate ") or ln.startswith("find ")]
    assert len(calls) == len(outs) == 5
    returned_some, repeated = False, False
    for call, out, asked in zip(calls, outs, (5, 5, 5, 40, mx)):
        n_hyp = max(asked, mx - state["iterations"])      # while(mnIterations<mRansacMaxIts || nCurrentIterations<nIterations): the ||
        assert (int(_field(call, "nhyp")), int(_field(call, "iterations")), int(_field(call, "best"))) == (n_hyp, state["iterations"], state["best_inliers"])
        assert (int(_field(call, "min")), int(_field(call, "max")), int(_field(call, "set"))) == (mi, mx, 4)
        sets = FR.draw_sets(lcg, n, 4, n_hyp)      # every draw of the chunk before the call, through the reference's loop with its quirk
        assert [int(v) for v in call[call.index("sets") + 1:]] == sets.reshape(-1).tolist()
        assert int(_field(out, "draws")) == 4 * n_hyp
        repeated = repeated or any(len(set(s)) < 4 for s in sets)
        rule = _stub(n, sets, state, mi, mx)
        state = rule["state"]
        assert int(_field(out, "nomore")) == (int(rule["no_more"]) if out[0] == "iterate" else 0)
        got = [int(v) for v in out[out.index("inliers") + 1:]]
        if rule["returned"] < 0:
            assert _field(out, "mat") == "empty" and int(_field(out, "size")) == 0 and int(_field(out, "ninl")) == 0 and got == []      # vbInliers cleared
        else:
            returned_some = True
            assert int(_field(out, "size")) == total and int(_field(out, "ninl")) == rule["n_inliers"]
            assert got == [index[i] for i in np.flatnonzero(rule["inlier"])]      # through mvKeyPointIndices
            assert np.array_equal(np.array(_field(out, "mat", 16), np.float32), rule["Tcw"].reshape(-1))
    assert returned_some
    assert state["iterations"] == 35 + 5 + 5 + 40 + 35 or returned_some


def test_draw_quirk_reaches_a_repeated_index(driver):
    c = SC.case(12, 77, 6, 1, outlier_frac=0.0)
    lines, _, _ = _run(driver, c["prob"], "params 0.99 6 300 6 0.5 5.991\niterate 60\n")
    call = [ln.split() for ln in lines if ln.startswith("call ")][0]
    sets = np.array(call[call.index("sets") + 1:], np.int32).reshape(-1, 6)
    assert np.array_equal(sets, FR.draw_sets(FR.Lcg(SEED), 12, 6, len(sets)))
    assert sets.min() >= 0 and sets.max() < 12 and any(len(set(s)) < 6 for s in sets)


def test_too_few_correspondences_draw_nothing(driver):
    c = SC.FAMILIES["n8_n9_below_min"]()
    lines, _, _ = _run(driver, c["prob"], "params 0.99 10 300 4 0.5 5.991\niterate 5\n")
    assert not any(ln.startswith("call ") for ln in lines)
    out = lines[-1].split()
    assert (int(_field(out, "draws")), int(_field(out, "nomore")), _field(out, "mat"), int(_field(out, "size"))) == (0, 1, "empty", 0)
