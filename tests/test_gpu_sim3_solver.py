"""Sim3Solver on the device (eao_sim3_solver_iterate / _batch, csrc/sim3_solver.hip) against the numpy restatement tests/sim3_solver_reference.py
on the families of tests/sim3_solver_scenes.py, the golden fixtures tests/golden/sim3_solver/*.npz, the batched entry point against single calls,
determinism, and the class surface include/eaofusion/Sim3Solver.h against stand-ins.  Every bound comes from tests/sim3_solver_tolerances.py.

The yardstick's arithmetic choices (OpenCV's own arithmetic is not in the reference tree): see the docstring of tests/sim3_solver_reference.py."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

import sim3_solver_reference as R
import sim3_solver_scenes as SC
from sim3_solver_child import result_bytes
from sim3_solver_tolerances import GAP_MIN, MARGIN_REL, T12_REL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILY_NAMES = [name for name, _ in SC.all_families()]
EVALUATED = [name for name in FAMILY_NAMES if name != "n0"]       # every family that has a correspondence to sample
_cache = {}


def _case(name):
    """(problem, triples, prepared problem, yardstick with every hypothesis evaluated, device with every hypothesis evaluated), computed once and left unchanged"""
    if name not in _cache:
        from eao_fusion_amd.sim3_solver import sim3_solver_iterate
        prob, triples = dict(SC.all_families())[name]()
        pre = R.prepare(prob)
        n, nh = pre["n"], len(triples)
        # min_inliers = n: no count exceeds it, so nothing returns and all hypotheses are evaluated
        ref = R.iterate(prob, None, triples, min_inliers=n, max_its=nh, pre=pre)
        dev = sim3_solver_iterate(prob, None, triples, min_inliers=n, max_its=nh, inspect=True)
        _cache[name] = (prob, triples, pre, ref, dev)
    return _cache[name]


def _conditioned(ref):
    ev = ref["hyp_eigenvalues"]
    with np.errstate(all="ignore"):
        return (ev[:, 0] - ev[:, 1]) / (np.abs(ev[:, 0]) + np.abs(ev[:, 3])) >= GAP_MIN


def _spread(a, b):
    """|dT| / max |T| of one transform; the NaN patterns must agree"""
    assert np.array_equal(np.isnan(a), np.isnan(b)), (a, b)
    if np.isnan(a).all():
        return 0.0
    with np.errstate(all="ignore"):
        d = float(np.nanmax(np.abs(a.astype(np.float64) - b.astype(np.float64))))
        return d / float(np.nanmax(np.abs(b.astype(np.float64)))) if d > 0 else 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("name", EVALUATED)
def test_horn_transforms(name):
    """ComputeSim3: on conditioned hypotheses T12 and T21 within T12_REL of the yardstick; ill-conditioned ones finite or NaN."""
    prob, triples, pre, ref, dev = _case(name)
    cond = _conditioned(ref)
    worst = 0.0
    for h in range(len(triples)):
        for key in ("hyp_T12", "hyp_T21"):
            got = dev[key][h]
            assert (np.isfinite(got) | np.isnan(got)).all() and np.array_equal(got[3], np.array([0, 0, 0, 1], np.float32)), (h, got)
            if cond[h]:
                worst = max(worst, _spread(got, ref[key][h]))
    print("\n[sim3 solver horn] %s: %d of %d conditioned, largest |dT| / max |T| %.3e (bound %.3e)" % (name, int(cond.sum()), len(triples), worst, T12_REL))
    assert worst <= T12_REL


@pytest.mark.gpu
@pytest.mark.parametrize("name", EVALUATED)
def test_check_inliers_on_the_devices_own_transform(name):
    """CheckInliers restated on the device's own T12 / T21 gives the device's flags bit for bit, for every hypothesis; the count is their sum."""
    prob, triples, pre, ref, dev = _case(name)
    assert dev["hyp_inlier"].shape == (len(triples), pre["n"])
    for h in range(len(triples)):
        want = R.check_inliers(pre, dev["hyp_T12"][h], dev["hyp_T21"][h])
        assert np.array_equal(want, dev["hyp_inlier"][h]), (name, h, np.nonzero(want != dev["hyp_inlier"][h])[0])
        assert int(dev["hyp_inliers"][h]) == int(want.sum())


@pytest.mark.gpu
@pytest.mark.parametrize("name", EVALUATED)
def test_flags_against_the_yardsticks_transform(name):
    """On conditioned hypotheses the flags equal the yardstick's outside MARGIN_REL of the gates; the counts differ by at most the pairs left out."""
    prob, triples, pre, ref, dev = _case(name)
    cond = _conditioned(ref)
    for h in np.nonzero(cond)[0]:
        e1, e2 = R.errors(pre, ref["hyp_T12"][h], ref["hyp_T21"][h])
        with np.errstate(all="ignore"):
            near = (np.abs(e1.astype(np.float64) / pre["max1"] - 1) < MARGIN_REL) | (np.abs(e2.astype(np.float64) / pre["max2"] - 1) < MARGIN_REL)
        assert np.array_equal(dev["hyp_inlier"][h][~near], ref["hyp_inlier"][h][~near]), (name, h)
        assert abs(int(dev["hyp_inliers"][h]) - int(ref["hyp_inliers"][h])) <= int(near.sum())


def _replay(dev_all, order, state, min_inliers, max_its, n):
    """The sequential rule in Python over the device's own counts: what a call over the hypotheses `order` must return."""
    state = dict(state or R.new_state())
    counts = dev_all["hyp_inliers"][order]
    ret, bk, it, best, no_more = R.sequential_rule(counts, state["iterations"], state["best_inliers"], min_inliers, max_its, n)
    want = dict(returned=ret, n_inliers=best if ret >= 0 else 0, no_more=no_more, iterations=it, best_inliers=best,
                best_T12=dev_all["hyp_T12"][order[bk]] if bk >= 0 else np.asarray(state["best_T12"], np.float32), bk=bk)
    want["T12"] = dev_all["hyp_T12"][order[ret]] if ret >= 0 else np.zeros((4, 4), np.float32)
    want["inlier"] = dev_all["hyp_inlier"][order[ret]] if ret >= 0 else None
    return want


def _assert_replay(got, want, n):
    s = got["state"]
    assert (got["returned"], got["n_inliers"], got["no_more"], s["iterations"], s["best_inliers"]) == \
        (want["returned"], want["n_inliers"], want["no_more"], want["iterations"], want["best_inliers"])
    assert np.array_equal(got["T12"], want["T12"], equal_nan=True)
    assert np.array_equal(s["best_T12"], want["best_T12"], equal_nan=True)
    if want["bk"] >= 0:
        # mBestRotation / mBestTranslation / mBestScale are the parts mBestT12 was assembled from (:316-326)
        assert np.array_equal(s["best_t"], s["best_T12"][:3, 3], equal_nan=True)
        assert np.array_equal((np.float64(s["best_s"]) * s["best_R"].astype(np.float64)).astype(np.float32), s["best_T12"][:3, :3], equal_nan=True)
    if want["inlier"] is not None:
        assert np.array_equal(got["inlier"], want["inlier"]) and int(got["inlier"].sum()) == got["n_inliers"]
    else:
        assert not got["inlier"].any()       # written only on a return


@pytest.mark.gpu
def test_sequential_rule():
    """returned, n_inliers, iterations, best_*, no_more and inlier equal the rule replayed on the device's own counts, over chunks chosen from those
    counts so that every branch of :183-206 occurs."""
    from eao_fusion_amd.sim3_solver import sim3_solver_iterate
    prob, triples, pre, ref, dev = _case("n64-fs1")
    n, c, mi = pre["n"], dev["hyp_inliers"], SC.MIN_INLIERS
    good = sorted((h for h in range(len(c)) if c[h] > mi), key=lambda h: c[h])
    weak = sorted((h for h in range(len(c)) if 0 < c[h] < mi), key=lambda h: c[h])
    zero = [h for h in range(len(c)) if c[h] == 0]
    assert len(good) >= 2 and c[good[0]] < c[good[-1]] and len(weak) >= 2 and len(zero) >= 2, c

    def run(order, state=None, min_inliers=mi, max_its=300):
        order = np.asarray(order)
        got = sim3_solver_iterate(prob, state, triples[order], min_inliers=min_inliers, max_its=max_its, inspect=True)
        want = _replay(dev, order, state, min_inliers, max_its, n)
        _assert_replay(got, want, n)
        return got, want

    # a return at the chunk's first position; better hypotheses after it are ignored
    got, want = run([good[0], good[-1], good[-1]])
    assert got["returned"] == 0 and got["state"]["iterations"] == 1 and got["n_inliers"] == c[good[0]] < c[good[-1]]
    # ... and at a middle position
    got, want = run([weak[0], zero[0], good[0], good[-1], weak[1]])
    assert got["returned"] == 2 and got["state"]["iterations"] == 3 and got["state"]["best_inliers"] == c[good[0]]
    # a tie goes to the later hypothesis (0 >= 0 twice: two different transforms, the second one is kept)
    got, want = run([zero[0], zero[1]])
    assert got["returned"] == -1 and want["bk"] == 1 and not np.array_equal(dev["hyp_T12"][zero[0]], dev["hyp_T12"][zero[1]], equal_nan=True)
    assert np.array_equal(got["state"]["best_T12"], dev["hyp_T12"][zero[1]], equal_nan=True)
    # a count equal to min_inliers becomes the best without returning (the comparison is strict)
    got, want = run([weak[0], good[0]], min_inliers=int(c[good[0]]))
    assert got["returned"] == -1 and got["state"]["best_inliers"] == c[good[0]] and got["state"]["iterations"] == 2 and not got["no_more"]
    # the state carries over: a weaker hypothesis does not replace the best, an equal one does
    got2, _ = run([weak[1], good[0]], state=got["state"], min_inliers=int(c[good[0]]))
    assert got2["state"]["iterations"] == 4 and got2["state"]["best_inliers"] == c[good[0]]
    # a chunk cut by max_its: two of five evaluated, bNoMore
    st = dict(R.new_state(), iterations=298)
    got, want = run([weak[0], weak[1], good[0], good[1], zero[0]], state=st)
    assert got["returned"] == -1 and got["no_more"] and got["state"]["iterations"] == 300 and list(got["hyp_inliers"][2:]) == [0, 0, 0]
    assert not got["hyp_T12"][2:].any() and not got["hyp_inlier"][2:].any()
    # ... and one already at the limit: nothing evaluated
    got, want = run([good[0]], state=dict(R.new_state(), iterations=300))
    assert got["no_more"] and got["state"]["iterations"] == 300 and got["hyp_inliers"][0] == 0
    # n < min_inliers: bNoMore, the state untouched, the triples not read
    p19, t19, pre19, _, _ = _case("n19")
    st = dict(R.new_state(), iterations=7, best_inliers=3, best_s=np.float32(1.5))
    got = sim3_solver_iterate(p19, st, np.full((5, 3), 1000, np.int32), min_inliers=mi, max_its=300, inspect=True)
    assert got["no_more"] and got["returned"] == -1 and got["state"]["iterations"] == 7 and got["state"]["best_inliers"] == 3
    assert got["state"]["best_s"] == np.float32(1.5) and not got["hyp_inliers"].any()
    p0, t0 = SC.irregular("n0")
    got = sim3_solver_iterate(p0, None, t0, min_inliers=mi, max_its=300, inspect=True)
    assert got["no_more"] and got["returned"] == -1 and got["state"]["iterations"] == 0 and got["inlier"].shape == (0,)


@pytest.mark.gpu
def test_invalid_arguments_fail_before_anything_is_written():
    from eao_fusion_amd import EaoError
    from eao_fusion_amd.sim3_solver import sim3_solver_iterate
    prob, triples = SC.friendly("n64-fs1")
    bad = triples.copy()
    bad[3, 1] = 64
    with pytest.raises(EaoError):
        sim3_solver_iterate(prob, None, bad)
    bad[3, 1] = -1
    with pytest.raises(EaoError):
        sim3_solver_iterate(prob, None, bad)
    neg = dict(prob, sigma2_1=-prob["sigma2_1"])
    with pytest.raises(EaoError):
        sim3_solver_iterate(neg, None, triples)


@pytest.mark.gpu
def test_chunking_sixty_calls_of_five():
    """Sixty iterate(5) calls over a 300-hypothesis stream, the solver restarted after each return as LoopClosing moves on after one, leave the same
    state and the same returns as the rule replayed in Python over the device's counts of the same stream."""
    from eao_fusion_amd.sim3_solver import sim3_solver_iterate
    prob, _ = SC.friendly("n65-fs0")
    n = len(prob["Xw1"])
    stream = SC.drawn_triples(n, 300, 99)
    whole = sim3_solver_iterate(prob, None, stream, min_inliers=n, max_its=300, inspect=True)
    counts = whole["hyp_inliers"]
    mi = int(np.sort(counts)[-12])           # a dozen hypotheses of the stream reach it: some calls return, most do not
    state, want_state, returns, want_returns = None, None, [], []
    for k in range(60):
        order = np.arange(5 * k, 5 * k + 5)
        got = sim3_solver_iterate(prob, state, stream[order], min_inliers=mi, max_its=300)
        want = _replay(whole, order, want_state, mi, 300, n)
        returns.append(got["returned"]); want_returns.append(want["returned"])
        assert np.array_equal(got["state"]["best_T12"], want["best_T12"], equal_nan=True)
        assert (got["state"]["iterations"], got["state"]["best_inliers"]) == (want["iterations"], want["best_inliers"])
        if got["returned"] >= 0:
            assert np.array_equal(got["inlier"], whole["hyp_inlier"][order[got["returned"]]])
            state = want_state = None
        else:
            state = got["state"]
            want_state = dict(iterations=want["iterations"], best_inliers=want["best_inliers"], best_T12=want["best_T12"])
    assert returns == want_returns and 1 <= sum(r >= 0 for r in returns) < 60


def _batch_inputs():
    names = [name for name, _ in SC.FRIENDLY] + ["n0", "n19"]
    assert len(names) == 16
    probs, tris, states = [], [], []
    for k, name in enumerate(names):
        prob, triples = dict(SC.all_families())[name]()
        probs.append(prob)
        tris.append(triples[:1 + (5 * k) % 24])
        states.append(None if k % 3 else dict(R.new_state(), iterations=290 + k, best_inliers=k))
    return probs, tris, states


@pytest.mark.gpu
def test_batch_bit_identical_to_single_calls():
    """16 problems with different n (0, 19, 2000 among them), n_hyp and states in one call: every output equal to the single call's, bit for bit."""
    from eao_fusion_amd.sim3_solver import sim3_solver_iterate, sim3_solver_iterate_batch
    probs, tris, states = _batch_inputs()
    ns = [len(p["Xw1"]) for p in probs]
    assert 0 in ns and 19 in ns and 2000 in ns and len({len(t) for t in tris}) > 8
    batch = sim3_solver_iterate_batch(probs, states, tris, inspect=True)
    for p, t, s, b in zip(probs, tris, states, batch):
        assert result_bytes(sim3_solver_iterate(p, s, t, inspect=True)) == result_bytes(b)
    assert any(b["returned"] >= 0 for b in batch) and any(b["no_more"] for b in batch)
    plain = sim3_solver_iterate_batch(probs, states, tris)
    for b, q in zip(batch, plain):
        assert result_bytes({k: v for k, v in b.items() if not k.startswith("hyp_")}) == result_bytes(q)


@pytest.mark.gpu
def test_large_batch_bit_identical_to_single_calls():
    """16 x 300 hypotheses in one launch -- more workgroups than the device has CUs -- against single calls."""
    from eao_fusion_amd.sim3_solver import sim3_solver_iterate, sim3_solver_iterate_batch
    probs = [p for p, _, _ in zip(*_batch_inputs())]
    tris = [SC.drawn_triples(len(p["Xw1"]), 300, 200 + k) if len(p["Xw1"]) else np.zeros((300, 3), np.int32) for k, p in enumerate(probs)]
    assert 16 * 300 > 2 * 256      # an MI355X has 256 CUs
    mi = [len(p["Xw1"]) if k % 2 else SC.MIN_INLIERS for k, p in enumerate(probs)]      # every other solver never returns: all 300 counted
    batch = sim3_solver_iterate_batch(probs, [None] * 16, tris, min_inliers=mi, inspect=True)
    for k, (p, t, b) in enumerate(zip(probs, tris, batch)):
        assert result_bytes(sim3_solver_iterate(p, None, t, min_inliers=mi[k], inspect=True)) == result_bytes(b), k
    assert any(b["state"]["iterations"] == 300 and b["no_more"] for b in batch)


@pytest.mark.gpu
def test_determinism():
    """Two calls give the same bytes; so does the same call after other entry points ran on the thread, and a process that has run nothing else."""
    from eao_fusion_amd.optimizer import optimize_sim3
    from eao_fusion_amd.sim3_solver import sim3_solver_iterate
    import sim3_scenes
    names = ["n257-fs0", "depth_edge", "pure_translation"]

    def run(name):
        prob, triples = dict(SC.all_families())[name]()
        return result_bytes(sim3_solver_iterate(prob, None, triples, inspect=True))

    first = [run(nm) for nm in names]
    assert first == [run(nm) for nm in names]
    optimize_sim3(sim3_scenes.scene(n=120, seed=71, fix_scale=True, outlier_frac=0.2))
    big, big_t = SC.friendly("n2000-fs1")
    sim3_solver_iterate(big, None, big_t, inspect=True)
    again = [run(nm) for nm in reversed(names)][::-1]
    assert first == again
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] + [v for v in [os.environ.get("PYTHONPATH")] if v]))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "sim3_solver_child.py"), names[0]], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert bytes.fromhex(out.stdout.strip().split("\n")[-1]) == first[0]


def _golden_files():
    return sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "sim3_solver", "sim3_solver_*.npz")))


def golden_problem(z):
    return dict(T1w=z["T1w"], T2w=z["T2w"], Xw1=z["Xw1"], Xw2=z["Xw2"], sigma2_1=z["sigma2_1"], sigma2_2=z["sigma2_2"], K1=z["K1"], K2=z["K2"],
                fix_scale=bool(z["fix_scale"]))


@pytest.mark.gpu
def test_golden():
    """The recorded yardstick results (tools/gen_golden_sim3_solver.py): flags and counts equal, transforms within T12_REL.  The fixtures hold
    conditioned hypotheses without a pair inside MARGIN_REL of its gate (the generator selects them), so nothing is left out here."""
    from eao_fusion_amd.sim3_solver import sim3_solver_iterate
    files = _golden_files()
    assert files, "tests/golden/sim3_solver/sim3_solver_*.npz missing (tools/gen_golden_sim3_solver.py)"
    for fn in files:
        z = np.load(fn)
        got = sim3_solver_iterate(golden_problem(z), None, z["triples"], min_inliers=int(z["min_inliers"]), max_its=int(z["max_its"]), inspect=True)
        assert np.array_equal(got["hyp_inliers"], z["hyp_inliers"]) and np.array_equal(got["hyp_inlier"], z["hyp_inlier"]), fn
        assert (got["returned"], got["n_inliers"], got["no_more"], got["state"]["iterations"]) == (int(z["returned"]), int(z["n_inliers"]), bool(z["no_more"]), int(z["iterations"])), fn
        assert np.array_equal(got["inlier"], z["inlier"]), fn
        for h in range(len(z["triples"])):
            assert _spread(got["hyp_T12"][h], z["hyp_T12"][h]) <= T12_REL and _spread(got["hyp_T21"][h], z["hyp_T21"][h]) <= T12_REL, (fn, h)
        assert _spread(got["T12"], z["T12"]) <= T12_REL, fn


@pytest.fixture(scope="module")
def class_driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sim3_solver") / "sim3_solver_driver")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-DEAOFUSION_FORCE_CV_COMPAT", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "sim3_solver", "sim3_solver_driver.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "eao_fusion_amd"), "-leaofusion_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "eao_fusion_amd"), "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    return exe


@pytest.mark.gpu
def test_class_surface_closes_a_loop(class_driver):
    """ComputeSim3's loop (src/LoopClosing.cc:286-342) over three candidates with a seeded stand-in generator: one has too few correspondences, one is
    all outliers and runs out of its 7 iterations in the second round, one closes in the fifth -- its Sim3 goes on to eaofusion::OptimizeSim3 and both stages
    end with >= 20 inliers.  The round, the iteration and the number of draws are what the yardstick gives over the same draw stream."""
    import sim3_solver_keyframes as KF
    txt = KF.loop_scene()
    out = subprocess.run([class_driver, "loop"], input=txt, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = dict(l.split(" ", 1) for l in out.stdout.strip().split("\n"))
    assert lines["candidate0"] == "discarded iterations 0" and lines["candidate1"] == "discarded iterations 7" and lines["candidate2"].startswith("match")
    f = lines["candidate2"].split()
    ransac, optimized, iterations = int(f[f.index("ransac") + 1]), int(f[f.index("optimized") + 1]), int(f[f.index("iterations") + 1])
    assert ransac > 20 and optimized >= 20 and iterations == 24
    assert lines["matched"] == "1 draws 96"
