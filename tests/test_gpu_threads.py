"""Thread safety of the C-ABI as the header states it: every entry point keeps its device workspace per host thread (one
HIP stream + arena each), an ORB handle belongs to one thread.  Four threads hammer different entry points at once; every
result must equal the single-threaded one."""
import threading

import numpy as np
import pytest

from eao_fusion_amd import synth

pytestmark = pytest.mark.gpu


def test_concurrent_entry_points():
    import torch  # noqa: F401
    import eao_fusion_amd as E
    from eao_fusion_amd import search
    assert E.load().eao_device_check() == 0
    img = synth.synth_frame(1002)
    ba = synth.synth_ba(n_free=6, n_fixed=2, n_points=400, seed=3100)
    pose = synth.synth_pose(n=500, seed=4100, n_planes=3)
    cur, last, mps = synth.synth_tracking(n=600, seed=7100)
    a, b = synth.synth_descriptors(300, 2100)
    sc = synth.synth_search_scene(n=300, seed=8300)
    s1 = dict(descriptors=sc["K1"]["descriptors"], angle=sc["K1"]["kp_angle"], valid=(sc["mp1"] >= 0).astype(np.uint8), fv=sc["fv1"])
    s2 = dict(descriptors=sc["K2"]["descriptors"], angle=sc["K2"]["kp_angle"], valid=(sc["mp2"] >= 0).astype(np.uint8), fv=sc["fv2"])

    def job_orb():
        k, d = E.ORBextractor(1000, 1.2, 8, 20, 7)(img)
        return k.tobytes() + d.tobytes()

    def job_ba():
        r = E.Optimizer.LocalBundleAdjustment(ba)
        return r["poses"].tobytes() + r["points"].tobytes() + r["edge_outlier"].tobytes()

    def job_pose():
        r = E.Optimizer.PoseOptimization(pose)
        return r["Tcw"].tobytes() + r["outlier"].tobytes() + r["plane_outlier"].tobytes()

    def job_match():
        m = E.ORBmatcher(0.8, True)
        n1, m1 = m.SearchByProjectionPoints(cur, mps, 1.0)
        n2, m2 = m.SearchByProjectionFrames(cur, last, 7.0, False)
        n3, m3 = search.product().search_by_bow(1, s1, s2, 0.75, True)
        return m1.tobytes() + m2.tobytes() + m3.tobytes() + E.hamming_best2(a, b).tobytes()

    jobs = [job_orb, job_ba, job_pose, job_match]
    expect = [j() for j in jobs]
    errors = []

    def worker(i):
        try:
            for rep in range(6):
                j = (i + rep) % len(jobs)
                if jobs[j]() != expect[j]:
                    errors.append("thread %d: job %s differs on repetition %d" % (i, jobs[j].__name__, rep))
        except Exception as ex:  # noqa: BLE001
            errors.append("thread %d: %r" % (i, ex))

    ths = [threading.Thread(target=worker, args=(i,)) for i in range(4)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    assert not errors, errors


def test_concurrent_sim3_threads_beside_pose_optimization():
    """eao_optimize_sim3 keeps its stream, events and device / host staging buffers per host thread (thread_local in csrc/sim3.hip).  Four threads
    each run their own slice of sim3_scenes.IRREGULAR twenty times -- sizes from 9 to 20000, so every thread's buffers grow and are reused --
    while a fifth runs PoseOptimization; every result equals the serial one bit for bit.  One process holds the GPU throughout."""
    import torch  # noqa: F401
    import eao_fusion_amd as E
    from eao_fusion_amd.optimizer import optimize_sim3
    import sim3_scenes as SC
    from sim3_child import result_bytes
    assert E.load().eao_device_check() == 0
    probs = [SC.irregular_scene(kw, edit) for _, kw, edit in SC.IRREGULAR]
    slices = [list(range(i, len(probs), 4)) for i in range(4)]
    pose = synth.synth_pose(n=500, seed=4100, n_planes=3)

    def job_pose():
        r = E.Optimizer.PoseOptimization(pose)
        return r["Tcw"].tobytes() + r["outlier"].tobytes() + r["plane_outlier"].tobytes()

    expect = [result_bytes(optimize_sim3(p)) for p in probs]
    expect_pose = job_pose()
    errors, running = [], [4]
    lock = threading.Lock()

    def sim3_worker(i):
        try:
            for rep in range(20):
                order = slices[i] if rep % 2 == 0 else slices[i][::-1]
                for k in order:
                    if result_bytes(optimize_sim3(probs[k])) != expect[k]:
                        errors.append("thread %d: IRREGULAR[%d] differs on repetition %d" % (i, k, rep))
        except Exception as ex:  # noqa: BLE001
            errors.append("thread %d: %r" % (i, ex))
        finally:
            with lock:
                running[0] -= 1

    pose_calls = [0]

    def pose_worker():
        try:
            while running[0] > 0 or pose_calls[0] < 20:
                if job_pose() != expect_pose:
                    errors.append("PoseOptimization differs on call %d" % pose_calls[0])
                pose_calls[0] += 1
        except Exception as ex:  # noqa: BLE001
            errors.append("pose thread: %r" % (ex,))

    ths = [threading.Thread(target=sim3_worker, args=(i,)) for i in range(4)] + [threading.Thread(target=pose_worker)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    assert not errors, errors[:10]
    assert pose_calls[0] >= 20


def test_concurrent_map_scale_batch_and_handle_calls(monkeypatch):
    """Round 5's host-side machinery under concurrency: two threads run map-scale BundleAdjustment (their covisibility set-up is split over the ONE process-wide host
    crew, forced onto these test-size maps), one runs eao_local_ba_batch (which owns the same crew for its set-up workers and group leaders), one runs the keyframe-handle
    searches.  Every result must equal the single-threaded one bit for bit, whatever the interleaving."""
    import torch  # noqa: F401
    import eao_fusion_amd as E
    from eao_fusion_amd import search
    assert E.load().eao_device_check() == 0
    monkeypatch.setenv("EAO_BA_SETUP_THREADS", "6")
    mapA = synth.synth_ba(n_free=90, n_fixed=1, n_points=3600, seed=5620, band=5)
    mapB = synth.synth_ba(n_free=64, n_fixed=2, n_points=2400, seed=5621)
    wins = [synth.synth_ba(seed=6300 + w) for w in range(9)] + [synth.synth_ba(n_free=40, n_fixed=1, n_points=1500, seed=6310)]
    sc = synth.synth_search_scene(n=500, seed=8310)

    def ba_bytes(r):
        return r["poses"].tobytes() + r["points"].tobytes() + bytes(list(r["iters"]))

    def job_map_a():
        return ba_bytes(E.Optimizer.BundleAdjustment(mapA, 6, bRobust=False))

    def job_map_b():
        return ba_bytes(E.Optimizer.BundleAdjustment(mapB, 6, bRobust=True))

    def job_batch():
        return b"".join(ba_bytes(r) + r["edge_outlier"].tobytes() for r in E.Optimizer.LocalBundleAdjustmentBatch(wins))

    def job_handles():
        g = search.product_handles()
        s1 = dict(descriptors=sc["K1"]["descriptors"], angle=sc["K1"]["kp_angle"], valid=(sc["mp1"] >= 0).astype(np.uint8), fv=sc["fv1"])
        s2 = dict(descriptors=sc["K2"]["descriptors"], angle=sc["K2"]["kp_angle"], valid=(sc["mp2"] >= 0).astype(np.uint8), fv=sc["fv2"])
        n, m = g.search_by_bow(1, s1, s2, 0.75, True)
        return m.tobytes() + bytes([n & 255])

    jobs = [job_map_a, job_map_b, job_batch, job_handles]
    expect = [j() for j in jobs]
    errors = []

    def worker(i):
        try:
            for rep in range(5):
                j = (i + rep) % len(jobs)
                if jobs[j]() != expect[j]:
                    errors.append("thread %d: job %s differs on repetition %d" % (i, jobs[j].__name__, rep))
        except Exception as ex:  # noqa: BLE001
            errors.append("thread %d: %r" % (i, ex))

    ths = [threading.Thread(target=worker, args=(i,)) for i in range(4)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    assert not errors, errors


def test_shared_keyframe_handles_across_threads(oracle):
    """include/eao_fusion.h: "A handle is immutable but for its occupancy; searches only read it, so any number of threads may search the same handle (each thread has
    its own stream and scratch)" -- LocalMapping creates the keyframes' handles, LoopClosing and Tracking search them.  Handles created on the MAIN thread, searched by
    four other threads at once (vocabulary-node search, triangulation over 12 neighbours, fusion into 10 targets): every result equals the oracle's."""
    import torch  # noqa: F401
    from eao_fusion_amd import search
    g, o = search.product_handles(), oracle.search_binding()
    sc = synth.synth_search_scene(n=900, seed=8120, n_nodes=40)
    k1, k2 = dict(sc["K1"]), dict(sc["K2"])
    k1["occupied"] = ((sc["mp1"] >= 0) & (np.arange(len(sc["mp1"])) % 3 == 0)).astype(np.uint8)
    k2["occupied"] = ((sc["mp2"] >= 0) & (np.arange(len(sc["mp2"])) % 4 == 1)).astype(np.uint8)
    h1, h2 = g.handle(k1, sc["fv1"]), g.handle(k2, sc["fv2"])
    h1.update_points(k1["occupied"]); h2.update_points(k2["occupied"])
    s1 = dict(descriptors=k1["descriptors"], angle=k1["kp_angle"], valid=(sc["mp1"] >= 0).astype(np.uint8), fv=sc["fv1"])
    s2 = dict(descriptors=k2["descriptors"], angle=k2["kp_angle"], valid=(sc["mp2"] >= 0).astype(np.uint8), fv=sc["fv2"])
    want_bow = o.search_by_bow(1, s1, s2, 0.75, True)
    want_tri = o.search_for_triangulation(k1, sc["fv1"], k2, sc["fv2"], sc["F12"], sc["ex"], sc["ey"], 0, True)
    T = sc["T2w"].astype(np.float64)
    pose = np.concatenate([T[:3, :3].ravel(), T[:3, 3], -T[:3, :3].T @ T[:3, 3]]).astype(np.float32)
    want_fuse = o.fuse_search(k2, 0, pose, sc["K"], sc["bf"], sc["points"], 3.0)
    assert want_bow[0] > 10 and want_tri[0] > 10 and want_fuse[0] > 10
    errors = []

    def worker(i):
        try:
            for rep in range(8):
                which = (i + rep) % 3
                if which == 0:
                    got = g.search_by_bow_h(1, h1, s1["valid"], h2, s2["valid"], 0.75, True)
                    ok = got[0] == want_bow[0] and np.array_equal(got[1], want_bow[1])
                elif which == 1:
                    nm, m = g.search_for_triangulation_h(h1, [h2] * 12, [sc["F12"]] * 12, [sc["ex"]] * 12, [sc["ey"]] * 12, 0, True)
                    ok = all(nm[k] == want_tri[0] and np.array_equal(m[k], want_tri[1]) for k in range(12))
                else:
                    nf, best = g.fuse_search_h([h2] * 10, 0, [pose] * 10, sc["K"], sc["bf"], sc["points"], 3.0)
                    ok = all(nf[k] == want_fuse[0] and np.array_equal(best[k], want_fuse[1]) for k in range(10))
                if not ok:
                    errors.append("thread %d: search %d differs on repetition %d" % (i, which, rep))
        except Exception as ex:  # noqa: BLE001
            errors.append("thread %d: %r" % (i, ex))

    ths = [threading.Thread(target=worker, args=(i,)) for i in range(4)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    assert not errors, errors


def test_three_threads_of_bundle_adjustment_return_identical_results():
    """Round 6 (tests/cpp/mixed_load.cpp found it: `results_identical` false in 3 of 16 scenarios): LocalBundleAdjustment beside ANOTHER thread's bundle adjustment returned, about
    once in 10 000 calls, one of a handful of wrong-but-repeatable results -- the last workgroup of k_ba_backsub summed a stale partial chi2 (published with an agent-scope
    atomic STORE that the ticket overtook on a busy fabric) and an LM decision flipped; never alone, never beside the extractor.  The partial sums are now published with
    returning atomic exchanges (csrc/lba.hip).  This test runs the reference's mix for a few seconds -- LocalMapping's LBA loop, a second LBA loop on another window, LoopClosing's
    map-scale BundleAdjustment -- and demands bit-identical results throughout; the long form is tools/dbg_lba_beside_gba.py (minutes, 10^5 calls)."""
    import time
    import torch  # noqa: F401
    import eao_fusion_amd as E
    assert E.load().eao_device_check() == 0
    pa, pb = synth.synth_ba(), synth.synth_ba(seed=6007)
    g = synth.synth_ba(n_free=200, n_fixed=1, n_points=8000, seed=5405, band=9)
    jobs = {"lba_a": lambda: E.Optimizer.LocalBundleAdjustment(pa), "lba_b": lambda: E.Optimizer.LocalBundleAdjustment(pb),
            "map_ba": lambda: E.Optimizer.BundleAdjustment(g, 10, bRobust=False)}
    key = lambda r: r["poses"].tobytes() + r["points"].tobytes() + r["edge_outlier"].tobytes()      # noqa: E731
    want = {k: key(j()) for k, j in jobs.items()}
    errors, counts = [], {k: 0 for k in jobs}
    t_end = time.perf_counter() + 6.0

    def worker(k):
        try:
            while time.perf_counter() < t_end:
                if key(jobs[k]()) != want[k]:
                    errors.append("%s: call %d differs" % (k, counts[k]))
                counts[k] += 1
        except Exception as ex:  # noqa: BLE001
            errors.append("%s: %r" % (k, ex))

    ths = [threading.Thread(target=worker, args=(k,)) for k in jobs]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    assert not errors, errors
    assert counts["lba_a"] > 500 and counts["map_ba"] > 50, counts
