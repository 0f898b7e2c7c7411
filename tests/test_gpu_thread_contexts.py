"""Life cycle of the per-thread contexts (csrc/common.h: ThreadStream, DevBuf, PinBuf).  Every entry point that keeps a thread_local context creates its stream --
and whatever else it needs -- on the calling thread's first call and destroys it when the thread exits.  A worker thread makes one call of each and exits, the main
thread makes the same calls, a second worker makes them again: each call succeeds (a failure raises) and the three sets of results are equal byte for byte."""
import threading

import numpy as np
import pytest

from eao_fusion_amd import synth

import essential_graph_scenes as EG
import sim3_scenes as S3
import sim3_solver_scenes as SS
import triangulation_scenes as TS
from sim3_child import result_bytes as sim3_bytes
from sim3_solver_child import result_bytes as solver_bytes

pytestmark = pytest.mark.gpu


def test_contexts_of_exited_threads_are_released_and_rebuilt():
    import torch  # noqa: F401
    import eao_fusion_amd as E
    from eao_fusion_amd import frame as FR
    from eao_fusion_amd import search
    from eao_fusion_amd.optimizer import optimize_essential_graph, optimize_sim3
    from eao_fusion_amd.sim3_solver import sim3_solver_iterate
    assert E.load().eao_device_check() == 0
    sim3 = S3.scene(11, seed=301)                          # one above the `nCorr - nBad < 10` early return
    solver, triples = SS.friendly("n21-fs1")               # one chunk of hypotheses
    graph = EG.ring(n=3, seed=5)
    tri = TS.single_pair()                                 # one neighbour
    sc = synth.synth_search_scene(n=40, seed=8340)
    T = np.ascontiguousarray(sc["T2w"], np.float32)
    Ow = (-(T[:3, :3].astype(np.float64).T @ T[:3, 3].astype(np.float64))).astype(np.float32)
    fr = dict(Tcw=T, Ow=Ow, fx=sc["K"][0], fy=sc["K"][1], cx=sc["K"][2], cy=sc["K"][3], mbf=sc["bf"], min_x=sc["K2"]["min_x"], max_x=sc["K2"]["max_x"],
              min_y=sc["K2"]["min_y"], max_y=sc["K2"]["max_y"], log_scale_factor=sc["K2"]["log_scale_factor"])
    rng = np.random.default_rng(77)
    sets = [rng.integers(0, 256, size=(k, 32), dtype=np.uint8) for k in (1, 2, 5, 9, 0, 17)]
    cur, _, mps = synth.synth_tracking(n=48, seed=7140)

    def calls():
        eg = optimize_essential_graph(graph)
        tv, tx = search.product().triangulate_matches_batch(tri["K1"], tri["cam1"], tri["K2s"], tri["cams2"], tri["match12"], tri["ratio_factor"])
        fv = FR.product().is_in_frustum(fr, sc["points"], 0.5)
        nm, mm = E.ORBmatcher(0.8, True).SearchByProjectionPoints(cur, mps, 1.0)
        return [sim3_bytes(optimize_sim3(sim3)),
                solver_bytes(sim3_solver_iterate(solver, None, triples, inspect=True)),
                b"".join(np.ascontiguousarray(eg[k]).tobytes() for k in ("Scw", "Tiw", "Xw_corrected", "trials", "lambda", "chi2")) + np.int32(eg["lm_iterations"]).tobytes(),
                tv.tobytes() + tx.tobytes(),
                b"".join(np.ascontiguousarray(fv[k]).tobytes() for k in sorted(fv)),
                E.distinctive_descriptors(sets).tobytes(),
                np.int32(nm).tobytes() + mm.tobytes()]

    got = {}

    def worker(name):
        try:
            got[name] = calls()
        except Exception as ex:  # noqa: BLE001
            got[name] = ex

    for name in ("first worker", "main", "second worker"):      # one after the other: the first worker's contexts are gone when the second one starts
        if name == "main":
            got[name] = calls()
        else:
            t = threading.Thread(target=worker, args=(name,))
            t.start()
            t.join()
    for name, res in got.items():
        assert not isinstance(res, Exception), "%s: %r" % (name, res)
    labels = ("eao_optimize_sim3", "eao_sim3_solver_iterate", "eao_optimize_essential_graph", "eao_triangulate_matches_batch", "eao_frame_is_in_frustum",
              "eao_distinctive_descriptors", "SearchByProjection (candidate lists)")
    for k, label in enumerate(labels):
        assert len(got["main"][k]) > 0, label
        assert got["first worker"][k] == got["main"][k], "%s: the first worker's result differs from the main thread's" % label
        assert got["second worker"][k] == got["main"][k], "%s: the second worker's result differs from the main thread's" % label
