#!/usr/bin/env python3
"""Times the triangulation half of CreateNewMapPoints beside the search it follows, on an MI355X, and writes profiles/triangulation_timing.txt.

Ten neighbours of 1000 keypoints over resident keyframes (the search scene of eao_fusion_amd.synth, neighbour variants as tests/test_gpu_search.py makes them, poses
and depths added).  Median of 50 calls after 10 warm-up calls of
  * eao_kf_search_for_triangulation alone  -- the parent commit's path: the match tables come back and the loop of src/LocalMapping.cc:288-454 runs on the host;
  * eao_kf_create_new_map_points           -- search and triangulation on one stream, one wait;
and the device time of the triangulation launches from HIP events on that stream (EAO_TRI_EVENTS=1).  The added cost is the difference of the two call times.
A record, not a gate; no comparison with the reference's host loop is made or implied (it needs OpenCV and is not built here).

    python tools/bench_triangulation.py
"""
import ctypes
import os
import sys
import time

os.environ["EAO_TRI_EVENTS"] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

N_NB, N_KP, WARMUP, CALLS = 10, 1000, 10, 50


def main():
    import torch  # noqa: F401
    from eao_fusion_amd import _lib, search, synth
    import test_gpu_search as TS
    import test_gpu_triangulation as TT
    import triangulation_reference as Y
    h = search.product_handles()
    scene = synth.synth_search_scene(n=N_KP, seed=8000)
    bf = scene["bf"]
    k1 = TT._with_depth(scene["K1"], bf)
    k1["occupied"] = ((scene["mp1"] >= 0) & (np.arange(len(scene["mp1"])) % 2 == 0)).astype(np.uint8)
    nb = TS._neighbours(scene, N_NB)
    k2s = [TT._with_depth(x[0], bf) for x in nb]
    cam1 = TT._cam_of(scene["T1w"], scene["K"], bf)
    cams2 = [TT._cam_of(scene["T2w"], scene["K"], bf, dz=0.01 * k) for k in range(N_NB)]
    rf = Y.ratio_factor(scene["K1"]["scale_factors"][1])
    h1 = search.KeyFrameHandle(h.lib, h.check, k1, scene["fv1"])
    h1.set_depth(k1["depth"], k1["raw_x"], k1["raw_y"])
    h2s = []
    for k2, x in zip(k2s, nb):
        hh = search.KeyFrameHandle(h.lib, h.check, k2, x[1])
        hh.set_depth(k2["depth"], k2["raw_x"], k2["raw_y"])
        h2s.append(hh)
    F, ex, ey = [x[2] for x in nb], [x[3] for x in nb], [x[4] for x in nb]

    def timed(fn, events=False):
        """median call time; with `events`, also the median of the device times the library measured (None where it measured none: the library was loaded before
        EAO_TRI_EVENTS was set, or an event call failed)"""
        for _ in range(WARMUP):
            fn()
        ts, dev = [], []
        for _ in range(CALLS):
            t0 = time.perf_counter()
            r = fn()
            ts.append((time.perf_counter() - t0) * 1e3)
            ms = ctypes.c_float(0)
            if events and _lib.load().eao_kf_last_triangulation_ms(ctypes.byref(ms)) == 0:
                dev.append(ms.value)
        return float(np.median(ts)), (float(np.median(dev)) if dev else None), r
    t_search, _d, (nm, _m) = timed(lambda: h.search_for_triangulation_h(h1, h2s, F, ex, ey, 0, True))
    t_both, t_dev, (nm2, _m2, verdict, _x) = timed(lambda: h.create_new_map_points_h(h1, cam1, h2s, cams2, F, ex, ey, 0, rf, True), events=True)
    lines = ["# tools/bench_triangulation.py: %d neighbours of %d keypoints over resident keyframes, median of %d calls after %d warm-up calls (Python caller, ms)" % (N_NB, N_KP, CALLS, WARMUP),
             "matched pairs %d, accepted %d" % (int(nm.sum()), int(np.isin(verdict, Y.ACCEPTING).sum())),
             "eao_kf_search_for_triangulation      %.4f ms per call" % t_search,
             "eao_kf_create_new_map_points         %.4f ms per call" % t_both,
             "added by the triangulation           %.4f ms per call" % (t_both - t_search),
             "triangulation launches, device time  %s (HIP events on the call's stream)" % ("%.4f ms" % t_dev if t_dev is not None else "not measured")]
    txt = "\n".join(lines) + "\n"
    with open(os.path.join(ROOT, "profiles", "triangulation_timing.txt"), "w") as f:
        f.write(txt)
    sys.stdout.write(txt)


if __name__ == "__main__":
    main()
