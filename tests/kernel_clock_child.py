"""The three kernel clocks that an environment variable arms (read once per process): one small call of the module and its reader, shared by
tests/test_gpu_kernel_clock.py (the unarmed half, in the test's process) and this program (the armed half, in a process of its own):

    EAO_PNP_EVENTS=1 python tests/kernel_clock_child.py pnp

prints one JSON line: whether the reader refused before the call, the values it returned after it, and the sha256 of the call's product results.
"""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def result_bytes(o):
    """every array and number of a result (dicts by sorted key), bit for bit"""
    if isinstance(o, dict):
        return b"".join(result_bytes(o[k]) for k in sorted(o))
    if isinstance(o, (list, tuple)):
        return b"".join(result_bytes(v) for v in o)
    return np.ascontiguousarray(o).tobytes()


def _read(symbol, n):
    """the n values of a reader; one slot more than n is handed over, and it stays as it was"""
    from eao_fusion_amd import _lib
    ms = np.full(n + 1, -7.0, np.float32)
    _lib.check(getattr(_lib.load(), symbol)(C.cast(_lib.ptr(ms), C.POINTER(C.c_float))))
    assert ms[n] == -7.0, "%s wrote more than %d values" % (symbol, n)
    return [float(v) for v in ms[:n]]


def _run_pnp():
    import pnp_solver_scenes as SC
    from eao_fusion_amd.pnp_solver import pnp_solver_iterate
    c = SC.FAMILIES["x6_n63"]()
    return pnp_solver_iterate(c["prob"], None, c["sets"], c["min_inliers"], c["max_its"], inspect=True)


def _run_initializer():
    import initializer_scenes as SC
    from eao_fusion_amd.initializer import initialize
    prob = SC.friendly("general_96")
    return initialize(prob, prob["sets"], inspect=True)


def _run_triangulation():
    """eao_kf_create_new_map_points over three neighbours of a 300-keypoint search scene, as tests/test_gpu_triangulation.py builds them"""
    import test_gpu_search as TS
    import test_gpu_triangulation as TT
    import triangulation_reference as Y
    from eao_fusion_amd import search, synth
    scene = synth.synth_search_scene(n=300, seed=8002, clutter=0.5, n_nodes=12)
    h, bf = search.product_handles(), scene["bf"]
    nb = TS._neighbours(scene, 3)
    frames = [TT._with_depth(scene["K1"], bf)] + [TT._with_depth(x[0], bf) for x in nb]
    handles = [search.KeyFrameHandle(h.lib, h.check, f, fv) for f, fv in zip(frames, [scene["fv1"]] + [x[1] for x in nb])]
    for hh, f in zip(handles, frames):
        hh.set_depth(f["depth"], f["raw_x"], f["raw_y"])
    cams = [TT._cam_of(scene["T1w"], scene["K"], bf)] + [TT._cam_of(scene["T2w"], scene["K"], bf, dz=0.01 * k) for k in range(3)]
    return search.kf_create_new_map_points(handles[0], cams[0], handles[1:], cams[1:], [x[2] for x in nb], [x[3] for x in nb], [x[4] for x in nb], 0,
                                           Y.ratio_factor(scene["K1"]["scale_factors"][1]), True)


# name: (environment variable, kernels, reader, call)
MODULES = {
    "pnp": ("EAO_PNP_EVENTS", 4, "eao_pnp_solver_last_kernel_ms", _run_pnp),
    "initializer": ("EAO_INIT_EVENTS", 5, "eao_initializer_last_kernel_ms", _run_initializer),
    "triangulation": ("EAO_TRI_EVENTS", 1, "eao_kf_last_triangulation_ms", _run_triangulation),
}


def read(name):
    return _read(MODULES[name][2], MODULES[name][1])


def run(name):
    return result_bytes(MODULES[name][3]())


def main():
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from eao_fusion_amd._lib import EaoError
    name = sys.argv[1]
    try:
        read(name)
        refused = None
    except EaoError as e:
        refused = e.status
    digest = hashlib.sha256(run(name)).hexdigest()
    sys.stdout.write(json.dumps(dict(refused_before=refused, ms=read(name), digest=digest)) + "\n")


if __name__ == "__main__":
    main()
