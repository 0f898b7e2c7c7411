"""GPU: the five per-kernel timing diagnostics that share KernelClock (csrc/common.h): eao_pnp_solver_last_kernel_ms, eao_initializer_last_kernel_ms,
eao_kf_last_triangulation_ms (armed by EAO_PNP_EVENTS / EAO_INIT_EVENTS / EAO_TRI_EVENTS, read once per process: their armed half runs in
tests/kernel_clock_child.py) and eao_iforest_last_kernel_ms, eao_object_assoc_last_kernel_ms (armed by their set_profiling call).  For each: the reader refuses
with EAO_ERR_INVALID on a fresh thread and after an unarmed call, returns exactly N finite values >= 0 after an armed one (-1 in the slot of the object
association's kernel that did not run), and arming changes no byte of the product's results."""
import hashlib
import json
import math
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import isolation_forest_scenes as FS
import kernel_clock_child as KC
import object_association_scenes as OS

from eao_fusion_amd import _lib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _in_thread(fn):
    """fn() on a new thread: the library's per-thread context, its clock included, starts fresh there"""
    box = {}

    def run():
        try:
            box["r"] = fn()
        except BaseException as e:      # noqa: BLE001
            box["e"] = e
    t = threading.Thread(target=run)
    t.start()
    t.join()
    if "e" in box:
        raise box["e"]
    return box["r"]


def _refused(reader):
    with pytest.raises(_lib.EaoError) as ei:
        reader()
    assert ei.value.status == _lib.EAO_ERR_INVALID
    return True


def _measured(v):
    return math.isfinite(v) and v >= 0.0


@pytest.mark.parametrize("name", list(KC.MODULES))
def test_clock_armed_by_the_environment(name):
    import torch  # noqa: F401  (first, so that the library resolves the same HIP runtime)
    var, n, _reader, _call = KC.MODULES[name]
    assert not int(os.environ.get(var, "0")), "%s is set in the test's own process: its half is the unarmed one" % var

    def unarmed():
        _refused(lambda: KC.read(name))
        bits = KC.run(name)
        _refused(lambda: KC.read(name))
        return bits
    bits = _in_thread(unarmed)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] + [v for v in [os.environ.get("PYTHONPATH")] if v]))
    env[var] = "1"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "kernel_clock_child.py"), name], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    got = json.loads(out.stdout.strip().split("\n")[-1])
    print(name, got["ms"])
    assert got["refused_before"] == _lib.EAO_ERR_INVALID
    assert len(got["ms"]) == n and all(_measured(v) for v in got["ms"]), got["ms"]
    assert got["digest"] == hashlib.sha256(bits).hexdigest()


def test_forest_clock_armed_by_set_profiling():
    import torch  # noqa: F401
    from eao_fusion_amd import isolation_forest as IF
    pts = FS.scenes()["gauss_30"]["points"]

    def call():
        return KC.result_bytes(IF.outliers_batch([pts], [0], want_scores=True))

    def body():
        _refused(IF.last_kernel_ms)
        plain = call()
        _refused(IF.last_kernel_ms)
        IF.set_profiling(True)
        try:
            _refused(IF.last_kernel_ms)
            timed = call()
            ms = IF.last_kernel_ms()
            us = IF.last_stage_us()
        finally:
            IF.set_profiling(False)
        _refused(IF.last_kernel_ms)
        _refused(IF.last_stage_us)
        return plain, timed, ms, us
    plain, timed, ms, us = _in_thread(body)
    print("forest", ms, us)
    assert len(ms) == 2 and all(_measured(v) for v in ms)
    assert len(us) == 3 and all(_measured(v) for v in us)
    assert plain == timed


def test_object_association_clock_armed_by_set_profiling():
    import torch  # noqa: F401
    from eao_fusion_amd import object_association as OA
    s, rs = OS.np_scenes()["same_distribution"], OS.rect_scenes()["in_view"]

    def counts():
        return KC.result_bytes(OA.np_counts([s["det"]], [s["map"]], [(0, 0)]))

    def rects():
        return KC.result_bytes(OA.project_rects([rs["points"]], rs["Tcw"], *[rs[k] for k in OS.CAM]))

    def body():
        _refused(OA.last_kernel_ms)
        plain = counts(), rects()
        _refused(OA.last_kernel_ms)
        try:
            OA.set_profiling(True)
            _refused(OA.last_kernel_ms)
            timed_counts = counts()
            ms_counts = [float(v) for v in OA.last_kernel_ms()]
            OA.set_profiling(True)      # (arming again clears: the rect call below is the only one measured)
            timed_rects = rects()
            ms_rects = [float(v) for v in OA.last_kernel_ms()]
        finally:
            OA.set_profiling(False)
        _refused(OA.last_kernel_ms)
        return plain, (timed_counts, timed_rects), ms_counts, ms_rects
    plain, timed, ms_counts, ms_rects = _in_thread(body)
    print("object association", ms_counts, ms_rects)
    assert len(ms_counts) == 2 and _measured(ms_counts[0]) and ms_counts[1] == -1.0
    assert len(ms_rects) == 2 and ms_rects[0] == -1.0 and _measured(ms_rects[1])
    assert plain == timed
