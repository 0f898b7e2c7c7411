"""The class surface include/eaofusion/ObjectMap.h without a device: compiled with g++ over the stand-in Object_Map / MapPoint of
tests/cpp/object_map/object_map_driver.cpp and linked with object_map_stub.cpp, which prints the library call it receives and answers by a made-up rule (point i
is flagged when i % 4 == 1 or it is the object's last).  Checked: what the adapter sends (the point order, the class, one call for a batch), the erase and the
mSumPointsPos writes (src/Object.cc:1324-1347) with the last point the last outlier, the early returns (:1241-1257: no call at all), and a refused call."""
import os
import subprocess

import numpy as np
import pytest

import isolation_forest_scenes as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def hx(a):
    return " ".join("%08x" % v for v in np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32))


def script(objects, bi_forest, batch):
    """objects: [(points, class_id)]"""
    body = ["%d %d %s" % (cls, len(p), hx(p)) for p, cls in objects]
    if batch:
        return "batch %d %d %s\n" % (bi_forest, len(objects), " ".join(body))
    return "".join("single %d %s\n" % (bi_forest, b) for b in body)


def run_driver(exe, text):
    out = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return out.stdout.strip().split("\n")


def split_objects(lines, k):
    """the lines of one `batch` command: ret, then (kept, sum) per object -> per object [ret, kept, sum]"""
    lines = [ln for ln in lines if not ln.startswith("call")]
    assert len(lines) == 1 + 2 * k
    return [[lines[0], lines[1 + 2 * j], lines[2 + 2 * j]] for j in range(k)]


def check_object(lines, points, flags, ret=None):
    """lines: [ret, kept, sum] of one object.  mSumPointsPos: float accumulation of every point in order, then the erased ones subtracted in order."""
    lines = [ln for ln in lines if not ln.startswith("call")]
    points = np.ascontiguousarray(points, np.float32)
    if ret is not None:
        assert lines[0] == "ret %d" % ret
    kept = np.nonzero(np.asarray(flags) == 0)[0]
    assert lines[1] == ("kept %d %s" % (len(kept), " ".join(str(int(i)) for i in kept))).rstrip()
    total = np.zeros(3, np.float32)
    for p in points:
        total = (total + p).astype(np.float32)
    for i in np.nonzero(flags)[0]:
        total = (total - points[i]).astype(np.float32)
    assert lines[2] == "sum " + hx(total)


def stub_flags(n):
    return np.array([1 if (i % 4 == 1 or i == n - 1) else 0 for i in range(n)], np.uint8)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("object_map") / "object_map_surface")
    src = os.path.join(ROOT, "tests", "cpp", "object_map")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"),
                           os.path.join(src, "object_map_driver.cpp"), os.path.join(src, "object_map_stub.cpp"), "-pthread", "-o", path])
    return path


def test_single_object_call_and_erase(exe):
    p = SC._cloud(33, 21)
    got = run_driver(exe, script([(p, 62)], 1, False))
    assert got[0] == "call n_obj 1 bi 1 scores 0 start 0 33 class 62 xyz " + hx(p)      # GetWorldPos() in vector order, mnClass, no scores asked for
    check_object(got[1:], p, stub_flags(33), ret=int(stub_flags(33).sum()))      # the last point is the last outlier: nothing is read past the list


def test_early_returns_make_no_call(exe):
    p40, p29 = SC._cloud(40, 22), SC._cloud(29, 23)
    for pts, cls, bi in ((p40, 0, 0), (p40, 75, 1), (p40, 64, 1), (p40, 65, 1), (p29, 0, 1)):
        got = run_driver(exe, script([(pts, cls)], bi, False))
        assert not any(ln.startswith("call") for ln in got)
        check_object(got, pts, np.zeros(len(pts), np.uint8), ret=0)
    got = run_driver(exe, script([(SC._cloud(30, 24), 63)], 1, False))      # 30 points, a class next to the exempt ones: runs
    assert got[0].startswith("call n_obj 1 bi 1 ")


def test_batch_is_one_call_over_the_objects_that_run(exe):
    objs = [(SC._cloud(31, 25), 0), (SC._cloud(29, 26), 0), (SC._cloud(40, 27), 75), (SC._cloud(36, 28), 62)]
    got = run_driver(exe, script(objs, 1, True))
    calls = [ln for ln in got if ln.startswith("call")]
    assert calls == ["call n_obj 2 bi 1 scores 0 start 0 31 67 class 0 62 xyz " + hx(np.concatenate([objs[0][0], objs[3][0]]))]
    per = split_objects(got, 4)
    want = [stub_flags(31), np.zeros(29, np.uint8), np.zeros(40, np.uint8), stub_flags(36)]
    assert per[0][0] == "ret %d" % int(want[0].sum() + want[3].sum())
    for (p, _), g, w in zip(objs, per, want):
        check_object(g, p, w)
    assert not any(ln.startswith("call") for ln in run_driver(exe, script(objs, 0, True)))      # biForest off: no call


def test_refused_call_leaves_the_objects_unchanged(exe):
    objs = [(SC._cloud(31, 29), 0), (SC._cloud(32, 30), 999)]
    got = run_driver(exe, script(objs, 1, True))
    per = split_objects(got, 2)
    assert per[0][0] == "ret -1"
    for (p, _), g in zip(objs, per):
        check_object(g, p, np.zeros(len(p), np.uint8))
