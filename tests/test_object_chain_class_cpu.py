"""DataAssociateUpdateChained of the class surface include/eaofusion/ObjectMap.h without a device: compiled with g++ over the stand-in Object_Map / MapPoint /
Object_2D / Frame of tests/cpp/object_chain/object_chain_driver.cpp and linked with object_chain_stub.cpp, which prints every library call it receives and answers
by made-up rules.  Checked: the chained form makes ONE library call and not three; what it sends beside the points desc (the bad flags, the alias of a candidate
that is a list entry, the centroids with the detection's own pushed last, the class and the forest flag); the library call comes before step2 and every host write
behind it; and DataAssociateUpdateChained and DataAssociateUpdate, fed the same stub answers, leave the same members, lists and MapPoint fields."""
import os
import subprocess

import numpy as np
import pytest

from test_object_points_class_cpu import hx, object_text, point, point_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("object_chain") / "object_chain_surface")
    src = os.path.join(ROOT, "tests", "cpp", "object_chain")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DEAOFUSION_FORCE_CV_COMPAT",
                           "-I", os.path.join(ROOT, "include"), os.path.join(src, "object_chain_driver.cpp"), os.path.join(src, "object_chain_stub.cpp"), "-pthread",
                           "-o", path])
    return path


def run_driver(exe, text):
    out = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return [ln.rstrip() for ln in out.stdout.strip().split("\n")]


def script(verb, lst, cand, flag=1, bi=1, ok=1, box=(100, 100, 50, 50), rect_x=1, cls=3, det_cls=3, frames=2):
    return "%s %d %d %d %d %d %d %d %d %s %d %d %s\n" % ((verb, flag, bi, ok) + tuple(box) + (rect_x, object_text(7, cls, frames, 0.75, lst), det_cls, len(cand),
                                                                                           " ".join(point_text(p) for p in cand)))


def scene():
    """five list points, one of them bad (id 1002) and one seen again as a candidate (id 1); six candidates, one of them bad (id 1011)"""
    lst = [point(0, [0.1, 0.2, 0.3], 4, 1, 11), point(1, [1, 2, 3], 8, 0, 12), point(1002, [2, 2, 2], 2), point(3, [3, 1, 2], -1), point(4, [4, 4, 4], 9)]
    cand = [point(10, [5, 5, 5], -1, 1, 21), point(1, [1, 2, 3], 8, 0, 12), point(12, [6, 6, 6], 3), point(1011, [7, 7, 7], -1), point(14, [8, 8, 8], 0, 1, 22), point(15, [9, 9, 9], 1)]
    return lst, cand


def split(lines):
    calls = [ln for ln in lines if ln.startswith("call ")]
    return calls, [ln for ln in lines if not ln.startswith("call ")]


def test_one_library_call_and_what_it_sends(exe):
    lst, cand = scene()
    lines = run_driver(exe, script("chained", lst, cand))
    calls, rest = split(lines)
    assert len(calls) == 1 and calls[0].startswith("call chain n_map 5 n_cand 6 class 3 bi 1 centroids 3 last " + hx([0.5, 0.25, 1.5]))
    assert calls[0].endswith("bad 0 0 1 0 0 | 0 0 0 1 0 0 alias -1 1 -1 -1 -1 -1")
    assert lines.index(calls[0]) < lines.index("step2") < lines.index("ret 1")      # the call, then step2, then the host writes
    three, _ = split(run_driver(exe, script("dau", lst, cand)))
    assert [c.split()[1] for c in three] == ["points", "cuboids"]      # (the forest's own entry is not asked below 30 points: three calls on a longer list)


@pytest.mark.parametrize("kw", [dict(), dict(flag=2), dict(bi=0), dict(box=(10, 10, 50, 50)), dict(frames=5), dict(cls=75, det_cls=75), dict(ok=0), dict(flag=2, rect_x=-1),
                                dict(det_cls=4)])
def test_both_forms_leave_the_same_members(exe, kw):
    lst, cand = scene()
    _, a = split(run_driver(exe, script("dau", lst, cand, **kw)))
    _, b = split(run_driver(exe, script("chained", lst, cand, **kw)))
    assert a == b
    assert any(ln.startswith("ret ") for ln in a)


def test_a_refused_call_leaves_everything_as_it_was(exe):
    lst, cand = scene()
    lst[0] = point(0, [999, 0, 0], 4, 1, 11)
    _, a = split(run_driver(exe, script("dau", lst, cand)))
    _, b = split(run_driver(exe, script("chained", lst, cand)))
    assert a == b and "ret -1" in b and "step2" not in b
    assert "list 0 1 1002 3 4" in b


def test_the_bad_points_leave_both_lists_alike(exe):
    lst, cand = scene()
    _, b = split(run_driver(exe, script("chained", lst, cand, box=(10, 10, 50, 50))))      # off the edge flag: erase by the stub's rule only where erase != NONE
    ids = [int(v) for v in next(ln for ln in b if ln.startswith("list")).split()[1:]]
    assert 1002 not in ids and 0 in ids


def test_the_order_of_the_host_writes(exe):
    """the append, then the erase by the stub's flags over the list as the append left it, then the bad points among the survivors, then the cuboid's members: the
    end state worked out from the stub's rules.  The list after the append is 0 1 1002 3 4 10 1011; the rule erases positions 1, 3 and 5, of which position 1 (id 1,
    count 8, seen again as candidate 1) stays by the alias rule; of the survivors 0 1 1002 4 1011 the bad ones leave.  Any other order of the three list writes
    gives another list: the bad-point erase indexes the survivors, so it lands on other entries when it runs on the list before the erase."""
    lst, cand = scene()
    _, b = split(run_driver(exe, script("chained", lst, cand)))
    assert b[:4] == ["step2", "ret 1", "list 0 1 4", "new 10 1011"]
    assert b[4] == "sum " + hx([20.5, 21.5, 22.5])      # the cuboid record's sum, written after apply_erase's (10.5, 11.5, 12.5)
    pts = {int(ln.split()[1]): ln.split()[2:] for ln in b if ln.startswith("pt ")}
    assert pts[10][:3] == ["7", "3", "1"] and pts[1][:3] == ["7", "3", "9"] and pts[12][0] == "-1"      # object_id, object_class, the raised count; j % 3 == 2 stays out
    assert pts[0][3:] == ["1", "22"]      # have_feature / feature through target[j] in candidate order: candidate 4 is the last writer on entry 0
