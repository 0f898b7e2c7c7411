"""The class surface include/eaofusion/ObjectAssociation.h without a device: compiled with g++ over the stand-in Object_2D / Object_Map / MapPoint / Frame of
tests/cpp/object_association/object_association_driver.cpp and linked with object_association_stub.cpp, which prints the library call it receives and answers by
a made-up rule (rank-sum: verdict 1 + nGood % 3; rects: {j, n, cols, rows} with status 0 / 2 / 1 for n == 0 / n % 5 == 4 / else).  Checked: what the adapter
sends (the good points only, S, the pair order of the descending loop, one call per detection), no call when m < 20, verdict 3 mapped to 2, the class and
bBadErase filters, the 30-frame rule with upstream's unsigned arithmetic, and the rect that stays untouched."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANTED = "rect -1 -2 -3 -4"


def hx(a):
    return " ".join("%08x" % v for v in np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32))


def cloud(n, seed):
    return np.random.RandomState(seed).normal(0, 1, (n, 3)).astype(np.float32)


def points(p, flags=None):
    flags = np.zeros(len(p), int) if flags is None else flags
    return " ".join(["%d" % len(p)] + ["%d %s" % (f, hx(q)) for q, f in zip(p, flags)])


def det(cls, p, flags=None):
    return "%d %s" % (cls, points(p, flags))


def mapobj(cls, p, flags=None, erase=0, last_add=0):
    return "%d %d %d %s" % (cls, erase, last_add, points(p, flags))


def frame(mn_id, cam=(500.0, 510.0, 320.0, 240.0), Tcw=None):
    return "%d %s %s" % (mn_id, hx(cam), hx(np.eye(4, dtype=np.float32) if Tcw is None else Tcw))


def run_driver(exe, text):
    out = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return out.stdout.strip().split("\n")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("object_association") / "object_association_surface")
    src = os.path.join(ROOT, "tests", "cpp", "object_association")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-sign-compare", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                           os.path.join(ROOT, "include"), os.path.join(src, "object_association_driver.cpp"), os.path.join(src, "object_association_stub.cpp"),
                           "-o", path])
    return path


def test_single_pair_sends_the_good_points_and_S(exe):
    d, m = cloud(24, 1), cloud(33, 2)      # 33 points, 3 of them bad: nGood = 30 -> the stub answers 1
    dflags, mflags = np.zeros(24, int), np.zeros(33, int)
    dflags[[2, 5]] = [1, 2]
    mflags[[0, 7, 32]] = [1, 2, 1]
    got = run_driver(exe, "single %s %s\n" % (det(3, d, dflags), mapobj(3, m, mflags)))
    assert got[0] == ("call np n_det 1 det_start 0 22 n_map 1 map_start 0 30 map_total 33 pairs 0:0 w 0 r 0 det %s map %s" % (hx(d[dflags == 0]), hx(m[mflags == 0])))
    assert got[1] == "ret 1"


def test_verdicts_and_the_mapping_of_undefined(exe):
    d = cloud(20, 3)
    for n_good, want in ((30, 1), (31, 2), (32, 2)):      # the stub's 3 (EAO_OBJECT_NP_UNDEFINED) becomes 2
        got = run_driver(exe, "single %s %s\n" % (det(0, d), mapobj(0, cloud(n_good, 4))))
        assert got[-1] == "ret %d" % want


def test_fewer_than_20_good_points_make_no_call(exe):
    d, flags = cloud(21, 5), np.zeros(21, int)
    flags[[1, 20]] = [2, 1]      # 19 good
    got = run_driver(exe, "single %s %s\n" % (det(0, d, flags), mapobj(0, cloud(30, 6))))
    assert got == ["ret 0"]
    got = run_driver(exe, "cands %s 2 %s %s\n" % (det(0, d, flags), mapobj(0, cloud(30, 7)), mapobj(0, cloud(30, 8))))
    assert got == ["ret 0", "ids 777"]


def test_candidates_one_call_in_descending_order_with_the_filters(exe):
    d = cloud(25, 9)
    objs = [(5, cloud(30, 10), 0), (5, cloud(31, 11), 0), (6, cloud(30, 12), 0), (5, cloud(30, 13), 1), (5, cloud(32, 14), 0), (5, cloud(33, 15), 0)]
    mflags = np.zeros(30, int)
    mflags[4] = 1      # object 0: 29 good of S = 30 -> nGood % 3 == 2 -> 3 -> 2
    body = " ".join(mapobj(c, p, mflags if i == 0 else None, erase=e) for i, (c, p, e) in enumerate(objs))
    got = run_driver(exe, "cands %s %d %s\n" % (det(5, d), len(objs), body))
    calls = [ln for ln in got if ln.startswith("call")]
    order = [5, 4, 1, 0]      # descending; object 2 is another class, object 3 is marked bBadErase
    good = [objs[i][1] if i else objs[0][1][mflags == 0] for i in order]
    starts = np.cumsum([0] + [len(g) for g in good])
    assert calls == ["call np n_det 1 det_start 0 25 n_map 4 map_start %s map_total %s pairs 0:0 0:1 0:2 0:3 w 0 r 0 det %s map %s" % (
        " ".join(str(int(s)) for s in starts), " ".join(str(len(objs[i][1])) for i in order), hx(d), hx(np.concatenate(good)))]
    # the stub: 33 -> 1, 32 -> 3, 31 -> 2, 29 -> 3: only object 5 is pushed, behind what the vector held
    assert got[-2:] == ["ret 1", "ids 777 5"]
    objs2 = [(5, cloud(30, 16), 0), (5, cloud(36, 17), 0), (5, cloud(33, 18), 0)]
    got = run_driver(exe, "cands %s 3 %s\n" % (det(5, d), " ".join(mapobj(c, p, erase=e) for c, p, e in objs2)))
    assert got[-2:] == ["ret 3", "ids 777 2 1 0"] and len([ln for ln in got if ln.startswith("call")]) == 1
    got = run_driver(exe, "cands %s 1 %s\n" % (det(4, d), mapobj(5, cloud(30, 19))))      # no object of the class: no call
    assert got == ["ret 0", "ids 777"]


def test_refused_call(exe):
    got = run_driver(exe, "cands %s 1 %s\nsingle %s %s\n" % (det(0, cloud(99, 20)), mapobj(0, cloud(30, 21)), det(0, cloud(99, 20)), mapobj(0, cloud(30, 21))))
    got = [ln for ln in got if not ln.startswith("call")]
    assert got == ["ret -1", "ids 777", "ret -1"]


def test_single_rect_sends_every_point_and_the_frame(exe):
    p, flags = cloud(7, 22), np.zeros(7, int)
    flags[[1, 3]] = [1, 2]      # ComputeProjectRectFrame does not filter (:1612)
    T = np.arange(16, dtype=np.float32).reshape(4, 4) / 7
    got = run_driver(exe, "rect %s 640 480 %s\n" % (frame(100, Tcw=T), mapobj(0, p, flags)))
    assert got[0] == "call rects n_map 1 map_start 0 7 cols 640 rows 480 uv 0 cam %s Tcw %s xyz %s" % (hx([500.0, 510.0, 320.0, 240.0]), hx(T), hx(p))
    assert got[1:] == ["ret 1", "rect 0 7 640 480"]
    for n, ret in ((0, 0), (4, 0)):      # status 0 and status 2: mRectProject stays
        got = run_driver(exe, "rect %s 640 480 %s\n" % (frame(100), mapobj(0, cloud(n, 23))))
        assert got[-2:] == ["ret %d" % ret, PLANTED]
    got = run_driver(exe, "rect %s 999 480 %s\n" % (frame(100), mapobj(0, cloud(5, 24))))
    assert got[-2:] == ["ret -1", PLANTED]


def test_step_10_1_in_one_call(exe):
    # frame 100: seen after frame 70 is recent (mnLastAddID > mnId - 30)
    objs = [(cloud(5, 25), 0, 71), (cloud(6, 26), 0, 70), (cloud(7, 27), 1, 99), (cloud(9, 28), 0, 100), (cloud(0, 29), 0, 90), (cloud(8, 30), 0, 80)]
    body = " ".join(mapobj(0, p, erase=e, last_add=la) for p, e, la in objs)
    got = run_driver(exe, "rects %s 640 480 %d %s\n" % (frame(100), len(objs), body))
    recent = [0, 3, 4, 5]
    starts = np.cumsum([0] + [len(objs[i][0]) for i in recent])
    assert got[0].startswith("call rects n_map 4 map_start %s cols 640 rows 480 uv 0 " % " ".join(str(int(s)) for s in starts))
    assert got[0].endswith(" xyz " + hx(np.concatenate([objs[i][0] for i in recent])))
    assert len([ln for ln in got if ln.startswith("call")]) == 1
    # object 1: not recent -> Rect(0, 0, 0, 0); object 2: bBadErase, untouched; object 3: 9 points -> status 2, untouched; object 4: no points, untouched
    assert got[1:] == ["ret 2", "rect 0 5 640 480", "rect 0 0 0 0", PLANTED, PLANTED, PLANTED, "rect 3 8 640 480"]
    # frame 10: mnId - 30 wraps in upstream's long unsigned arithmetic, nothing is recent and there is no call
    got = run_driver(exe, "rects %s 640 480 2 %s %s\n" % (frame(10), mapobj(0, cloud(5, 31), last_add=9), mapobj(0, cloud(5, 32), erase=1, last_add=9)))
    assert got == ["ret 0", "rect 0 0 0 0", PLANTED]
