"""The point-list half of the class surface include/eaofusion/ObjectMap.h without a device: compiled with g++ over the stand-in Object_Map / MapPoint / Object_2D /
Frame of tests/cpp/object_points/object_points_driver.cpp and linked with object_points_stub.cpp, which prints every library call it receives and answers by
made-up rules (restated in stub_answer below).  Checked: what each of the four functions sends (stages, lists, counts, the caller's edge flag and frame count,
the pose, the bounds); the host writes in upstream's order -- object_id, object_class and the count of the gated-in candidates, the have_feature / feature copies
through target[j] in candidate order so that the last writer wins, the appended points on both lists, the erases, mSumPointsPos --; where step2 runs; the cuboid
and the forest behind it; a rejected, a refused and a declined call leaving everything as it was; a list entry that is itself a candidate keeping its raised
count."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def hx(a):
    return " ".join("%08x" % v for v in np.ascontiguousarray(a, f32).reshape(-1).view(np.uint32))


def hx64(a):
    return " ".join("%016x" % v for v in np.ascontiguousarray(a, np.float64).reshape(-1).view(np.uint64))


def point(pid, xyz, count=-1, have=0, feature=0):
    return dict(id=pid, xyz=np.asarray(xyz, f32), count=count, have=have, feature=feature)


def point_text(p):
    return "%d %s %d %d %d" % (p["id"], hx(p["xyz"]), p["count"], p["have"], p["feature"])


def object_text(oid, cls, frames, rmax, pts):
    return "%d %d %d %s %d %s" % (oid, cls, frames, hx([rmax]), len(pts), " ".join(point_text(p) for p in pts))


def stub_answer(n_map, n_cand, gate, erase):
    """the stub's rules: (gate, target, appended candidates, erased per final-list position)"""
    g = [int(gate != 0 and j % 3 != 2) for j in range(n_cand)]
    target = [(0 if n_map > 0 else n_map) if g[j] and j % 3 == 1 else -1 for j in range(n_cand)]
    app = [j for j in range(n_cand) if g[j] and j % 3 == 0]
    erased = [int(erase != 0 and k % 2 == 1) for k in range(n_map + len(app))]
    return g, target, app, erased


def call_line(cg, gate, erase, edge, lst, cand, nf=0, rect1=(0, 0, 0, 0), box=(0, 0, 0, 0), frame=False, center=(0, 0, 0), rmax=0.0, extent=(0, 0, 0), pose=None, cc=(0, 0, 0),
              bounds=(0,) * 6, overlap=(0, 0, 0)):
    """the line the stub prints for a desc; `lst` and `cand` are the points as the adapter must have gathered them (a count of -1 is sent as 0)"""
    tcw = TCW if frame else [0] * 16
    s = np.zeros(3, f32)
    for p in lst:
        s = (s + p["xyz"]).astype(f32)      # the driver's mSumPointsPos: float adds in list order
    pts = lambda ps: " ".join("%s %d" % (hx(p["xyz"]), max(p["count"], 0)) for p in ps)      # noqa: E731
    parts = ["call points cg %d gate %d erase %d edge %d n_map %d n_cand %d nf %d cols %d rows %d rect1 %d %d %d %d box %d %d %d %d" % (
        (cg, gate, erase, edge, len(lst), len(cand), nf) + ((640, 480) if frame else (0, 0)) + tuple(rect1) + tuple(box)),
        "tcw " + hx(tcw), "k " + hx([500, 501, 320, 240] if frame else [0] * 4), "center " + hx(center) + " " + hx([rmax]), "extent " + hx(extent),
        "pose " + hx64(pose if pose is not None else [0] * 7), "cc " + hx64(cc), "bounds " + hx(bounds), "overlap " + hx(overlap), "sum " + hx(s),
        ("map " + pts(lst)).rstrip(), ("cand " + pts(cand)).rstrip()]
    return " ".join(parts)


def state_lines(ret, list_ids, new_ids, total, points, oid):
    out = ["ret %d" % ret, ("list " + " ".join(map(str, list_ids))).rstrip(), ("new " + " ".join(map(str, new_ids))).rstrip(), "sum " + hx(total)]
    for p in sorted(points, key=lambda p: p["id"]):
        out.append("pt %d %d %d %d %d %d" % (p["id"], p.get("object_id", -1), p.get("object_class", -1), p["count"], p["have"], p["feature"]))
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("object_points") / "object_points_surface")
    src = os.path.join(ROOT, "tests", "cpp", "object_points")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DEAOFUSION_FORCE_CV_COMPAT",
                           "-I", os.path.join(ROOT, "include"), os.path.join(src, "object_points_driver.cpp"), os.path.join(src, "object_points_stub.cpp"), "-pthread",
                           "-o", path])
    return path


def run_driver(exe, text):
    out = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return [ln.rstrip() for ln in out.stdout.strip().split("\n")]


OID, CLS, RMAX = 5, 3, 1.75
TCW = [1, 0, 0, 0.5, 0, 1, 0, -0.25, 0, 0, 1, 2.0, 0, 0, 0, 1]      # the driver's Frame
CENTER = (0.25, 0.5, 0.75)
POSE = [0.125, -0.25, 0.5, 0.75, 1.5, 2.5, 3.5]
EXTENT = (2.5, 3.5, 4.5)
STUB_SUM, CUBOID_SUM = [10.5, 11.5, 12.5], [20.5, 21.5, 22.5]


def the_list(n=4, counts=(-1, 8, 2, 0)):
    return [point(1 + i, [i + 0.5, -i, 2.0 * i], counts[i % len(counts)], i % 2, 100 + i) for i in range(n)]


def the_candidates(n=7, base=10):
    return [point(base + j, [10.0 + j, 0.25 * j, -1.0 * j], [-1, 0, 3, 8, 1, 2, 7][j % 7], (j + 1) % 2, 200 + j) for j in range(n)]


def dau_text(Flag, bi, ok, box, rect1x, lst, cand, cls=CLS, frames=5):
    return "dau %d %d %d %d %d %d %d %d %s %d %d %s\n" % ((Flag, bi, ok) + tuple(box) + (rect1x, object_text(OID, CLS, frames, RMAX, lst), cls, len(cand),
                                                                                       " ".join(point_text(p) for p in cand)))


def applied(lst, cand, gate_kind, erase_kind, current_new, keep=()):
    """the state the adapter must leave behind the stub's answer: (list ids, new ids, the points with their members)"""
    g, target, app, erased = stub_answer(len(lst), len(cand), gate_kind, erase_kind)
    pts = {p["id"]: dict(p) for p in lst + cand}
    final = [p["id"] for p in lst] + [cand[j]["id"] for j in app]
    for j, c in enumerate(cand):
        if not g[j]:
            continue
        me = pts[c["id"]]
        me["object_id"], me["object_class"], me["count"] = OID, CLS, max(c["count"], 0) + 1
        if target[j] >= 0:
            old = pts[final[target[j]]]
            old["have"], old["feature"] = c["have"], c["feature"]      # in candidate order: the last writer wins
    left = [pid for k, pid in enumerate(final) if not erased[k] or k in keep]
    return left, ([cand[j]["id"] for j in app] if current_new else []), list(pts.values()), sum(e for k, e in enumerate(erased) if k not in keep), len(app)


def test_data_associate_update_writes_in_upstreams_order(exe):
    lst, cand = the_list(), the_candidates()
    got = run_driver(exe, dau_text(2, 1, 1, (30, 30, 100, 100), 7, lst, cand))
    left, new, pts, _, _ = applied(lst, cand, 1, 1, True)
    assert [c["id"] for j, c in enumerate(cand) if j % 3 == 1] == [11, 14] and next(p for p in pts if p["id"] == 1)["feature"] == 204      # candidate 4 wrote last
    want = [call_line(1, 1, 1, 1, lst, cand, nf=6, rect1=(7, 2, 3, 4), box=(30, 30, 100, 100), frame=True, center=CENTER, rmax=RMAX), "step2",
            "call cuboids n_obj 1 points %d" % len(left)] + state_lines(1, left, new, CUBOID_SUM, pts, OID)
    assert got == want
    assert left == [1, 3, 10, 16] and new == [10, 13, 16]


@pytest.mark.parametrize("Flag,box,cg,edge", [(1, (30, 30, 100, 100), 0, 1), (4, (26, 26, 588, 428), 0, 1), (3, (25, 30, 100, 100), 1, 0), (2, (30, 25, 100, 100), 1, 0),
                                              (2, (30, 30, 585, 100), 1, 0), (2, (30, 30, 100, 425), 1, 0), (2, (26, 26, 588, 428), 1, 1)])
def test_flags_and_the_edge_condition(exe, Flag, box, cg, edge):
    lst, cand = the_list(), the_candidates(2)
    got = run_driver(exe, dau_text(Flag, 0, 1, box, 7, lst, cand, frames=4))
    assert got[0] == call_line(cg, 1, 1, edge, lst, cand, nf=5, rect1=(7, 2, 3, 4), box=box, frame=True, center=CENTER, rmax=RMAX)


def test_the_forest_follows_the_cuboid(exe):
    lst, cand = the_list(80), the_candidates(3, base=1000)
    got = run_driver(exe, dau_text(1, 1, 1, (30, 30, 100, 100), 7, lst, cand))
    left = applied(lst, cand, 1, 1, True)[0]
    assert got[1:4] == ["step2", "call cuboids n_obj 1 points %d" % len(left), "call iforest n_obj 1 bi 1 points %d" % len(left)] and got[4] == "ret 1"


@pytest.mark.parametrize("case", ["rejected", "step2_declines", "another_class", "refused"])
def test_nothing_is_written(exe, case):
    lst, cand = the_list(), the_candidates()
    if case == "refused":
        lst[0]["xyz"][0] = 999.0
    text = dau_text(2, 1, int(case != "step2_declines"), (30, 30, 100, 100), -1 if case == "rejected" else 7, lst, cand, cls=CLS + (case == "another_class"))
    got = run_driver(exe, text)
    s = np.zeros(3, f32)
    for p in lst:
        s = (s + p["xyz"]).astype(f32)
    state = state_lines(-1 if case == "refused" else 0, [p["id"] for p in lst], [], s, lst + cand, OID)
    calls = {"rejected": 1, "step2_declines": 2, "another_class": 0, "refused": 1}[case]
    assert got[calls:] == state and len(got) == calls + len(state)
    assert ("step2" in got) == (case == "step2_declines") and not any(ln.startswith("call cuboids") for ln in got)


def test_an_entry_that_is_itself_a_candidate_keeps_its_raised_count(exe):
    """entry 1 (count 8) and entry 3 (count 7) are erased by the stub's rule; both are gated-in candidates too, so step 3 raised their counts to 9 and 8: above 8 stays"""
    lst = the_list(4, counts=(0, 8, 0, 7))
    cand = [lst[1], lst[3], point(20, [7, 7, 7]), point(21, [8, 8, 8], 2)]
    got = run_driver(exe, dau_text(1, 0, 1, (30, 30, 100, 100), 7, lst, cand))
    assert got[0] == call_line(0, 1, 1, 1, lst, cand, nf=6, rect1=(7, 2, 3, 4), box=(30, 30, 100, 100), frame=True, center=CENTER, rmax=RMAX)      # the counts of before
    assert got[3] == "ret 1" and got[4] == "list 1 2 3 2"      # (the stub appends candidate 0, its own rule) entry 1 stays, entry 3 and the appended 21 go
    assert "pt 2 5 3 9 1 101" in got and "pt 4 5 3 8 1 103" in got


def test_merge_two_map_objs_points(exe):
    lst, rep = the_list(), the_candidates()
    got = run_driver(exe, "merge %s %s\n" % (object_text(OID, CLS, 2, RMAX, lst), object_text(9, CLS, 1, RMAX, rep)))
    left, new, pts, _, n_app = applied(lst, rep, 2, 0, False)
    # the counts sent are those under THIS object's id: the other object's points have none
    sent = [dict(p, count=-1) for p in rep]
    for p in pts:
        if p["id"] >= 10 and p.get("object_id") == OID:
            p["count"] = 1
        elif p["id"] >= 10:
            p["count"] = -1
    assert got == [call_line(0, 2, 0, 0, lst, sent, extent=EXTENT, pose=POSE)] + state_lines(n_app, left, new, STUB_SUM, pts, OID)
    assert n_app == 3 and left == [1, 2, 3, 4, 10, 13, 16]


def test_big_to_small(exe):
    lst = the_list(5)
    bounds = [0.5, 1.5, -2.0, 2.0, 0.0, 9.0]
    got = run_driver(exe, "big %s %s\n" % (object_text(OID, CLS, 2, RMAX, lst), hx(bounds)))
    assert got == [call_line(0, 0, 2, 0, lst, [], bounds=bounds), "call cuboids n_obj 1 points 3"] + state_lines(2, [1, 3, 5], [], CUBOID_SUM, lst, OID)


def test_divide_equally_two_objs(exe):
    lst = the_list(3)
    cc, extent, overlap = [0.5, -0.25, 3.0], [1.0, 2.0, 3.0], [0.25, 0.5, 0.75]
    got = run_driver(exe, "divide %s %s %s %s\n" % (object_text(OID, CLS, 2, RMAX, lst), hx64(cc), hx(extent), hx(overlap)))
    assert got == [call_line(0, 0, 3, 0, lst, [], cc=cc, extent=extent, overlap=overlap)] + state_lines(1, [1, 3], [], STUB_SUM, lst, OID)
