"""The class surface include/eaofusion/FrameObjects.h without a device: compiled with g++ over the stand-in Frame / MapPoint / Object_2D of
tests/cpp/frame_objects/frame_objects_driver.cpp and linked with frame_objects_stub.cpp, which prints the library call it receives and answers by a made-up rule
(box k: assigned = the keypoints with a map point and i % (k + 2) == 0, kept = assigned without its first entry; bad for k % 3 == 1, on_edge for odd k, a feature
box for even k).  Checked: what the adapter sends (NULL and isBad() map points as -1, one id per MapPoint, the boxes, scores, pose and intrinsics, capacities
no list can exceed), every member it writes, the order of the `feature` writes (keypoint by keypoint, box by box), the erase of the bad objects, the members it
leaves alone, a refused call, and the overload over several frames."""
import os
import subprocess

import numpy as np
import pytest

import frame_objects_reference as Y
import frame_objects_scenes as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def hx(a):
    return " ".join("%08x" % v for v in np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("frame_objects") / "frame_objects_surface")
    src = os.path.join(ROOT, "tests", "cpp", "frame_objects")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-DEAOFUSION_FORCE_CV_COMPAT", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "include"), os.path.join(src, "frame_objects_driver.cpp"), os.path.join(src, "frame_objects_stub.cpp"), "-o", path])
    return path


def run_driver(exe, mode, frames):
    out = subprocess.run([exe, mode], input="".join(Y.walk_script(fr) for fr in frames), capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return out.stdout.strip().split("\n")


def small_frame(seed, n_kp=23, n_box=5, **cam):
    rs = np.random.RandomState(seed)
    kp = rs.uniform(0, 600, (n_kp, 2)).astype(np.float32)
    ids = np.arange(n_kp, dtype=np.int32)
    ids[[3, 8]] = -1          # no map point
    ids[6] = -2               # a map point whose isBad() is true
    ids[12] = ids[4] = 40     # one MapPoint at two keypoints
    boxes = [(10 * k, 20 * k, 50 + k, 60 + k) for k in range(n_box)]
    return SC.frame(kp, SC.cloud(rs, n_kp), boxes, ids=ids, score=rs.uniform(0.3, 0.9, n_box), Tcw=SC.pose(seed), **cam)


def stub_rule(fr):
    """what the stub answers for a frame and what the adapter must make of it: (sent ids, per box dict, writes)"""
    ids = np.asarray(fr["mp_id"])
    sent, seen = [], {}
    for v in ids:
        sent.append(-1 if v < 0 else seen.setdefault(int(v), len(seen)))
    boxes, writes = [], []
    M = len(fr["boxes"])
    for k in range(M):
        assigned = [i for i in range(len(ids)) if ids[i] >= 0 and i % (k + 2) == 0]
        boxes.append(dict(assigned=assigned, kept=assigned[1:], bad=k % 3 == 1, on_edge=k % 2 == 1, has_rect=k % 2 == 0))
    for i in range(len(ids)):
        for k in range(M):
            if i in boxes[k]["assigned"]:
                writes.append("write %d %d" % (ids[i], i))
    return sent, boxes, writes


def first_keypoint(fr, i):
    ids = np.asarray(fr["mp_id"])
    return int(np.nonzero(ids == ids[i])[0][0])


def check_frame(fr, lines, sent_line):
    sent, boxes, writes = stub_rule(fr)
    tok = sent_line.split()
    n_kp, M = len(sent), len(boxes)
    assert tok[2:10] == ["n_kp", str(n_kp), "n_box", str(M), "cols", str(fr["cols"]), "rows", str(fr["rows"])]
    at = tok.index("cam")
    assert tok[at + 1:at + 5] == hx([fr["fx"], fr["fy"], fr["cx"], fr["cy"]]).split() and tok[at + 6:at + 22] == hx(fr["Tcw"]).split()
    at = tok.index("ids")
    assert [int(v) for v in tok[at + 1:at + 1 + n_kp]] == sent
    at = tok.index("kp")
    assert tok[at + 1:at + 1 + 2 * n_kp] == hx(np.column_stack([fr["kp_x"], fr["kp_y"]])).split()
    at = tok.index("xyz")
    held = [first_keypoint(fr, i) for i in range(n_kp) if sent[i] >= 0]      # a MapPoint has one position: the driver gives it its first keypoint's
    assert tok[at + 1:tok.index("boxes")] == hx(np.asarray(fr["mp_xyz"])[held]).split()
    at = tok.index("boxes")
    assert [int(v) for v in tok[at + 1:at + 1 + 4 * M]] == [int(v) for v in np.asarray(fr["boxes"]).reshape(-1)]
    assert tok[tok.index("score") + 1:] == hx(fr["score"]).split()
    # what the adapter wrote
    assert [l for l in lines if l.startswith("write ")] == writes
    alive = [k for k in range(M) if not boxes[k]["bad"]]
    assert [l for l in lines if l.startswith("survivors")] == [("survivors " + " ".join(str(k) for k in alive)).rstrip()]
    objs = {int(l.split()[1]): l.split()[2:] for l in lines if l.startswith("obj ")}
    lists = {int(l.split()[1]): [int(v) for v in l.split()[2:]] for l in lines if l.startswith("list ")}
    assert sorted(objs) == alive
    for k in alive:
        b = boxes[k]
        rect = [k, k + 1, k + 2, k + 3] if b["has_rect"] else [-1, -2, -3, -4]      # the planted rect stays where upstream does not assign
        fl = [k + 0.5, len(b["assigned"]), 2, 1.5, k, 3, 0.25, 0.5, k, 10 + k, 20 + k]
        assert objs[k] == [str(len(b["kept"])), str(int(b["on_edge"]))] + [str(v) for v in rect] + hx(fl).split(), k
        assert lists[k] == [first_keypoint(fr, i) for i in b["kept"]], k
    viewed = sorted({int(np.asarray(fr["mp_id"])[i]) for b in boxes for i in b["assigned"]})
    assert [l for l in lines if l.startswith("views")] == [("views " + " ".join(str(v) for v in viewed)).rstrip()]


def test_one_frame(exe):
    fr = small_frame(1)
    lines = run_driver(exe, "single", [fr])
    valid = int((np.asarray(fr["mp_id"]) >= 0).sum())
    assert lines[0] == "call frames 1 caps %d %d" % (valid * 5, valid * 5)
    assert lines[2] == "frame 0 ret 3"      # boxes 1 and 4 are bad
    check_frame(fr, lines[3:], lines[1])


def test_frame_without_boxes_and_frame_without_keypoints(exe):
    lines = run_driver(exe, "single", [SC.scenes()["frame_without_boxes"][0], SC.scenes()["frame_without_keypoints"][0]])
    assert "frame 0 ret 0" in lines and "frame 1 ret 1" in lines and not [l for l in lines if l.startswith("write ")]


def test_refused_call_writes_nothing(exe):
    fr = small_frame(2, cols=999)
    lines = run_driver(exe, "single", [fr])
    assert "frame 0 ret -1" in lines and not [l for l in lines if l.startswith("write ")]
    assert [l for l in lines if l.startswith("survivors")] == ["survivors 0 1 2 3 4"]
    for l in lines:
        if l.startswith("obj "):
            assert l.split()[2:8] == ["-1", "0", "-1", "-2", "-3", "-4"]      # mCountMappoint, bOnEdge and the planted rect as they were
        if l.startswith("list "):
            assert l.split()[2:] == []
    assert [l for l in lines if l.startswith("views")] == ["views"]


def test_several_frames_in_one_call(exe):
    frames = [small_frame(3), small_frame(4, n_kp=31, n_box=3), SC.scenes()["frame_without_boxes"][0], small_frame(5, n_kp=17, n_box=7)]
    lines = run_driver(exe, "batch", frames)
    assert lines[0].startswith("call frames 4 ") and len([l for l in lines if l.startswith("call ")]) == 1
    sent = [l for l in lines if l.startswith("sent ")]
    assert len(sent) == 4
    assert lines[5] == "ret %d" % sum(sum(1 for k in range(len(fr["boxes"])) if k % 3 != 1) for fr in frames)
    starts = [i for i, l in enumerate(lines) if l.startswith("frame ")] + [len(lines)]
    assert [lines[i] for i in starts[:-1]] == ["frame %d" % f for f in range(4)]
    for f, fr in enumerate(frames):
        check_frame(fr, lines[starts[f] + 1:starts[f + 1]], sent[f])
