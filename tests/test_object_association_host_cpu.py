"""The host half of the device data association (eao_fusion_amd/csrc/object_assoc_internal.h) without a device: tools/object_association_walk.cpp -- the plan of
a pair, a brute-force count in the kernel's form, the decision, the projection, the clamps and the float -> int conversion -- is built with
g++ -fsanitize=address,undefined and run as a program of its own.  On every scene it must print what the yardstick (tests/object_association_reference.py,
the literal transcription) computes: m, n, step, the nine counts, w and r bit for bit, the verdict; u and v bit for bit, the rect and its status."""
import os
import subprocess

import numpy as np
import pytest

import object_association_reference as Y
import object_association_scenes as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NP_SCENES, RECT_SCENES = SC.np_scenes(), SC.rect_scenes()
CAM = ("fx", "fy", "cx", "cy", "cols", "rows")


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("object_association") / "object_association_walk")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tools", "object_association_walk.cpp"), "-o", exe])
    return exe


def hx(a):
    return " ".join("%08x" % v for v in np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32))


def run_walk(walk, script):
    out = subprocess.run([walk], input=script, capture_output=True, text=True)
    assert out.returncode == 0, "exit %d\n%s" % (out.returncode, out.stderr[-3000:])
    return out.stdout.strip().split("\n") if out.stdout.strip() else []


def np_line(det, mp, S):
    return ("np %d %d %s %d %s" % (S, len(det), hx(det), len(mp), hx(mp))).replace("  ", " ") + "\n"


def check_np(lines, want):
    assert lines[0] == "mns %d %d %d" % (want["m"], want["n"], want["step"])
    assert lines[1] == "counts " + " ".join(str(int(c)) for c in want["counts"])
    assert lines[2] == "w " + hx(want["w"]) and lines[3] == "r " + hx(want["r"])
    assert lines[4] == "verdict %d" % want["verdict"]


@pytest.mark.parametrize("name", sorted(NP_SCENES))
def test_rank_sum_scene(walk, name):
    s = NP_SCENES[name]
    check_np(run_walk(walk, np_line(s["det"], s["map"], s["S"])), Y.np_literal(s["det"], s["map"], s["S"]))


def rect_line(s):
    return ("rect %d %d %s %s %d %s" % (s["cols"], s["rows"], hx([s["fx"], s["fy"], s["cx"], s["cy"]]), hx(s["Tcw"]), len(s["points"]), hx(s["points"]))).rstrip() + "\n"


@pytest.mark.parametrize("name", sorted(RECT_SCENES))
def test_rect_scene(walk, name):
    s = RECT_SCENES[name]
    st, rect, uv = Y.rect_literal(s["points"], s["Tcw"], **{k: s[k] for k in CAM})
    got = run_walk(walk, rect_line(s))
    assert got[0] == "status %d" % st
    if st == Y.RECT_OK:
        assert got[1] == "rect %d %d %d %d" % tuple(int(v) for v in rect)
    assert got[-1] == ("uv " + hx(uv)).rstrip() and len(got) == (3 if st == Y.RECT_OK else 2)


def test_random_small_pairs(walk):
    """two hundred small pairs with ties, bad points and every early return, in one run of the program"""
    rs = np.random.RandomState(7)
    cases = []
    for _ in range(200):
        m, k = int(rs.randint(15, 40)), int(rs.randint(15, 200))
        S = k + int(rs.randint(0, 3 * k))
        q = float(rs.choice([0.0, 0.05, 0.25]))      # a grid: ties
        det, mp = rs.normal(0, 0.3, (m, 3)), rs.normal(0, 0.3, (k, 3))
        if q:
            det, mp = np.round(det / q) * q, np.round(mp / q) * q
        cases.append((det.astype(np.float32), mp.astype(np.float32), S))
    got = run_walk(walk, "".join(np_line(*c) for c in cases))
    assert len(got) == 5 * len(cases)
    for i, c in enumerate(cases):
        check_np(got[5 * i:5 * i + 5], Y.np_literal(*c))
