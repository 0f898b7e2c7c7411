"""The host header of the point-list update (eao_fusion_amd/csrc/object_points_internal.h) without a device: tools/object_points_walk.cpp -- upstream's literal
form and the checks in front of the entry points -- is built with g++ -fsanitize=address,undefined and run as a program of its own.  On every scene it must
print what the yardstick (tests/object_points_reference.py) and the recorded results hold: integers as integers, floats bit for bit, a NaN as a NaN."""
import os
import subprocess
import sys

import numpy as np
import pytest

import object_points_reference as Y
import object_points_scenes as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden_object_points as GG  # noqa: E402

SCENES = SC.scenes()
NAMES = sorted(SCENES)


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("object_points") / "object_points_walk")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tools", "object_points_walk.cpp"), "-o", exe])
    return exe


def run_walk(walk, script):
    out = subprocess.run([walk], input=script, capture_output=True, text=True)
    assert out.returncode == 0, "exit %d\n%s" % (out.returncode, out.stderr[-3000:])
    return out.stdout.strip().split("\n") if out.stdout.strip() else []


@pytest.fixture(scope="module")
def lines(walk):
    """every scene in one run of the program"""
    got = run_walk(walk, "".join(Y.walk_script(SCENES[name]) for name in NAMES))
    assert len(got) == len(NAMES)
    return dict(zip(NAMES, got))


@pytest.fixture(scope="module")
def gold():
    return np.load(GG.PATH)


@pytest.mark.parametrize("name", NAMES)
def test_scene(lines, gold, name):
    res, _variant = GG.unpack(gold, name)
    assert lines[name].split() == Y.walk_line(res).split()
    assert lines[name].split() == Y.walk_line(Y.literal(SCENES[name])).split()


def test_the_checks_in_front_of_the_entry_points(walk):
    base = SCENES["frame_M65_C3"]

    def edit(key, at, value):
        o = dict(base)
        if at is None:
            o[key] = value
        else:
            o[key] = np.array(base[key], np.float64)
            o[key][at] = value
        return o

    cases = [(base, "accepted"), (SCENES["nothing_at_all"], "accepted"), (SCENES["empty_list"], "accepted"), (SCENES["empty_candidates"], "accepted"),
             (edit("map_points", (7, 1), np.nan), "refused a non-finite point"), (edit("cand_points", (2, 2), -np.inf), "refused a non-finite candidate"),
             (dict(base, Tcw=[np.nan] + [0.0] * 15), "refused a non-finite Tcw"), (edit("fx", None, np.inf), "refused a non-finite intrinsic"),
             (edit("center", 0, np.nan), "refused a non-finite center"), (edit("rmax", None, np.inf), "refused a non-finite rmax"),
             (edit("height", None, np.nan), "refused a non-finite extent"), (dict(base, pose_q=[0, 0, np.nan, 1]), "refused a non-finite pose"),
             (dict(base, pose_t=[0, np.inf, 0]), "refused a non-finite pose"), (dict(base, cuboid_center=[np.nan, 0, 0]), "refused a non-finite cuboid_center"),
             (dict(base, bounds=[0, 1, 0, np.inf, 0, 1]), "refused a non-finite bound"), (dict(base, overlap=[np.nan, 0, 0]), "refused a non-finite overlap"),
             (edit("sum_pos", 2, np.inf), "refused a non-finite sum_pos"), (dict(base, gate=3), "refused an unknown gate"), (dict(base, erase=-1), "refused an unknown erase"),
             (dict(base, cols=-1), "refused cols or rows out of range"), (dict(base, rows=(1 << 15) + 1), "refused cols or rows out of range"),
             (dict(base, box_rect=[0, 0, -1, 5]), "refused a rect out of range"), (dict(base, project_rect1=[1 << 16, 0, 1, 1]), "refused a rect out of range"),
             (edit("map_points", (0, 0), np.finfo(np.float32).max), "accepted")]
    got = run_walk(walk, "".join(Y.walk_script(o, "refuse") for o, _ in cases))
    assert got == [want for _, want in cases]
    neg = Y.walk_script(SCENES["nothing_at_all"], "refuse").split()
    neg[8] = "-1"      # n_map
    assert run_walk(walk, " ".join(neg) + "\n") == ["refused a negative count"]
    neg[8], neg[9] = "0", "-4"
    assert run_walk(walk, " ".join(neg) + "\n") == ["refused a negative count"]
