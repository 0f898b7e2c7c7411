"""The host header of a map object's cuboid (eao_fusion_amd/csrc/object_cuboid_internal.h) without a device: tools/object_cuboid_walk.cpp -- upstream's literal
form, the checks in front of the entry points, the overlap matrix -- is built with g++ -fsanitize=address,undefined and run as a program of its own.  On every
scene it must print what the yardstick (tests/object_cuboid_reference.py) and the recorded results hold: integers as integers, floats and doubles bit for bit, a
NaN as a NaN; the zeros of the fields tests/test_object_cuboid_reference_cpu.py names lose their signs on both sides (std::sort decides them here)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import object_cuboid_reference as Y
import object_cuboid_scenes as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden_object_cuboid as GG  # noqa: E402

SCENES = SC.scenes()
NAMES = sorted(SCENES)
OVERLAPS = SC.overlap_scenes()


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("object_cuboid") / "object_cuboid_walk")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tools", "object_cuboid_walk.cpp"), "-o", exe])
    return exe


def run_walk(walk, script):
    out = subprocess.run([walk], input=script, capture_output=True, text=True)
    assert out.returncode == 0, "exit %d\n%s" % (out.returncode, out.stderr[-3000:])
    return out.stdout.strip().split("\n") if out.stdout.strip() else []


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "object_cuboid", "results.npz"))


@pytest.mark.parametrize("name", NAMES)
def test_scene(walk, gold, name):
    rec, _variant, drop = GG.unpack(gold, name)
    got = run_walk(walk, Y.walk_script(SCENES[name]))
    assert len(got) == 1
    assert Y.drop_line(got[0], drop) == Y.walk_line(rec, drop)
    assert Y.drop_line(got[0], drop) == Y.walk_line(Y.literal(SCENES[name]), drop)


@pytest.mark.parametrize("name", sorted(OVERLAPS))
def test_overlaps(walk, gold, name):
    rows, eligible = OVERLAPS[name]
    assert run_walk(walk, Y.overlap_script(rows, eligible)) == Y.overlap_lines(*GG.unpack_overlaps(gold, name))


def test_the_checks_in_front_of_the_entry_points(walk):
    base = SCENES["n63_m5"]

    def edit(key, at, value):
        o = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in base.items()}
        o[key][at] = value
        return o

    cases = [(base, "accepted"), (SCENES["n0_m0"], "accepted"), (SCENES["empty_with_centroids"], "accepted"), (SCENES["squares_overflow"], "accepted"),
             (edit("points", (7, 1), np.nan), "refused a non-finite point"), (edit("points", (62, 2), -np.inf), "refused a non-finite point"),
             (edit("centroids", (4, 0), np.inf), "refused a non-finite centroid"), (edit("Ryaw", 5, np.nan), "refused a non-finite Ryaw"),
             (edit("prev_cuboid_center", 2, np.inf), "refused a non-finite prev_cuboid_center"),
             (edit("points", (0, 0), np.finfo(np.float32).max), "accepted")]
    got = run_walk(walk, "".join(Y.walk_script(o, "refuse") for o, _ in cases))
    assert got == [want for _, want in cases]
    assert run_walk(walk, "refuse -1 0 %s %s\n" % (" ".join(["3f800000"] * 9), " ".join(["0" * 16] * 3))) == ["refused a negative count"]
    assert run_walk(walk, "refuse 0 -3 %s %s\n" % (" ".join(["3f800000"] * 9), " ".join(["0" * 16] * 3))) == ["refused a negative count"]
