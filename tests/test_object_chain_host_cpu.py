"""The host half of the chained update (eao_fusion_amd/csrc/object_chain_internal.h over the three HIP-free headers) without a device:
tools/object_chain_walk.cpp is built with g++ -fsanitize=address,undefined and run as a program of its own.  On every scene it must print what the yardstick
(tests/object_chain_reference.py) holds: integers as integers, floats bit for bit, a NaN as a NaN.  The FAILED record of the forest, for which no input is
known, is covered by handing the host finish a planted failure word."""
import os
import subprocess

import numpy as np
import pytest

import object_chain_reference as Y
import object_chain_scenes as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = SC.scenes()
NAMES = sorted(SCENES)


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("object_chain") / "object_chain_walk")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tools", "object_chain_walk.cpp"), "-o", exe])
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


@pytest.mark.parametrize("name", NAMES)
def test_scene(lines, name):
    want = Y.chain(SCENES[name], "literal")
    drop = Y.OC.zero_sign_fields(Y.final_object(SCENES[name], want)) if "final" in want else ()
    assert Y.drop_tokens(lines[name].split(), drop) == Y.walk_tokens(SCENES[name], want, drop)


def test_a_planted_failure_gives_the_failed_record(walk):
    d = SCENES["n_final_31"]
    got = run_walk(walk, Y.walk_script(d, planted_failure=True))[0].split()
    want = Y.chain(d, "literal")
    st, flags, removed, scores = Y.forest_of(np.zeros((31, 3), np.float32), d["class_id"], d["bi_forest"], planted_failure=True)
    want["chain"]["forest_status"], want["chain"]["removed"], want["forest_flags"], want["scores"] = st, removed, flags, scores
    assert st == Y.FOREST_FAILED and got == Y.walk_tokens(d, want)
    # a desc the rules skip stays skipped whatever the word says
    d = SCENES["n_final_29"]
    assert run_walk(walk, Y.walk_script(d, planted_failure=True))[0].split() == Y.walk_tokens(d, Y.chain(d, "literal"))


def test_the_checks_in_front_of_the_entry_points(walk):
    base = SCENES["n_final_31"]
    n_map, n_cand = len(base["map_points"]), len(base["cand_points"])

    def edit(key, at, value):
        o = dict(base)
        o[key] = np.array(base[key], np.float64)
        o[key][at] = value
        return o

    cases = [(base, "accepted"), (SCENES["every_point_erased"], "accepted"), (SCENES["alias_null_erases"], "accepted"),
             (edit("map_points", (7, 1), np.nan), "refused a non-finite point"), (edit("centroids", (0, 2), np.inf), "refused a non-finite centroid"),
             (edit("Ryaw", 8, np.nan), "refused a non-finite Ryaw"), (edit("prev_cuboid_center", 0, np.inf), "refused a non-finite prev_cuboid_center"),
             (dict(base, gate=3), "refused an unknown gate"), (dict(base, cand_alias=np.full(n_cand, n_map, np.int32)), "refused an alias outside -1 .. n_map - 1"),
             (dict(base, cand_alias=np.full(n_cand, -2, np.int32)), "refused an alias outside -1 .. n_map - 1"),
             (dict(base, cand_alias=np.full(n_cand, n_map - 1, np.int32)), "accepted")]
    assert run_walk(walk, "".join(Y.walk_script(o, "refuse") for o, _ in cases)) == [want for _, want in cases]
