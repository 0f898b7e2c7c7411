"""The yardstick of the chained update of a map object (tests/object_chain_reference.py) on the seeded scenes (tests/object_chain_scenes.py): every scene shows
what it claims, upstream's literal form and the device's form agree on every output, and the arithmetic the device needs in another form than the host's
(max_depth without libm, the LDS edge) is held to the host's."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import isolation_forest_reference as IF
import object_chain_reference as Y
import object_chain_scenes as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden_object_chain as GG  # noqa: E402

SCENES = SC.scenes()
NAMES = sorted(SCENES)


@pytest.fixture(scope="module")
def results():
    return {n: Y.chain(SCENES[n], "literal") for n in NAMES}


@pytest.mark.parametrize("name", NAMES)
def test_scene_shows_what_it_claims(results, name):
    d, r = SCENES[name], results[name]
    assert d["claims"], name
    for key, want in d["claims"].items():
        if key.startswith("points."):
            assert int(r["rec"][key[7:]]) == want, key
        elif key.startswith("cuboid."):
            assert int(r["cuboid"][key[7:]]) == want, key
        elif key in Y.RECORD_DTYPE.names:
            assert int(r["chain"][key]) == want, key
        elif key == "final_lacks":
            assert not (r["final"] == np.array(want)).all(axis=1).any() and (r["list"] == np.array(want)).all(axis=1).any()
        else:
            assert np.array_equal(r[key], np.array(want)), key


@pytest.mark.parametrize("name", NAMES)
def test_literal_and_device_forms_agree(results, name):
    assert Y.differences(results[name], Y.chain(SCENES[name], "device")) == []


def test_recorded_results_are_the_yardsticks(results):
    z = np.load(GG.PATH)
    assert {k.split(".")[0] for k in z.files} == set(NAMES)
    for n in NAMES:
        assert Y.differences(GG.recorded_part(results[n]), GG.unpack(z, n)) == [], n
    assert os.path.getsize(GG.PATH) < os.path.getsize(os.path.join(ROOT, "tests", "golden", "object_points", "results.npz"))


def test_the_scenes_cover_what_they_are_there_for(results):
    finals = {int(r["chain"]["n_final"]) for r in results.values() if "chain" in r}
    edge = SC.lds_edge()
    assert {0, 29, 30, 31, SC.CHUNK - 1, SC.CHUNK, SC.CHUNK + 1, edge, edge + 1} <= finals
    assert {int(r["rec"]["status"]) for r in results.values()} == {Y.OP.DONE, Y.OP.REJECTED, Y.OP.UNDEFINED}
    assert {int(r["chain"]["forest_status"]) for r in results.values() if "chain" in r} == {Y.FOREST_SKIPPED, Y.FOREST_DONE}
    assert any(int(r["chain"]["removed"]) > 0 for r in results.values() if "chain" in r)
    # the aliased entry: erased without the alias, kept with it, and nothing else differs in the list
    a, b = results["alias_raises_8_to_9"], results["alias_null_erases"]
    assert np.array_equal(a["list"], b["list"]) and a["erased"][0] == 0 and b["erased"][0] == 1
    # a non-finished update has no output behind the points record
    assert set(results["rejected"]) == {"rec"} and set(results["undefined"]) == {"rec"}
    # the first and the last survivor are the bad ones
    for n, at in (("bad_point_first", 0), ("bad_point_last", -1)):
        r = results[n]
        assert not np.array_equal(r["survivors"][at], r["final"][at]) and len(r["final"]) == len(r["survivors"]) - 1


def test_a_planted_failure_gives_the_failed_record():
    """no input is known on which upstream's Build fails: the yardstick's own finish is handed the failure"""
    pts = SC.PS.cloud(np.random.default_rng(1), 40)
    st, flags, removed, scores = Y.forest_of(pts, 0, 1, planted_failure=True)
    assert st == Y.FOREST_FAILED and not flags.any() and removed == 0 and (scores == -1.0).all()


def test_lds_edge_is_the_header_budget():
    hdr = open(os.path.join(ROOT, "eao_fusion_amd", "csrc", "iforest_internal.h")).read()
    assert int(re.search(r"kLdsBudget = (\d+);", hdr).group(1)) == SC.LDS_BUDGET
    edge = SC.lds_edge()
    assert SC.lds_bytes(edge) <= SC.LDS_BUDGET < SC.lds_bytes(edge + 1)
    assert all(SC.lds_bytes(n) <= SC.lds_bytes(n + 1) for n in range(30, 65535))      # a list below the bound fits wherever the bound does


def test_integer_max_depth_equals_the_libm_form(tmp_path):
    """max_depth_int of csrc/iforest_internal.h (what the plan kernel runs) against max_depth (ceil(log2) through libm) for every S in 1 .. 32767, in C++; and
    against the yardstick's Python form"""
    src = tmp_path / "depth.cpp"
    src.write_text('#include <cstdio>\n#include "iforest_internal.h"\nint main() {\n    int bad = 0;\n    for (uint32_t s = 1; s <= 32767; s++) {\n'
                   '        if (eao::iforest::max_depth(s) != eao::iforest::max_depth_int(s)) bad++;\n        if (s < 40 || (s & (s - 1)) == 0 || (s & (s + 1)) == 0) '
                   'std::printf("%u %u\\n", s, eao::iforest::max_depth_int(s));\n    }\n    std::printf("bad %d\\n", bad);\n    return bad != 0;\n}\n')
    exe = str(tmp_path / "depth")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-I", os.path.join(ROOT, "eao_fusion_amd", "csrc"), str(src), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-500:]
    lines = out.stdout.strip().split("\n")
    assert lines[-1] == "bad 0" and len(lines) > 50
    for line in lines[:-1]:
        s, d = (int(v) for v in line.split())
        assert d == IF.max_depth(s) == (s - 1).bit_length(), s
