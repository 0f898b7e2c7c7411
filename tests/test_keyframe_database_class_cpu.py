"""The class surface include/eaofusion/KeyFrameDatabase.h without a device: compiled with g++ against the stand-in KeyFrame / Frame of
tests/cpp/keyframe_database/keyframe_database_driver.cpp and linked with keyframe_database_stub.cpp, which prints every library call and answers by a made-up rule.
Checked: what add passes (mnId and mBowVec in std::map order, an empty vector included), that a refused add throws and leaves the map alone, the connected ids and
minScore of a loop query, the neighbour CSR (GetBestCovisibilityKeyFrames is asked for ten and ten are sent; an entry without neighbours), the pointer order
returned -- a neighbour the database does not hold among them --, erase of a held, a foreign and an unknown keyframe, and clear."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("kfdb_class") / "keyframe_database_surface")
    src = os.path.join(ROOT, "tests", "cpp", "keyframe_database")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(src, "keyframe_database_driver.cpp"),
                           os.path.join(src, "keyframe_database_stub.cpp"), "-o", exe])
    out = subprocess.run([exe, "surface"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout.strip().split("\n")


def test_constructor_and_add(lines):
    assert lines[0] == "create n_words 50"      # voc.size()
    assert lines[1:4] == ["add 4 n 2 1:0.5 7:0.5", "add 2 n 1 7:1", "add 9 n 0"]
    assert lines[4] == "add 2 n 1 7:1" and lines[5] == "threw eao_keyframe_db_add: stub"


def test_loop_query_and_the_neighbour_csr(lines):
    # cap is the number of keyframes held: the refused add did not enter the map
    assert lines[6] == "query kind 0 id 12 min_score 0.25 cap 3 q 1:0.25 7:0.25 30:0.5 connected 2 33"
    # the stub scored 9, 2, 4: 9 has no neighbours, 2 has twelve of which ten are sent, 4 has two (33 is not held by the database)
    assert lines[7] == ("candidates kind 0 id 12 min_common 2 min_score 0.25 scored 9:0.5 2:0.625 4:0.75 start 0 0 10 12 nb 9 4 9 4 9 4 9 4 9 4 2 33 optional 0 0")
    assert lines[8] == "loop 9 4 2"      # the stub's order, as pointers
    assert lines[9] == "asked 10 10 10"


def test_relocalisation_query_erase_and_clear(lines):
    assert lines[10] == "query kind 1 id 40 min_score 0 cap 3 q 3:1 connected"
    assert lines[11].startswith("candidates kind 1 id 40 min_common 2 min_score 0 scored 9:0.5 2:0.625 4:0.75") and lines[12] == "reloc 9 4 2"
    # erase: another object with a held id and a keyframe never added do not reach the library
    assert lines[13] == "erase 2" and lines[14].startswith("query kind 1 id 40 min_score 0 cap 2")
    assert lines[15] == "candidates kind 1 id 40 min_common 2 min_score 0 scored 9:0.5 4:0.625 start 0 0 2 nb 2 33 optional 0 0"
    assert lines[16] == "reloc 2 4"      # keyframe 2 is no longer held: the pointer is the neighbour list's
    assert lines[17] == "clear" and lines[18].startswith("query kind 1 id 40 min_score 0 cap 0") and lines[19] == "reloc"
    assert lines[20] == "destroy" and len(lines) == 21
