"""The class surface include/eaofusion/MapPlanes.h without a device: compiled with g++ over the stand-in Map / Frame / KeyFrame / MapPlane of
tests/cpp/map_planes/map_planes_driver.cpp and linked with map_planes_stub.cpp, which prints every library call and answers by a made-up rule (row i matches
candidate n_cand - 1 - (i / 2) % n_cand when i is even, nothing when i is odd).  Checked: what each hook sends and that it fires once; the candidate order handed
over (the std::set's for AssociatePlanesByBoundary -- the planes' addresses, not their ids --, the vector's for SearchMatchedPlanes, an id twice); the matrices
row-major and untransposed; mvpMapPlanes, mbNewPlane and vpMatched written exactly as upstream's loops write them (src/Map.cc:160, :200, :210-214, :253, :286)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TH = "th 0.200000003 0.800000012 optional 0 0 0"      # mfDisTh, mfAngleTh as floats; only match and match_dis are asked for


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("map_planes") / "map_planes_surface")
    src = os.path.join(ROOT, "tests", "cpp", "map_planes")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(src, "map_planes_driver.cpp"),
                           os.path.join(src, "map_planes_stub.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout.strip().split("\n")


def test_hooks_fire_once_each_with_upstreams_arguments(lines):
    assert lines[0] == "create"
    # MapPlane::MapPlane: Pos, pRefKF->mvBoundaryPoints[idx] (x y z of each point; the colour stays behind), pRefKF->GetPose() row-major
    assert lines[1] == "add 7 w 0 0 1 -0 n 2 xyz 1 2 3 4 5 6 T 1 0.125 0 0.25 0 1 0 0.5 0 0 1 0.75 0 0 0 1"
    assert lines[2].startswith("add 7 ") and lines[3] == "threw eao_plane_map_add: stub"      # a refused call throws
    # MapPlane::UpdateBoundary: pF.mvBoundaryPoints[id] with pF.mTcw; an empty cloud goes through
    assert lines[4] == "update 7 n 1 xyz 7 8 9 T 1 0.125 0 0.5 0 1 0 1 0 0 1 1.5 0 0 0 1"
    assert lines[5] == "update 7 n 0 xyz T 1 0.125 0 0.5 0 1 0 1 0 0 1 1.5 0 0 0 1"
    assert lines[6] == "setw 7 w 1 0 0 -2"
    assert lines[-3:] == ["erase 7", "clear", "destroy"]
    for verb, count in (("create", 1), ("add", 2), ("update", 2), ("setw", 1), ("erase", 1), ("clear", 1), ("destroy", 1), ("associate", 5)):
        assert sum(ln.split()[0] == verb for ln in lines) == count, verb


def test_associate_planes_by_boundary(lines):
    call = "associate sets 1 start 0 3 M 1 0.125 0 0.5 0 1 0 1 0 0 1 1.5 0 0 0 1 coef 0 0 1 1 0 1 0 2 1 0 0 3 cand 7 3 9 5 " + TH
    assert lines[7] == call      # mTcw as it is; the set's order (the array the planes live in), not ascending ids
    # rows 0 and 2 matched candidates 3 and 2; row 1 matched nothing and KEEPS what its slot held (upstream writes a slot only on a match), so no slot is null
    assert lines[8] == "frame 5 99 9" and lines[9] == "new 0"      # mbNewPlane was true before the call: it is reset first (:160)
    assert lines[10] == call and lines[11] == "frame 5 - 9" and lines[12] == "new 1"


def test_search_matched_planes_and_the_batch(lines):
    one = "associate sets 1 start 0 2 M 2 0.125 0 1 0 2 0 2 0 0 2 3 0 0 0 1 coef 0 0 1 4 0 0 -1 5 cand 9 7 9 " + TH
    assert lines[13] == one      # Scw with its scale, the vector's order with plane 9 twice
    assert lines[14] == "matched 9 -"      # vpMatched is rebuilt with mnPlaneNum null entries (:253): the four stale ones are gone
    assert lines[15].endswith("coef 0 0 1 4 0 0 -1 5 cand " + TH) and lines[16] == "matched - -"
    assert lines[17] == ("associate sets 3 start 0 2 2 3 M 2 0.125 0 1 0 2 0 2 0 0 2 3 0 0 0 1 3 0.125 0 1 0 3 0 2 0 0 3 3 0 0 0 1 4 0.125 0 1 0 4 0 2 0 0 4 3 0 0 0 1 "
                         "coef 0 0 1 4 0 0 -1 5 0 1 0 6 cand 9 7 9 " + TH)
    assert lines[18:21] == ["batch 9 -", "batch", "batch 7"]      # row 2 of the call is the third keyframe's row 0
    assert len(lines) == 24
