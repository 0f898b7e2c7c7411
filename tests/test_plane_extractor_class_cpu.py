"""The class surface include/eaofusion/PlaneExtractor.h without a device: compiled with g++ over the stand-in Frame / MapPlane of
tests/cpp/plane_extractor/plane_extractor_driver.cpp and linked with plane_extractor_stub.cpp, which prints every library call and answers by a made-up rule
(three planes; plane i has coef (i, 10 + i, 20 + i, 30 + i) and a cloud of i + 1 points; plane 1 is not kept; a negative first pixel is refused).  Checked: the
configuration and the image handed over (the view's stride, not its width), one handle per geometry, plane_num_ / mvPlaneCoefficients / mvBoundaryPoints /
mvPlanePoints written as upstream writes them (src/Frame.cc:410, :447-455), the frame-plane to handle-plane index of the MapPlane hooks, and what throws."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = "T 1 0.125 0 1 0 1 0 2 0 0 1 3 0 0 0 1"
RUN = ["run stride 48 first 1 last 2.43100023", "planes cap 0 count", "planes cap 3 table", "cloud 0 cap 1", "cloud 2 cap 3"]
KEPT = "[4 x 1: 0 10 20 30] [4 x 1: 2 12 22 32] boundary ( 0 0.25 0.5 ) ( 200 200.25 200.5 201 201.25 201.5 202 202.25 202.5 ) points 1 3"


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plane_extractor") / "plane_extractor_surface")
    src = os.path.join(ROOT, "tests", "cpp", "plane_extractor")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(src, "plane_extractor_driver.cpp"),
                           os.path.join(src, "plane_extractor_stub.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout.strip().split("\n")


def test_a_frame_is_filled_as_upstream_fills_it(lines):
    # the Frame's statics and the image's size; the constructor defaults come from the library, nothing is configured (plane_filter never is upstream)
    assert lines[0:2] == ["cfg_default 40 30 500 501 20.5 15.25", "create 40 30 window 10 min_support 3000"]
    # the 40 x 30 view of a 48-wide image goes over with the stride of 48; the cloud of the plane that was not kept is never asked for
    assert lines[2:7] == RUN
    # plane_num_ counts every extracted plane (:410); only kept planes reach the three vectors (:447-455), the cloud in both, x y z only
    assert lines[7] == "frame plane_num_ 3 coef " + KEPT
    # a second frame of the same geometry: no second handle; what the frame's vectors held stays in front (upstream appends)
    assert lines[8:13] == RUN and lines[13] == "frame plane_num_ 3 coef [4 x 1: 0 0 0 0] " + KEPT
    assert sum(ln.startswith("create") for ln in lines[:14]) == 1


def test_map_plane_hooks_take_the_cloud_from_the_handle(lines):
    # frame plane 1 is the handle's plane 2; Pos and the pose row-major and untransposed
    assert lines[14] == "add_from_seg 7 plane 2 seg 40 w 0.5 1 1.5 2 " + T
    assert lines[15] == "update_from_seg 7 plane 0 seg 40 " + T
    assert lines[16] == "threw PlaneExtractor: the handle no longer holds that frame's clouds"      # frame 41: the extractor ran frame 42 since
    assert lines[17] == "threw PlaneExtractor: no such frame plane"
    assert lines[18].startswith("add_from_seg 666 plane 0 ") and lines[19] == "threw eao_plane_map_add_from_seg: stub"


def test_failures_and_geometry_changes(lines):
    # a refused run throws, writes nothing into the frame and leaves the extractor without a frame
    assert lines[20:24] == ["run stride 48 first -1 last 2.43100023", "threw eao_plane_seg_run: stub", "frame plane_num_ -1 coef boundary points", "holds 0 0"]
    # another image size: a new handle first, then the old one goes
    assert lines[24:28] == ["cfg_default 30 20 500 501 20.5 15.25", "create 30 20 window 10 min_support 3000", "destroy 40", "run stride 30 first 2 last 2"]
    assert lines[32] == "threw PlaneExtractor: imDepth must be a CV_32F image" and lines[33] == "destroy 30"
    # the free function runs the calling thread's extractor, which leaves with the thread
    assert lines[34:36] == ["cfg_default 40 30 500 501 20.5 15.25", "create 40 30 window 10 min_support 3000"]
    assert lines[-2:] == ["free plane_num_ 3 kept 2", "destroy 40"] and len(lines) == 43
