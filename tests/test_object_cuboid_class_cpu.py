"""The cuboid half of the class surface include/eaofusion/ObjectMap.h without a device: compiled with g++ over the stand-in Object_Map / MapPoint / Object_2D of
tests/cpp/object_cuboid/object_cuboid_driver.cpp and linked with object_cuboid_stub.cpp, which prints every library call it receives and answers by made-up
rules (the k-th float of object j's record is 1000 j + k + 0.5, the k-th double 1000 j + k + 0.25).  Checked: what the adapter sends (the points that are not
bad in list order, the centroids, Ryaw by upstream's expression, the previous cuboidCenter, one call for a batch); every member written on each of the three paths
(EMPTY; fewer than 5 centroids; 5 or more) and every other member left as it was; the erase of the bad points; RefineObjects' call order; the conversion policy
receiving exactly the returned Twobj matrices; OverlapMatrix over the members; a refused call."""
import os
import subprocess

import numpy as np
import pytest

import object_cuboid_reference as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def hx(a):
    return " ".join("%08x" % v for v in np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32))


def hx64(a):
    return " ".join("%016x" % v for v in np.ascontiguousarray(a, np.float64).reshape(-1).view(np.uint64))


def cloud(n, seed):
    return np.random.default_rng(seed).uniform(-2, 2, (n, 3)).astype(f32)


def stub_record(j, n, m):
    """the record the stub answers for object j of n good points and m centroids"""
    rec = np.zeros(1, Y.RECORD_DTYPE)
    raw = rec.view(np.uint8).reshape(-1)
    at = Y.RECORD_DTYPE.fields["sum_pos"][1]
    raw[at:at + 4 * 56] = (1000.0 * j + np.arange(56) + 0.5).astype(np.float32).view(np.uint8)
    at = Y.RECORD_DTYPE.fields["cuboid_center"][1]
    raw[at:at + 8 * 65] = (1000.0 * j + np.arange(65) + 0.25).astype(np.float64).view(np.uint8)
    rec["reserved"] = 0
    rec["status"] = Y.EMPTY if n == 0 else Y.DONE
    rec["bounds_written"] = int(n > 0 and m < 5)
    return rec[0]


def desc_line(points, centroids, ryaw, prev):
    return ("desc n %d m %d null %d %d ryaw %s prev %s points %s centroids %s" % (len(points), len(centroids), int(len(points) == 0), int(len(centroids) == 0), hx(ryaw),
                                                                                  hx64(prev), hx(points), hx(centroids))).replace("  ", " ").rstrip()


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("object_cuboid") / "object_cuboid_surface")
    src = os.path.join(ROOT, "tests", "cpp", "object_cuboid")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DEAOFUSION_FORCE_CV_COMPAT",
                           "-I", os.path.join(ROOT, "include"), os.path.join(src, "object_cuboid_driver.cpp"), os.path.join(src, "object_cuboid_stub.cpp"), "-pthread",
                           "-o", path])
    return path


def run_driver(exe, text):
    out = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return [ln.rstrip() for ln in out.stdout.strip().split("\n")]


def conv_lines(rec):
    return ["conv " + hx(rec["Twobj"]), "conv " + hx(rec["Twobj_without_yaw"])]


@pytest.mark.parametrize("n,m", [(12, 3), (12, 5), (12, 0), (0, 4)])
def test_single_object_every_member_on_its_path(exe, n, m):
    """the three paths: EMPTY writes the sum, the centre and the three deviations and nothing else; fewer than 5 centroids writes everything; 5 or more leaves the
    six bounds alone"""
    p, c, prev, rot = cloud(n, 40 + n), cloud(m, 50 + m), np.array([0.5, -1.25, 3.0]), (0.3, -0.2, 1.1)
    got = run_driver(exe, "cuboid single %s\n" % Y.driver_object(p, c, rot=rot, prev=prev, cls=7))
    rec = stub_record(0, n, m)
    want = ["call cuboids n_obj 1", desc_line(p, c, Y.ryaw_libm(*rot), prev)]
    if n > 0:
        want += conv_lines(rec)      # the policy receives exactly the returned matrices, pose first
    want += ["ret 0", ("kept " + " ".join(str(i) for i in range(n))).rstrip(), Y.members_line(rec, prev)]
    assert got == want
    members = got[-1].split()[1:]
    untouched = [t in (Y.SENTINEL32, Y.SENTINEL64) for t in members]
    assert sum(untouched) == {(12, 3): 0, (12, 5): 6, (12, 0): 0, (0, 4): len(members) - 9 - 3}[(n, m)]      # (EMPTY: cuboidCenter keeps what the script set)


def test_bad_points_leave_the_list_before_the_call(exe):
    p, c = cloud(9, 61), cloud(2, 62)
    bad = np.array([1, 0, 0, 1, 1, 0, 0, 0, 1], np.uint8)
    got = run_driver(exe, "cuboid single %s\n" % Y.driver_object(p, c, bad=bad))
    assert got[1] == desc_line(p[bad == 0], c, Y.ryaw_libm(0, 0, 0), np.zeros(3))
    assert got[-2] == "kept " + " ".join(str(i) for i in np.nonzero(bad == 0)[0])
    all_bad = run_driver(exe, "cuboid single %s\n" % Y.driver_object(p, c, bad=np.ones(9, np.uint8)))
    assert all_bad[1].startswith("desc n 0 m 2 null 1 0 ") and all_bad[-2] == "kept" and all_bad[-1] == Y.members_line(stub_record(0, 0, 2), np.zeros(3))


def test_ryaw_is_upstreams_expression(exe):
    """rotP = rotR = rotY = 0, the case this fork's tracker produces: the identity with -sp = -0.0f; and three angles at once"""
    got = run_driver(exe, "cuboid single %s\n" % Y.driver_object(cloud(3, 63), cloud(1, 64)))
    assert " ryaw 3f800000 00000000 00000000 00000000 3f800000 00000000 80000000 00000000 3f800000 prev " in got[1]
    rot = (2.9, -0.6, 0.75)
    got = run_driver(exe, "cuboid single %s\n" % Y.driver_object(cloud(3, 63), cloud(1, 64), rot=rot))
    assert " ryaw %s prev " % hx(Y.ryaw_libm(*rot)) in got[1]
    assert np.abs(Y.ryaw_libm(*rot) - Y.ryaw(*rot)).max() < 1e-6


def test_batch_is_one_call(exe):
    shapes = [(10, 2), (0, 3), (7, 6), (31, 5)]
    objs = [(cloud(n, 70 + j), cloud(m, 80 + j), np.array([j, -j, 0.5 * j], np.float64)) for j, (n, m) in enumerate(shapes)]
    got = run_driver(exe, "cuboid batch %d %s\n" % (len(objs), " ".join(Y.driver_object(p, c, prev=prev) for p, c, prev in objs)))
    assert [ln for ln in got if ln.startswith("call")] == ["call cuboids n_obj 4"]
    assert [ln for ln in got if ln.startswith("desc")] == [desc_line(p, c, Y.ryaw_libm(0, 0, 0), prev) for p, c, prev in objs]
    members = [ln for ln in got if ln.startswith("members")]
    assert members == [Y.members_line(stub_record(j, n, m), objs[j][2]) for j, (n, m) in enumerate(shapes)]
    assert [ln for ln in got if ln.startswith("conv")] == sum((conv_lines(stub_record(j, n, m)) for j, (n, m) in enumerate(shapes) if n), [])
    assert "ret 0" in got
    assert run_driver(exe, "cuboid batch 0\n") == ["ret 0"]      # no objects: no call


def test_refine_objects_call_order(exe):
    """the forest (and its erase), then the cuboids over what is left: :718-719.  The stub's forest flags point i when i % 4 == 1 or it is the last."""
    p30, p8 = cloud(30, 91), cloud(8, 92)
    got = run_driver(exe, "refine 1 2 %s %s\n" % (Y.driver_object(p30, cloud(2, 93)), Y.driver_object(p8, cloud(1, 94))))
    calls = [ln for ln in got if ln.startswith("call")]
    assert calls == ["call iforest n_obj 1 bi 1 start 0 30", "call cuboids n_obj 2"]      # 8 points: below the forest's gate
    keep = np.array([not (i % 4 == 1 or i == 29) for i in range(30)])
    descs = [ln for ln in got if ln.startswith("desc")]
    assert descs[0].startswith("desc n %d m 2 " % keep.sum()) and descs[0].endswith(" points %s centroids %s" % (hx(p30[keep]), hx(cloud(2, 93))))
    assert descs[1].startswith("desc n 8 m 1 ")
    assert "ret %d" % int((~keep).sum()) in got and "kept " + " ".join(str(i) for i in np.nonzero(keep)[0]) in got
    off = run_driver(exe, "refine 0 1 %s\n" % Y.driver_object(p30, cloud(2, 93)))
    assert [ln for ln in off if ln.startswith("call")] == ["call cuboids n_obj 1"] and "ret 0" in off


def test_refused_call_writes_no_member(exe):
    p = cloud(6, 95)
    p[0, 0] = 999.0
    bad = np.array([0, 1, 0, 0, 0, 0], np.uint8)
    got = run_driver(exe, "cuboid single %s\n" % Y.driver_object(p, cloud(2, 96), bad=bad))
    assert "ret -1" in got and not any(ln.startswith("conv") for ln in got)
    assert got[-2] == "kept 0 2 3 4 5"      # erased before anything is computed, as upstream
    assert set(got[-1].split()[1:]) == {Y.SENTINEL32, "0000000000000000", Y.SENTINEL64}


def test_overlap_matrix_over_the_members(exe):
    centers, scales, eligible = np.array([[0, 0, 0], [1.5, 0, 0.25], [-2, 3, 1]], np.float64), np.array([[1, 2, 3], [0.5, 0.25, 4], [2, 2, 2]], f32), [1, 0, 1]
    body = " ".join("%s %s %d" % (hx64(c), hx(s), e) for c, s, e in zip(centers, scales, eligible))
    got = run_driver(exe, "overlap 1 3 %s\n" % body)
    assert got[0] == "call overlaps m 3 extents 1 " + " ".join("row %s %s %d" % (hx64(c), hx(s), e) for c, s, e in zip(centers, scales, eligible))
    assert got[1:] == ["ret 1", "ov 001000000", "ex 0 2 " + hx(f32([2.0, 2.25, 2.5]))]
    got = run_driver(exe, "overlap 0 3 %s\n" % body)
    assert got[0].startswith("call overlaps m 3 extents 0 ") and got[1:] == ["ret 1", "ov 001000000"]
    assert run_driver(exe, "overlap 1 0\n") == ["ret 0", "ov"]
