"""The object-cuboid entry points at the drop-in boundary, without a device: the header declares them, the shared object exports them, the ctypes table binds
them, the three structs have in C the layout the ctypes mirror and the numpy records assume (a C program prints its offsets), the header's bounds are the
internal header's, every refusal comes before the device is asked for and leaves the outputs untouched, and nothing is computed without a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["eao_object_cuboids_batch", "eao_object_cuboids", "eao_object_overlaps", "eao_object_cuboid_set_profiling", "eao_object_cuboid_last_kernel_ms"]
DESC = ["n_points", "points", "n_centroids", "centroids", "Ryaw", "prev_cuboid_center"]
RECORD = ["status", "bounds_written", "sum_pos", "center", "standar", "center_standar", "center_standar_dis", "bounds", "lenth", "width", "height", "rmax", "reserved",
          "Twobj", "Twobj_without_yaw", "cuboid_center", "corners", "corners_w", "pose_q", "pose_t", "pose_without_yaw_q", "pose_without_yaw_t"]
ROW = ["cuboid_center", "lenth", "width", "height", "reserved"]


@pytest.fixture(scope="module")
def built():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "eao_fusion_amd", "csrc")])
    from eao_fusion_amd import _lib
    return _lib


def test_symbols_declared_exported_and_bound(built):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "eao_fusion.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(eao_object_(?:cuboid|overlap)[a-z0-9_]*)\s*\(", hdr)) == set(NAMES)
    L = built.load()
    for name in NAMES:
        assert hasattr(L, name) and built.SYMBOLS[name] is not None, name
    assert "object_cuboid.hip" in open(os.path.join(ROOT, "eao_fusion_amd", "csrc", "Makefile")).read()


def test_record_layouts_c_against_ctypes(built, tmp_path):
    src = tmp_path / "layout.c"
    lines = ["#include <stddef.h>", "#include <stdio.h>", "#include <eao_fusion.h>", "int main(void) {"]
    for struct, fields in (("eao_object_cuboid_desc", DESC), ("eao_object_cuboid_rec", RECORD), ("eao_object_overlap_row", ROW)):
        lines.append('    printf("%s %%zu", sizeof(%s));' % (struct, struct))
        for f in fields:
            lines.append('    printf(" %s:%%zu:%%zu", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (f, struct, f, struct, f))
        lines.append('    printf("\\n");')
    lines += ["    return 0;", "}"]
    src.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])      # (the header is C)
    got = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.strip().split("\n")
    for line, (ct, fields) in zip(got, ((built.ObjectCuboidDesc, DESC), (built.ObjectCuboidRec, RECORD), (built.ObjectOverlapRow, ROW))):
        assert [f for f, _ in ct._fields_] == fields
        want = "%s %d" % (line.split()[0], C.sizeof(ct)) + "".join(" %s:%d:%d" % (f, getattr(ct, f).offset, getattr(ct, f).size) for f in fields)
        assert line == want
    from eao_fusion_amd import object_cuboid
    assert object_cuboid.RECORD_DTYPE.itemsize == C.sizeof(built.ObjectCuboidRec) == 752 and object_cuboid.ROW_DTYPE.itemsize == C.sizeof(built.ObjectOverlapRow) == 40
    assert [object_cuboid.RECORD_DTYPE.fields[f][1] for f in RECORD] == [getattr(built.ObjectCuboidRec, f).offset for f in RECORD]
    assert [object_cuboid.ROW_DTYPE.fields[f][1] for f in ROW] == [getattr(built.ObjectOverlapRow, f).offset for f in ROW]
    import object_cuboid_reference as Y
    assert Y.RECORD_DTYPE == object_cuboid.RECORD_DTYPE and Y.ROW_DTYPE == object_cuboid.ROW_DTYPE
    assert (Y.EMPTY, Y.DONE) == (object_cuboid.EMPTY, object_cuboid.DONE)


def test_bounds(built):
    from eao_fusion_amd import object_cuboid
    hdr = open(os.path.join(ROOT, "include", "eao_fusion.h")).read()
    assert "#define EAO_OBJECT_CUBOID_MAX_OBJECTS %d\n" % object_cuboid.MAX_OBJECTS in hdr and "#define EAO_OBJECT_OVERLAP_MAX_ROWS %d\n" % object_cuboid.OVERLAP_MAX_ROWS in hdr
    assert "#define EAO_OBJECT_CUBOID_EMPTY %d\n" % object_cuboid.EMPTY in hdr and "#define EAO_OBJECT_CUBOID_DONE %d\n" % object_cuboid.DONE in hdr
    h = open(os.path.join(ROOT, "eao_fusion_amd", "csrc", "object_cuboid_internal.h")).read()
    assert "kMaxObjects = EAO_OBJECT_CUBOID_MAX_OBJECTS, kMaxOverlapRows = EAO_OBJECT_OVERLAP_MAX_ROWS;" in h


def untouched(*arrays):
    return all(set(np.ascontiguousarray(a).tobytes()) <= {0xAB} for a in arrays if a is not None)


def refusals():
    """(objects, keyword arguments of object_cuboids_raw) of every refusal"""
    import object_cuboid_scenes as SC
    scenes = SC.scenes()
    base = scenes["n63_m5"]

    def edit(key, at, value, **more):
        o = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in base.items()}
        if key:
            o[key][at] = value
        o.update(more)
        return o

    good = scenes["m4"]
    return [([good, edit("points", (5, 2), np.nan)], {}), ([edit("points", (0, 0), np.inf), good], {}), ([edit("centroids", (1, 1), -np.inf)], {}),
            ([edit("Ryaw", 8, np.nan)], {}), ([good, good, edit("prev_cuboid_center", 0, np.inf)], {}),
            ([edit(None, None, None, n_points=-1)], {}), ([edit(None, None, None, n_centroids=-7)], {}),
            ([dict(base, points=np.zeros((0, 3), np.float32), n_points=3)], {}),            # a null pointer where the count is positive
            ([dict(base, centroids=np.zeros((0, 3), np.float32), n_centroids=1)], {}),
            ([good], dict(n_obj=-1)), ([good], dict(n_obj=65536))]


def test_arguments_are_checked_before_the_device_is_asked_for(built):
    from eao_fusion_amd import object_cuboid
    for objs, kw in refusals():
        st, rec = object_cuboid.object_cuboids_raw(objs, fill=0xAB, **kw)
        assert st == built.EAO_ERR_INVALID and untouched(rec), (kw, built.load().eao_last_error())
    L = built.load()
    rec = object_cuboid._filled(1, object_cuboid.RECORD_DTYPE, 0xAB)
    assert L.eao_object_cuboids(None, built.ptr(rec)) == built.EAO_ERR_INVALID and untouched(rec)
    desc = built.ObjectCuboidDesc()
    assert L.eao_object_cuboids(C.byref(desc), None) == built.EAO_ERR_INVALID
    assert L.eao_object_cuboids_batch(1, None, built.ptr(rec)) == built.EAO_ERR_INVALID and untouched(rec)
    assert L.eao_object_cuboids_batch(0, None, None) == built.EAO_OK      # no objects: no device work
    # the overlap matrix
    import object_cuboid_scenes as SC
    rows, eligible = SC.overlap_scenes()["ineligible_row"]
    bad = rows.copy()
    bad["cuboid_center"][1, 2] = np.nan
    st, v, e = object_cuboid.object_overlaps_raw(bad, eligible, fill=0xAB)
    assert st == built.EAO_ERR_INVALID and untouched(v, e)
    bad = rows.copy()
    bad["width"][0] = np.inf
    st, v, e = object_cuboid.object_overlaps_raw(bad, eligible, fill=0xAB)
    assert st == built.EAO_ERR_INVALID and untouched(v, e)
    for m in (-1, object_cuboid.OVERLAP_MAX_ROWS + 1):
        st, v, e = object_cuboid.object_overlaps_raw(rows, eligible, fill=0xAB, m=m)
        assert st == built.EAO_ERR_INVALID and untouched(v, e)
    v = object_cuboid._filled(9, np.uint8, 0xAB)
    assert L.eao_object_overlaps(3, None, built.ptr(eligible), built.ptr(v), None) == built.EAO_ERR_INVALID and untouched(v)
    assert L.eao_object_overlaps(3, built.ptr(rows), None, built.ptr(v), None) == built.EAO_ERR_INVALID and untouched(v)
    assert L.eao_object_overlaps(3, built.ptr(rows), built.ptr(eligible), None, None) == built.EAO_ERR_INVALID
    assert L.eao_object_overlaps(0, None, None, None, None) == built.EAO_OK
    assert L.eao_object_cuboid_last_kernel_ms(None) == built.EAO_ERR_INVALID


def test_nothing_is_computed_without_a_device(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    import object_cuboid_scenes as SC
    from eao_fusion_amd import object_cuboid
    st, rec = object_cuboid.object_cuboids_raw([SC.scenes()["m4"]], fill=0xAB)
    assert st == built.EAO_ERR_NO_DEVICE and untouched(rec)
    rows, eligible = SC.overlap_scenes()["inside"]
    st, v, e = object_cuboid.object_overlaps_raw(rows, eligible, fill=0xAB)
    assert st == built.EAO_ERR_NO_DEVICE and untouched(v, e)
    ms = (C.c_float * 2)()
    assert built.load().eao_object_cuboid_last_kernel_ms(ms) == built.EAO_ERR_INVALID
