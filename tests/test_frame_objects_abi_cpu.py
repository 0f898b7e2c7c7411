"""The frame-objects entry points at the drop-in boundary, without a device: the header declares them, the shared object exports them, the ctypes table binds
them, the three structs have in C the layout the ctypes mirror and the numpy record assume (a C program prints its offsets), the header's bounds are the
internal header's, and nothing is computed without a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["eao_frame_objects_batch", "eao_frame_objects", "eao_frame_objects_set_profiling", "eao_frame_objects_last_kernel_ms"]
DESC = ["n_kp", "kp_x", "kp_y", "mp_id", "mp_xyz", "n_box", "boxes", "score", "Tcw", "fx", "fy", "cx", "cy", "cols", "rows"]
RECORD = ["n_assigned", "n", "sum_pos", "pos", "std", "q1", "q3", "max_th", "boxplot_ran", "center_2d", "has_feature_rect", "feature_rect", "num_overlaps", "bad",
          "on_edge"]
OUT = ["records", "assigned_start", "assigned", "assigned_cap", "kept_start", "kept", "kept_cap"]


@pytest.fixture(scope="module")
def built():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "eao_fusion_amd", "csrc")])
    from eao_fusion_amd import _lib
    return _lib


def test_symbols_declared_exported_and_bound(built):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "eao_fusion.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(eao_frame_objects[a-z0-9_]*)\s*\(", hdr)) == set(NAMES)
    L = built.load()
    for name in NAMES:
        assert hasattr(L, name) and built.SYMBOLS[name] is not None, name


def test_record_layouts_c_against_ctypes(built, tmp_path):
    src = tmp_path / "layout.c"
    lines = ["#include <stddef.h>", "#include <stdio.h>", "#include <eao_fusion.h>", "int main(void) {"]
    for struct, fields in (("eao_frame_objects_desc", DESC), ("eao_frame_object_record", RECORD), ("eao_frame_objects_out", OUT)):
        lines.append('    printf("%s %%zu", sizeof(%s));' % (struct, struct))
        for f in fields:
            lines.append('    printf(" %s:%%zu:%%zu", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (f, struct, f, struct, f))
        lines.append('    printf("\\n");')
    lines += ["    return 0;", "}"]
    src.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])      # (the header is C)
    got = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.strip().split("\n")
    for line, (ct, fields) in zip(got, ((built.FrameObjectsDesc, DESC), (built.FrameObjectRecord, RECORD), (built.FrameObjectsOut, OUT))):
        assert [f for f, _ in ct._fields_] == fields
        want = "%s %d" % (line.split()[0], C.sizeof(ct)) + "".join(" %s:%d:%d" % (f, getattr(ct, f).offset, getattr(ct, f).size) for f in fields)
        assert line == want
    from eao_fusion_amd import frame_objects
    assert frame_objects.RECORD_DTYPE.itemsize == C.sizeof(built.FrameObjectRecord) == 100
    assert [frame_objects.RECORD_DTYPE.fields[f][1] for f in RECORD] == [getattr(built.FrameObjectRecord, f).offset for f in RECORD]
    import frame_objects_reference as Y
    assert Y.RECORD_DTYPE == frame_objects.RECORD_DTYPE


def test_bounds(built):
    from eao_fusion_amd import frame_objects
    hdr = open(os.path.join(ROOT, "include", "eao_fusion.h")).read()
    assert "#define EAO_FRAME_OBJECTS_MAX_KEYPOINTS %d\n" % frame_objects.MAX_KEYPOINTS in hdr and "#define EAO_FRAME_OBJECTS_MAX_BOXES %d\n" % frame_objects.MAX_BOXES in hdr
    h = open(os.path.join(ROOT, "eao_fusion_amd", "csrc", "frame_objects_internal.h")).read()
    assert "kMaxKeypoints = EAO_FRAME_OBJECTS_MAX_KEYPOINTS, kMaxBoxes = EAO_FRAME_OBJECTS_MAX_BOXES;" in h


def test_arguments_are_checked_before_the_device_is_asked_for(built):
    import frame_objects_scenes as SC
    from eao_fusion_amd import frame_objects
    scenes = SC.scenes()
    bad = dict(scenes["box_edges"][0])
    bad["mp_id"] = np.full(len(bad["kp_x"]), -2, np.int32)
    raw = frame_objects.frame_objects_raw([bad], fill=0xAB)
    assert raw[0] == built.EAO_ERR_INVALID and all(set(np.ascontiguousarray(a).tobytes()) <= {0xAB} for a in raw[1:])      # before the device is asked for
    st, rec, sa, la, sk, lk = frame_objects.frame_objects_raw([scenes["frame_without_boxes"][0]], fill=0xAB)
    assert st == built.EAO_OK and sa.tolist() == [0] and sk.tolist() == [0]      # no boxes: no device work
    # more frames than one call takes (zeroed descriptors are valid empty frames)
    starts = np.full(2, 7, np.int32)
    out = built.FrameObjectsOut(None, built.ptr(starts), None, 0, built.ptr(starts), None, 0)
    many = (built.FrameObjectsDesc * 65536)()
    assert built.load().eao_frame_objects_batch(65536, many, C.byref(out)) == built.EAO_ERR_INVALID and starts.tolist() == [7, 7]
    assert built.load().eao_frame_objects_batch(65535, many, C.byref(out)) == built.EAO_OK and starts.tolist() == [0, 7]
    assert "#define EAO_FRAME_OBJECTS_MAX_FRAMES 65535\n" in open(os.path.join(ROOT, "include", "eao_fusion.h")).read()


def test_nothing_is_computed_without_a_device(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    import frame_objects_scenes as SC
    from eao_fusion_amd import frame_objects
    raw = frame_objects.frame_objects_raw([SC.scenes()["box_edges"][0]], fill=0xAB)
    assert raw[0] == built.EAO_ERR_NO_DEVICE and all(set(np.ascontiguousarray(a).tobytes()) <= {0xAB} for a in raw[1:])
    ms = (C.c_float * 3)()
    assert built.load().eao_frame_objects_last_kernel_ms(ms) == built.EAO_ERR_INVALID
