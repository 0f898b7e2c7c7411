"""The object-points entry points at the drop-in boundary, without a device: the header declares them, the shared object exports them, the ctypes table binds
them, the three structs have in C the layout the ctypes mirror and the numpy record assume (a C program prints its offsets), the header's constants are the
Python mirror's and the internal header's, every refusal comes before the device is asked for and leaves the outputs untouched, and nothing is computed without
a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["eao_object_points_update_batch", "eao_object_points_update", "eao_object_points_set_profiling", "eao_object_points_last_kernel_ms"]
DESC = ["change_gate", "gate", "erase", "box_off_edge", "n_map", "n_cand", "map_points", "map_count", "cand_points", "cand_count", "Tcw", "fx", "fy", "cx", "cy", "cols", "rows",
        "project_rect1", "box_rect", "center", "rmax", "n_frames_after_push", "lenth", "width", "height", "pose_q", "pose_t", "cuboid_center", "bounds", "overlap", "sum_pos",
        "reserved", "survivors"]
RECORD = ["status", "n_gated", "n_appended", "n_list", "n_erased", "n_survivors", "rect2", "iou", "iou2", "sum_pos_appended", "sum_pos", "reserved"]
OUT = ["rec", "gate", "target", "count", "list", "erased", "survivors"]


@pytest.fixture(scope="module")
def built():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "eao_fusion_amd", "csrc")])
    from eao_fusion_amd import _lib
    return _lib


def test_symbols_declared_exported_and_bound(built):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "eao_fusion.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(eao_object_points[a-z0-9_]*)\s*\(", hdr)) == set(NAMES)
    L = built.load()
    for name in NAMES:
        assert hasattr(L, name) and built.SYMBOLS[name] is not None, name
    assert "object_points.hip" in open(os.path.join(ROOT, "eao_fusion_amd", "csrc", "Makefile")).read()


def test_record_layouts_c_against_ctypes(built, tmp_path):
    src = tmp_path / "layout.c"
    lines = ["#include <stddef.h>", "#include <stdio.h>", "#include <eao_fusion.h>", "int main(void) {"]
    for struct, fields in (("eao_object_points_desc", DESC), ("eao_object_points_rec", RECORD), ("eao_object_points_out", OUT)):
        lines.append('    printf("%s %%zu", sizeof(%s));' % (struct, struct))
        for f in fields:
            lines.append('    printf(" %s:%%zu:%%zu", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (f, struct, f, struct, f))
        lines.append('    printf("\\n");')
    lines += ["    return 0;", "}"]
    src.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])      # (the header is C)
    got = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.strip().split("\n")
    for line, (ct, fields) in zip(got, ((built.ObjectPointsDesc, DESC), (built.ObjectPointsRec, RECORD), (built.ObjectPointsOut, OUT))):
        assert [f for f, _ in ct._fields_] == fields
        want = "%s %d" % (line.split()[0], C.sizeof(ct)) + "".join(" %s:%d:%d" % (f, getattr(ct, f).offset, getattr(ct, f).size) for f in fields)
        assert line == want
    from eao_fusion_amd import object_points
    assert object_points.RECORD_DTYPE.itemsize == C.sizeof(built.ObjectPointsRec) == 80
    assert [object_points.RECORD_DTYPE.fields[f][1] for f in RECORD] == [getattr(built.ObjectPointsRec, f).offset for f in RECORD]
    import object_points_reference as Y
    assert Y.RECORD_DTYPE == object_points.RECORD_DTYPE
    assert set(Y.INTS) | set(Y.FLOATS) | {k for k, _, _ in Y.VECTORS} | {"n_map", "n_cand", "map_points", "map_count", "cand_points", "cand_count", "reserved",
                                                                           "survivors"} == set(DESC)
    assert Y.INTS == object_points.INTS and Y.FLOATS == object_points.FLOATS and [k for k, _, _ in Y.VECTORS] == list(object_points.VECTORS)


def test_constants(built):
    from eao_fusion_amd import object_points as P
    import object_points_reference as Y
    hdr = open(os.path.join(ROOT, "include", "eao_fusion.h")).read()
    for name, value in (("MAX_DESCS", P.MAX_DESCS), ("DONE", P.DONE), ("REJECTED", P.REJECTED), ("UNDEFINED", P.UNDEFINED), ("GATE_NONE", P.GATE_NONE),
                        ("GATE_RADIUS", P.GATE_RADIUS), ("GATE_CUBOID", P.GATE_CUBOID), ("ERASE_NONE", P.ERASE_NONE), ("ERASE_PROJECTION", P.ERASE_PROJECTION),
                        ("ERASE_BOX", P.ERASE_BOX), ("ERASE_SHRUNK", P.ERASE_SHRUNK)):
        assert "#define EAO_OBJECT_POINTS_%s %d\n" % (name, value) in hdr, name
        assert name == "MAX_DESCS" or getattr(Y, name) == value
    h = open(os.path.join(ROOT, "eao_fusion_amd", "csrc", "object_points_internal.h")).read()
    assert "kMaxDescs = EAO_OBJECT_POINTS_MAX_DESCS;" in h and "kMaxBatchPoints = (int64_t)1 << 27;" in h


def untouched(outs):
    return all(set(np.ascontiguousarray(a).tobytes()) <= {0xAB} for o in outs for a in o.values() if a is not None)


def refusals():
    """(descs, keyword arguments of update_raw) of every refusal that is decided before the device"""
    import object_points_scenes as SC
    scenes = SC.scenes()
    base, good = scenes["frame_M65_C3"], scenes["append_then_box"]

    def edit(key, at, value):
        o = dict(base)
        o[key] = np.array(base[key], np.float64)
        o[key][at] = value
        return o

    bad = [edit("map_points", (5, 2), np.nan), edit("cand_points", (0, 0), np.inf), edit("center", 1, np.nan), edit("sum_pos", 0, -np.inf),
           dict(base, Tcw=[np.inf] + [0.0] * 15), dict(base, fy=np.nan), dict(base, cx=np.inf), dict(base, rmax=np.nan), dict(base, lenth=np.inf), dict(base, width=np.nan),
           dict(base, pose_q=[np.nan, 0, 0, 1]), dict(base, pose_t=[0, 0, np.inf]), dict(base, cuboid_center=[0, np.nan, 0]), dict(base, bounds=[0, 1, 0, 1, np.nan, 1]),
           dict(base, overlap=[0, np.inf, 0]), dict(base, gate=3), dict(base, gate=-1), dict(base, erase=4), dict(base, cols=-1), dict(base, rows=1 << 16),
           dict(base, box_rect=[0, 0, -1, 1]), dict(base, project_rect1=[-(1 << 16), 0, 1, 1]), dict(base, n_map=-1), dict(base, n_cand=-7),
           dict(base, null=("map_points",)), dict(base, null=("map_count",)), dict(base, null=("cand_points",)), dict(base, null=("cand_count",)),
           dict(base, null=("rec",)), dict(base, null=("gate",)), dict(base, null=("target",)), dict(base, null=("count",)), dict(base, null=("list",)),
           dict(base, null=("erased",)), dict(base, null=("survivors",))]
    cases = [([good, b], {}) for b in bad[::2]] + [([b, good], {}) for b in bad[1::2]]
    return cases + [([good], dict(n=-1)), ([good], dict(n=65536))]


def test_arguments_are_checked_before_the_device_is_asked_for(built):
    from eao_fusion_amd import object_points
    for descs, kw in refusals():
        st, outs = object_points.update_raw(descs, fill=0xAB, **kw)
        assert st == built.EAO_ERR_INVALID and untouched(outs), (kw, built.load().eao_last_error())
    L = built.load()
    assert L.eao_object_points_update(None, C.byref(built.ObjectPointsOut())) == built.EAO_ERR_INVALID
    assert L.eao_object_points_update(C.byref(built.ObjectPointsDesc()), None) == built.EAO_ERR_INVALID
    assert L.eao_object_points_update_batch(1, None, C.byref(built.ObjectPointsOut())) == built.EAO_ERR_INVALID
    assert L.eao_object_points_update_batch(1, C.byref(built.ObjectPointsDesc()), None) == built.EAO_ERR_INVALID
    assert L.eao_object_points_update_batch(0, None, None) == built.EAO_OK      # no descs: no device work
    assert L.eao_object_points_last_kernel_ms(None) == built.EAO_ERR_INVALID
    # more than 2^27 points in one call: the counts alone decide, no list is read
    import object_points_scenes as SC
    big = dict(SC.scenes()["append_then_box"], n_map=1 << 27, n_cand=1)
    st, outs = object_points.update_raw([big], fill=0xAB)
    assert st == built.EAO_ERR_INVALID and untouched(outs) and b"2^27" in L.eao_last_error()
    # a missing map_count is no refusal where no erase by projection reads it
    ok = dict(SC.scenes()["append_then_box"], null=("map_count",))
    st, _ = object_points.update_raw([ok], fill=0xAB)
    assert st != built.EAO_ERR_INVALID


def test_nothing_is_computed_without_a_device(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    import object_points_scenes as SC
    from eao_fusion_amd import object_points
    st, outs = object_points.update_raw([SC.scenes()["frame_M65_C3"]], fill=0xAB)
    assert st == built.EAO_ERR_NO_DEVICE and untouched(outs)
    ms = (C.c_float * 2)()
    assert built.load().eao_object_points_last_kernel_ms(ms) == built.EAO_ERR_INVALID
