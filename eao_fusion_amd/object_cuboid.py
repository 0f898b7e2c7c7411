"""A map object's cuboid (Object_Map::ComputeMeanAndStandard with Object_Map::UpdateObjPose, reference src/Object.cc:999-1235, :2243-2303) and the pairwise
overlap test (Object_Map::WhetherOverlap, :1954-1970) through eao_object_cuboids_batch / eao_object_cuboids / eao_object_overlaps (csrc/object_cuboid.hip): the
ctypes mirror the tests and tools/bench_object_cuboid.py use.

An object is a dict: points (n, 3) float32 = GetWorldPos() of mvpMapObjectMappoints after the erase of the bad ones; centroids (m, 3) float32 =
mObjectFrame[i]->_Pos; Ryaw (9,) float32, row-major; prev_cuboid_center (3,) float64."""
import ctypes as C

import numpy as np

from . import _lib

EMPTY, DONE = 0, 1
MAX_OBJECTS, OVERLAP_MAX_ROWS = 65535, 2048

# eao_object_cuboid_rec and eao_object_overlap_row (include/eao_fusion.h), field by field
RECORD_DTYPE = np.dtype([("status", np.int32), ("bounds_written", np.int32), ("sum_pos", np.float32, 3), ("center", np.float32, 3), ("standar", np.float32, 3),
                         ("center_standar", np.float32, 3), ("center_standar_dis", np.float32), ("bounds", np.float32, 6),
                         ("lenth", np.float32), ("width", np.float32), ("height", np.float32), ("rmax", np.float32), ("reserved", np.int32),
                         ("Twobj", np.float32, 16), ("Twobj_without_yaw", np.float32, 16), ("cuboid_center", np.float64, 3),
                         ("corners", np.float64, (8, 3)), ("corners_w", np.float64, (8, 3)), ("pose_q", np.float64, 4), ("pose_t", np.float64, 3),
                         ("pose_without_yaw_q", np.float64, 4), ("pose_without_yaw_t", np.float64, 3)])
ROW_DTYPE = np.dtype([("cuboid_center", np.float64, 3), ("lenth", np.float32), ("width", np.float32), ("height", np.float32), ("reserved", np.int32)])
assert RECORD_DTYPE.itemsize == 752 == C.sizeof(_lib.ObjectCuboidRec) and ROW_DTYPE.itemsize == 40 == C.sizeof(_lib.ObjectOverlapRow)


def _descs(objs):
    keep, descs = [], (_lib.ObjectCuboidDesc * max(len(objs), 1))()
    for k, o in enumerate(objs):
        pts, cen = np.ascontiguousarray(o["points"], np.float32).reshape(-1, 3), np.ascontiguousarray(o["centroids"], np.float32).reshape(-1, 3)
        keep.append((pts, cen))
        d = descs[k]
        d.n_points, d.n_centroids = o.get("n_points", len(pts)), o.get("n_centroids", len(cen))      # (a test overrides a count to provoke a refusal)
        d.points, d.centroids = (_lib.ptr(a) if len(a) else None for a in (pts, cen))
        d.Ryaw = (C.c_float * 9)(*np.asarray(o["Ryaw"], np.float32).reshape(9).tolist())
        d.prev_cuboid_center = (C.c_double * 3)(*np.asarray(o["prev_cuboid_center"], np.float64).reshape(3).tolist())
    return keep, descs


def _filled(n, dtype, fill):
    return np.frombuffer(bytes([fill]) * (n * np.dtype(dtype).itemsize), dtype).copy()


def object_cuboids_raw(objs, single=False, fill=0, n_obj=None):
    """(status, records (len(objs),) RECORD_DTYPE): the call's buffer as it left it, pre-filled with `fill` bytes"""
    keep, descs = _descs(objs)
    rec = _filled(max(len(objs), 1), RECORD_DTYPE, fill)
    L = _lib.load()
    st = L.eao_object_cuboids(descs, _lib.ptr(rec)) if single else L.eao_object_cuboids_batch(len(objs) if n_obj is None else n_obj, descs, _lib.ptr(rec))
    return st, rec[:len(objs)]


def object_cuboids_batch(objs):
    """One library call for all objects: (len(objs),) RECORD_DTYPE."""
    st, rec = object_cuboids_raw(objs)
    _lib.check(st)
    return rec


def object_cuboids(obj):
    """One object through eao_object_cuboids: a RECORD_DTYPE record."""
    st, rec = object_cuboids_raw([obj], single=True)
    _lib.check(st)
    return rec[0]


def rows_of(records):
    """the rows eao_object_overlaps reads, from the records of object_cuboids_batch"""
    rows = np.zeros(len(records), ROW_DTYPE)
    for k in ("cuboid_center", "lenth", "width", "height"):
        rows[k] = records[k]
    return rows


def object_overlaps_raw(rows, eligible, want_extents=True, fill=0, m=None):
    """(status, verdict (m, m) uint8, extents (m, m, 3) float32 or None): the call's buffers as it left them, pre-filled with `fill` bytes"""
    rows, eligible = np.ascontiguousarray(rows, ROW_DTYPE), np.ascontiguousarray(eligible, np.uint8)
    M = len(rows)
    assert len(eligible) == M
    verdict = _filled(max(M * M, 1), np.uint8, fill)
    extents = _filled(max(M * M * 3, 1), np.float32, fill) if want_extents else None
    st = _lib.load().eao_object_overlaps(M if m is None else m, _lib.ptr(rows) if M else None, _lib.ptr(eligible) if M else None, _lib.ptr(verdict), _lib.ptr(extents))
    return st, verdict[:M * M].reshape(M, M), None if extents is None else extents[:M * M * 3].reshape(M, M, 3)


def object_overlaps(rows, eligible, want_extents=True):
    """The verdict matrix and, where wanted, the extents (zero where the verdict is 0)."""
    st, verdict, extents = object_overlaps_raw(rows, eligible, want_extents)
    _lib.check(st)
    return verdict, extents


def set_profiling(on):
    _lib.check(_lib.load().eao_object_cuboid_set_profiling(1 if on else 0))


def last_kernel_ms():
    """Device time of k_object_cuboids and k_object_overlaps in this thread's last calls (after set_profiling(True)); -1 where not measured."""
    ms = (C.c_float * 2)()
    _lib.check(_lib.load().eao_object_cuboid_last_kernel_ms(ms))
    return float(ms[0]), float(ms[1])
