"""The object layer's per-frame data association (Tracking step 10): Object_2D::NoParaDataAssociation (reference src/Object.cc:728-962) through
eao_object_np_counts_batch / eao_object_np_association_batch and Object_Map::ComputeProjectRectFrame (:1606-1651) through eao_object_project_rects_batch
(csrc/object_assoc.hip): the ctypes mirror the tests and tools/bench_object_association.py use.

A detection or a map object is an (n, 3) float32 array of its GOOD map points' world positions in vector order; map_total[j] is the map object's
mvpMapObjectMappoints.size() with the bad points (default: the list's length).  pairs: (detection index, map object index) per test."""
import ctypes as C

import numpy as np

from . import _lib

UNDEFINED = 3
RECT_EMPTY, RECT_OK, RECT_UNDEFINED = 0, 1, 2


def _pack(lists):
    pts = [np.ascontiguousarray(o, np.float32).reshape(-1, 3) for o in lists]
    start = np.zeros(len(pts) + 1, np.int32)
    start[1:] = np.cumsum([len(p) for p in pts])
    xyz = np.ascontiguousarray(np.concatenate(pts) if pts else np.zeros((0, 3), np.float32), np.float32)
    if len(xyz) == 0:
        xyz = np.zeros((1, 3), np.float32)
    return start, xyz


def _lists(dets, maps, map_total, pairs):
    ds, dx = _pack(dets)
    ms, mx = _pack(maps)
    tot = np.ascontiguousarray([len(m) for m in maps] if map_total is None else map_total, np.int32).reshape(len(maps))
    pr = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    pd, pm = np.ascontiguousarray(pr[:, 0]), np.ascontiguousarray(pr[:, 1])
    keep = (ds, dx, ms, mx, tot, pd, pm)
    return keep, (len(dets), _lib.ptr(ds), _lib.ptr(dx), len(maps), _lib.ptr(ms), _lib.ptr(mx), _lib.ptr(tot), len(pr), _lib.ptr(pd), _lib.ptr(pm)), len(pr)


def np_counts(dets, maps, pairs, map_total=None):
    """(mns (P, 3) int32 = m, n, step; counts (P, 9) uint32 = x12 x21 x00 y12 .. z00) per pair."""
    keep, args, P = _lists(dets, maps, map_total, pairs)
    mns, counts = np.zeros((max(P, 1), 3), np.int32), np.zeros((max(P, 1), 9), np.uint32)
    _lib.check(_lib.load().eao_object_np_counts_batch(*args, _lib.ptr(mns), _lib.ptr(counts)))
    return mns[:P], counts[:P]


def np_association(dets, maps, pairs, map_total=None):
    """(verdict (P,) int32: 0 / 1 / 2 as upstream, 3 = undefined upstream; w (P, 3) float32; r (P, 2) float32) per pair."""
    keep, args, P = _lists(dets, maps, map_total, pairs)
    verdict, w, r = np.zeros(max(P, 1), np.int32), np.zeros((max(P, 1), 3), np.float32), np.zeros((max(P, 1), 2), np.float32)
    _lib.check(_lib.load().eao_object_np_association_batch(*args, _lib.ptr(verdict), _lib.ptr(w), _lib.ptr(r)))
    return verdict[:P], w[:P], r[:P]


def no_para_data_association(det, map_obj, map_total=None):
    """Object_2D::NoParaDataAssociation over one pair: upstream's return value (or UNDEFINED)."""
    return int(np_association([det], [map_obj], [(0, 0)], None if map_total is None else [map_total])[0][0])


def project_rects(maps, Tcw, fx, fy, cx, cy, cols, rows, want_uv=False):
    """Object_Map::ComputeProjectRectFrame per object under one pose: (rect (n, 4) int32 = x, y, width, height -- rows of objects whose status is not RECT_OK are
    left at -1 --, status (n,) uint8[, uv list of (k, 2) float32])."""
    n = len(maps)
    start, xyz = _pack(maps)
    T = np.ascontiguousarray(Tcw, np.float32).reshape(16)
    rect, status = np.full((max(n, 1), 4), -1, np.int32), np.zeros(max(n, 1), np.uint8)
    uv = np.zeros((max(int(start[-1]), 1), 2), np.float32) if want_uv else None
    _lib.check(_lib.load().eao_object_project_rects_batch(n, _lib.ptr(start), _lib.ptr(xyz), _lib.ptr(T), fx, fy, cx, cy, cols, rows, _lib.ptr(rect), _lib.ptr(status),
                                                          _lib.ptr(uv)))
    if want_uv:
        return rect[:n], status[:n], [uv[start[j]:start[j + 1]].copy() for j in range(n)]
    return rect[:n], status[:n]


def set_profiling(on):
    _lib.check(_lib.load().eao_object_assoc_set_profiling(1 if on else 0))


def last_kernel_ms():
    """Device time of k_np_counts and k_project_rects in this thread's last calls (after set_profiling(True)); -1 for a kernel that has not run since."""
    ms = (C.c_float * 2)()
    _lib.check(_lib.load().eao_object_assoc_last_kernel_ms(ms))
    return float(ms[0]), float(ms[1])
