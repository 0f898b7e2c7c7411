"""The update of a map object's point list (the change gate, the append and the erase of Object_Map::DataAssociateUpdate, reference src/Object.cc:1352-1601; the
append of MergeTwoMapObjs, :1766-1821; the erases of BigToSmall and DivideEquallyTwoObjs, :2070-2120) through eao_object_points_update_batch /
eao_object_points_update (csrc/object_points.hip): the ctypes mirror the tests and tools/bench_object_points.py use.

A desc is a dict.  map_points (n_map, 3) and cand_points (n_cand, 3) float32, map_count and cand_count int32 are its lists; every other key is the field of
eao_object_points_desc of the same name and defaults to zero (Tcw to the identity, pose_q to the unit quaternion)."""
import ctypes as C

import numpy as np

from . import _lib

DONE, REJECTED, UNDEFINED = 1, 2, 3
GATE_NONE, GATE_RADIUS, GATE_CUBOID = 0, 1, 2
ERASE_NONE, ERASE_PROJECTION, ERASE_BOX, ERASE_SHRUNK = 0, 1, 2, 3
MAX_DESCS = 65535

# eao_object_points_rec (include/eao_fusion.h), field by field
RECORD_DTYPE = np.dtype([("status", np.int32), ("n_gated", np.int32), ("n_appended", np.int32), ("n_list", np.int32), ("n_erased", np.int32), ("n_survivors", np.int32),
                         ("rect2", np.int32, 4), ("iou", np.float32), ("iou2", np.float32), ("sum_pos_appended", np.float32, 3), ("sum_pos", np.float32, 3),
                         ("reserved", np.int32, 2)])
assert RECORD_DTYPE.itemsize == 80 == C.sizeof(_lib.ObjectPointsRec)

INTS = ["change_gate", "gate", "erase", "box_off_edge", "cols", "rows", "n_frames_after_push"]
FLOATS = ["fx", "fy", "cx", "cy", "rmax", "lenth", "width", "height"]
VECTORS = {"Tcw": (C.c_float, 16, np.float32), "project_rect1": (C.c_int32, 4, np.int32), "box_rect": (C.c_int32, 4, np.int32), "center": (C.c_float, 3, np.float32),
           "pose_q": (C.c_double, 4, np.float64), "pose_t": (C.c_double, 3, np.float64), "cuboid_center": (C.c_double, 3, np.float64),
           "bounds": (C.c_float, 6, np.float32), "overlap": (C.c_float, 3, np.float32), "sum_pos": (C.c_float, 3, np.float32)}
DEFAULTS = {"Tcw": np.eye(4, dtype=np.float32).reshape(16), "pose_q": np.array([0.0, 0.0, 0.0, 1.0])}


def _filled(n, dtype, fill):
    return np.frombuffer(bytes([fill]) * (n * np.dtype(dtype).itemsize), dtype).copy()


def lists_of(d):
    """(map_points, map_count, cand_points, cand_count) of a desc, contiguous; a missing count list is zeros"""
    mp, cp = np.ascontiguousarray(d["map_points"], np.float32).reshape(-1, 3), np.ascontiguousarray(d["cand_points"], np.float32).reshape(-1, 3)
    mc = np.ascontiguousarray(d["map_count"] if d.get("map_count") is not None else np.zeros(len(mp)), np.int32).reshape(-1)
    cc = np.ascontiguousarray(d["cand_count"] if d.get("cand_count") is not None else np.zeros(len(cp)), np.int32).reshape(-1)
    return mp, mc, cp, cc


def fill_desc(c, o, d, fill, want_points):
    """one eao_object_points_desc `c` and eao_object_points_out `o` from the dict d; returns the numpy buffers behind them.  An `n_map` / `n_cand` / `null` key
    overrides what the lists say (a test provokes a refusal)"""
    mp, mc, cp, cc = lists_of(d)
    M, Cn = len(mp), len(cp)
    for f in INTS:
        setattr(c, f, int(d.get(f, 0)))
    for f in FLOATS:
        setattr(c, f, float(np.float32(d.get(f, 0.0))))
    for f, (ct, n, dt) in VECTORS.items():
        setattr(c, f, (ct * n)(*np.asarray(d.get(f, DEFAULTS.get(f, np.zeros(n))), dt).reshape(n).tolist()))
    c.n_map, c.n_cand = d.get("n_map", M), d.get("n_cand", Cn)
    null = d.get("null", ())
    c.map_points = _lib.ptr(mp) if M and "map_points" not in null else None
    c.map_count = _lib.ptr(mc) if M and "map_count" not in null else None
    c.cand_points = _lib.ptr(cp) if Cn and "cand_points" not in null else None
    c.cand_count = _lib.ptr(cc) if Cn and "cand_count" not in null else None
    out = dict(rec=_filled(1, RECORD_DTYPE, fill), gate=_filled(max(Cn, 1), np.uint8, fill), target=_filled(max(Cn, 1), np.int32, fill),
               count=_filled(max(Cn, 1), np.int32, fill), list=_filled(2 * max(M + Cn, 1), np.int32, fill), erased=_filled(max(M + Cn, 1), np.uint8, fill),
               survivors=_filled(2 * max(M + Cn, 1), np.int32, fill), points=_filled(3 * max(M + Cn, 1), np.float32, fill) if want_points else None)
    c.survivors = _lib.ptr(out["points"])
    for f in ("rec", "gate", "target", "count", "list", "erased", "survivors"):
        setattr(o, f, None if f in null else _lib.ptr(out[f]))
    return mp, mc, cp, cc, out


def _descs(descs, fill, want_points):
    """the C arrays of a batch and the numpy buffers behind them"""
    keep, cd, co = [], (_lib.ObjectPointsDesc * max(len(descs), 1))(), (_lib.ObjectPointsOut * max(len(descs), 1))()
    for k, d in enumerate(descs):
        keep.append(fill_desc(cd[k], co[k], d, fill, want_points))
    return keep, cd, co


def update_raw(descs, single=False, fill=0, n=None, want_points=True):
    """(status, [the output buffers of each desc as the call left them, pre-filled with `fill` bytes])"""
    keep, cd, co = _descs(descs, fill, want_points)
    L = _lib.load()
    st = L.eao_object_points_update(cd, co) if single else L.eao_object_points_update_batch(len(descs) if n is None else n, cd, co)
    return st, [k[4] for k in keep]


def trim(desc, out):
    """the written part of a desc's output buffers: a dict of rec (a RECORD_DTYPE record) and, with status DONE, gate, target, count (n_cand), list, erased
    (n_list), survivors, points (n_survivors)"""
    rec = out["rec"][0]
    res = dict(rec=rec)
    if rec["status"] != DONE:
        return res
    C_ = len(lists_of(desc)[2])
    nl, ns = int(rec["n_list"]), int(rec["n_survivors"])
    res.update(gate=out["gate"][:C_], target=out["target"][:C_], count=out["count"][:C_], list=out["list"][:2 * nl].reshape(-1, 2), erased=out["erased"][:nl],
               survivors=out["survivors"][:2 * ns].reshape(-1, 2))
    if out["points"] is not None:
        res["points"] = out["points"][:3 * ns].reshape(-1, 3)
    return res


def update_batch(descs):
    """One library call for all descs: a list of trim()med results."""
    st, outs = update_raw(descs)
    _lib.check(st)
    return [trim(d, o) for d, o in zip(descs, outs)]


def update(desc):
    """One desc through eao_object_points_update."""
    st, outs = update_raw([desc], single=True)
    _lib.check(st)
    return trim(desc, outs[0])


def set_profiling(on):
    _lib.check(_lib.load().eao_object_points_set_profiling(1 if on else 0))


def last_kernel_ms():
    """Device time of k_object_points_match and of k_object_points (or k_object_points_finish) in this thread's last call (after set_profiling(True)); -1 where
    not measured."""
    ms = (C.c_float * 2)()
    _lib.check(_lib.load().eao_object_points_last_kernel_ms(ms))
    return float(ms[0]), float(ms[1])
