"""A frame's 2D objects (steps 2, 4, 5 and 6 of the object layer, reference src/Tracking.cc:1768-1973) through eao_frame_objects_batch / eao_frame_objects
(csrc/frame_objects.hip): the ctypes mirror the tests and tools/bench_frame_objects.py use.

A frame is a dict: kp_x, kp_y (n_kp,) float32 = mvKeysUn[i].pt; mp_id (n_kp,) int32, -1 where the keypoint has no good map point, equal ids = one MapPoint;
mp_xyz (n_kp, 3) float32 = GetWorldPos(); boxes (n_box, 4) int32 = {x, y, width, height} of mBoxRect; score (n_box,) float32; Tcw (4, 4) float32; fx, fy, cx,
cy; cols, rows."""
import ctypes as C

import numpy as np

from . import _lib

MAX_KEYPOINTS, MAX_BOXES = 4096, 256

# eao_frame_object_record (include/eao_fusion.h), field by field
RECORD_DTYPE = np.dtype([("n_assigned", np.int32), ("n", np.int32), ("sum_pos", np.float32, 3), ("pos", np.float32, 3), ("std", np.float32, 3),
                         ("q1", np.float32), ("q3", np.float32), ("max_th", np.float32), ("boxplot_ran", np.int32), ("center_2d", np.float32, 2),
                         ("has_feature_rect", np.int32), ("feature_rect", np.int32, 4), ("num_overlaps", np.int32), ("bad", np.int32), ("on_edge", np.int32)])
assert RECORD_DTYPE.itemsize == 100 == C.sizeof(_lib.FrameObjectRecord)


def _descs(frames):
    keep, descs = [], (_lib.FrameObjectsDesc * max(len(frames), 1))()
    for f, fr in enumerate(frames):
        kx, ky = np.ascontiguousarray(fr["kp_x"], np.float32).reshape(-1), np.ascontiguousarray(fr["kp_y"], np.float32).reshape(-1)
        ids = np.ascontiguousarray(fr["mp_id"], np.int32).reshape(-1)
        xyz = np.ascontiguousarray(fr["mp_xyz"], np.float32).reshape(-1, 3)
        boxes, score = np.ascontiguousarray(fr["boxes"], np.int32).reshape(-1, 4), np.ascontiguousarray(fr["score"], np.float32).reshape(-1)
        assert len(kx) == len(ky) == len(ids) == len(xyz) and len(boxes) == len(score)
        keep.append((kx, ky, ids, xyz, boxes, score))
        d = descs[f]
        d.n_kp, d.n_box = len(kx), len(boxes)
        d.kp_x, d.kp_y, d.mp_id, d.mp_xyz = (_lib.ptr(a) if len(a) else None for a in (kx, ky, ids, xyz))
        d.boxes, d.score = (_lib.ptr(a) if len(a) else None for a in (boxes, score))
        d.Tcw = (C.c_float * 16)(*np.asarray(fr["Tcw"], np.float32).reshape(16).tolist())
        d.fx, d.fy, d.cx, d.cy, d.cols, d.rows = fr["fx"], fr["fy"], fr["cx"], fr["cy"], fr["cols"], fr["rows"]
    return keep, descs


def _filled(n, dtype, fill):
    return np.frombuffer(bytes([fill]) * (n * np.dtype(dtype).itemsize), dtype).copy()


def frame_objects_raw(frames, assigned_cap=None, kept_cap=None, single=False, fill=0):
    """(status, records (total boxes,) RECORD_DTYPE, assigned_start, assigned, kept_start, kept): the call's buffers as it left them, pre-filled with `fill` bytes.
    The default capacities hold every list the frames can produce."""
    keep, descs = _descs(frames)
    nB = sum(len(k[4]) for k in keep)
    worst = sum(len(k[4]) * int((k[2] >= 0).sum()) for k in keep)
    ca, ck = worst if assigned_cap is None else assigned_cap, worst if kept_cap is None else kept_cap
    rec = _filled(max(nB, 1), RECORD_DTYPE, fill)
    sa, sk, la, lk = (_filled(n, np.int32, fill) for n in (nB + 1, nB + 1, max(ca, 1), max(ck, 1)))
    out = _lib.FrameObjectsOut(_lib.ptr(rec), _lib.ptr(sa), _lib.ptr(la), ca, _lib.ptr(sk), _lib.ptr(lk), ck)
    L = _lib.load()
    st = L.eao_frame_objects(descs, C.byref(out)) if single else L.eao_frame_objects_batch(len(frames), descs, C.byref(out))
    return st, rec[:nB], sa, la[:ca], sk, lk[:ck]


def frame_objects_batch(frames):
    """Per frame {records (n_box,) RECORD_DTYPE, assigned: [keypoint indices per box], kept: [..]}."""
    st, rec, sa, la, sk, lk = frame_objects_raw(frames)
    _lib.check(st)
    res, b = [], 0
    for fr in frames:
        m = len(np.asarray(fr["boxes"]).reshape(-1, 4))
        res.append(dict(records=rec[b:b + m].copy(), assigned=[la[sa[k]:sa[k + 1]].copy() for k in range(b, b + m)],
                        kept=[lk[sk[k]:sk[k + 1]].copy() for k in range(b, b + m)]))
        b += m
    return res


def frame_objects(frame):
    """One frame through eao_frame_objects."""
    st, rec, sa, la, sk, lk = frame_objects_raw([frame], single=True)
    _lib.check(st)
    m = len(rec)
    return dict(records=rec, assigned=[la[sa[k]:sa[k + 1]].copy() for k in range(m)], kept=[lk[sk[k]:sk[k + 1]].copy() for k in range(m)])


def set_profiling(on):
    _lib.check(_lib.load().eao_frame_objects_set_profiling(1 if on else 0))


def last_kernel_ms():
    """Device time of k_frame_features, k_frame_objects and k_frame_pack in this thread's last call (after set_profiling(True)); -1 where not measured."""
    ms = (C.c_float * 3)()
    _lib.check(_lib.load().eao_frame_objects_last_kernel_ms(ms))
    return float(ms[0]), float(ms[1]), float(ms[2])
