"""The map's plane boundaries resident on the device and the plane association over them, through eao_plane_map_* (csrc/plane_map.hip,
csrc/plane_map_internal.h): Map::AssociatePlanesByBoundary and Map::SearchMatchedPlanes (reference src/Map.cc:155-292), MapPlane::MapPlane /
UpdateBoundary / SetWorldPos (src/MapPlane.cc:34-37, :137-153)."""
import ctypes as C

import numpy as np

from . import _lib

DIS_TH = 0.2        # Map::mfDisTh, src/Map.cc:22
ANGLE_TH = 0.8      # Map::mfAngleTh, src/Map.cc:23
NO_DISTANCE = 100.0  # PointDistanceFromPlane's initial value, src/Map.cc:219
MAX_ROWS, MAX_POINTS, MAX_CANDIDATES = 2048, 1 << 20, 1 << 16
CHUNK = 512         # points of one workgroup of the distance kernel (csrc/plane_map_internal.h kChunk)


def _f32(a, shape):
    return None if a is None else np.ascontiguousarray(a, np.float32).reshape(shape)


class PlaneMap:
    def __init__(self):
        self.h = C.c_void_p()
        self._lib = _lib.load()
        _lib.check(self._lib.eao_plane_map_create(C.byref(self.h)))

    def add(self, plane_id, world_pos, xyz, Tcw=None):
        """MapPlane::MapPlane: xyz (n, 3) in the camera frame of Tcw (4x4), or in the world frame when Tcw is None"""
        w, p, T = _f32(world_pos, 4), _f32(xyz, (-1, 3)), _f32(Tcw, 16)
        _lib.check(self._lib.eao_plane_map_add(self.h, int(plane_id), _lib.ptr(w), len(p), _lib.ptr(p), _lib.ptr(T)))

    def update_boundary(self, plane_id, xyz, Tcw=None):
        p, T = _f32(xyz, (-1, 3)), _f32(Tcw, 16)
        _lib.check(self._lib.eao_plane_map_update_boundary(self.h, int(plane_id), len(p), _lib.ptr(p), _lib.ptr(T)))

    def add_from_seg(self, plane_id, world_pos, seg, plane, Tcw=None):
        """add() with the cloud of kept plane `plane` of a plane_seg.PlaneSegmenter's last run, device to device"""
        w, T = _f32(world_pos, 4), _f32(Tcw, 16)
        _lib.check(self._lib.eao_plane_map_add_from_seg(self.h, int(plane_id), _lib.ptr(w), seg.h, int(plane), _lib.ptr(T)))

    def update_boundary_from_seg(self, plane_id, seg, plane, Tcw=None):
        T = _f32(Tcw, 16)
        _lib.check(self._lib.eao_plane_map_update_boundary_from_seg(self.h, int(plane_id), seg.h, int(plane), _lib.ptr(T)))

    def set_world_pos(self, plane_id, world_pos):
        w = _f32(world_pos, 4)
        _lib.check(self._lib.eao_plane_map_set_world_pos(self.h, int(plane_id), _lib.ptr(w)))

    def erase(self, plane_id):
        _lib.check(self._lib.eao_plane_map_erase(self.h, int(plane_id)))

    def clear(self):
        _lib.check(self._lib.eao_plane_map_clear(self.h))

    def info(self):
        """dict(n_live, n_points_in_use, arena_capacity) (eao_plane_map_info)"""
        n, w, c = C.c_int32(0), C.c_int64(0), C.c_int64(0)
        _lib.check(self._lib.eao_plane_map_info(self.h, C.byref(n), C.byref(w), C.byref(c)))
        return dict(n_live=int(n.value), n_points_in_use=int(w.value), arena_capacity=int(c.value))

    def boundary(self, plane_id):
        """(xyz (n, 3) f32 in the world frame, world_pos (4,) f32) as resident"""
        n = C.c_int32(0)
        _lib.check(self._lib.eao_plane_map_boundary(self.h, int(plane_id), 0, None, C.byref(n), None))
        cap = int(n.value)
        xyz, w = np.zeros((max(cap, 1), 3), np.float32), np.zeros(4, np.float32)
        _lib.check(self._lib.eao_plane_map_boundary(self.h, int(plane_id), cap, _lib.ptr(xyz), C.byref(n), _lib.ptr(w)))
        return xyz[:int(n.value)].copy(), w

    def associate(self, M, coef, cand_id=None, set_start=None, dis_th=DIS_TH, angle_th=ANGLE_TH, full=False):
        """M: (4, 4) or (n_sets, 4, 4); coef: (rows, 4); set_start: CSR over coef (one set by default); cand_id: ids in the caller's order, None = every live
        plane in add order.  dict(match i32, match_dis f32[, world_coef (rows, 4), dis (rows, n_cand), gated (rows, n_cand) u8 when full])"""
        M = _f32(M, (-1, 16))
        coef = _f32(coef, (-1, 4))
        rows = len(coef)
        start = np.ascontiguousarray([0, rows] if set_start is None else set_start, np.int32).reshape(-1)
        assert len(start) == len(M) + 1
        if cand_id is None:
            cand, n_cand = None, self.info()["n_live"]
        else:
            cand = np.ascontiguousarray(cand_id, np.uint64).reshape(-1)
            n_cand = len(cand)
        match, mdis = np.zeros(max(rows, 1), np.int32), np.zeros(max(rows, 1), np.float32)
        wc = np.zeros((max(rows, 1), 4), np.float32) if full else None
        dis = np.zeros((max(rows, 1), max(n_cand, 1)), np.float32) if full else None
        gated = np.zeros((max(rows, 1), max(n_cand, 1)), np.uint8) if full else None
        _lib.check(self._lib.eao_plane_map_associate(self.h, len(M), _lib.ptr(M), _lib.ptr(start), _lib.ptr(coef), n_cand, _lib.ptr(cand), float(dis_th),
                                                     float(angle_th), _lib.ptr(match), _lib.ptr(mdis), _lib.ptr(wc), _lib.ptr(dis), _lib.ptr(gated)))
        out = dict(match=match[:rows].copy(), match_dis=mdis[:rows].copy())
        if full:
            out.update(world_coef=wc[:rows].copy(), dis=dis.reshape(-1)[:rows * n_cand].reshape(rows, n_cand).copy(),
                       gated=gated.reshape(-1)[:rows * n_cand].reshape(rows, n_cand).copy())
        return out

    def __del__(self):
        try:
            if self.h:
                self._lib.eao_plane_map_destroy(self.h)
                self.h = None
        except Exception:
            pass
