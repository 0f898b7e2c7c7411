"""Frame::ComputePlanesFromPEAC on the device, through eao_plane_seg_* (csrc/plane_seg.hip, csrc/plane_seg_internal.h): reference src/Frame.cc:381-460 over
include/PEAC/AHCPlaneFitter.hpp at its constructor defaults."""
import ctypes as C

import numpy as np

from . import _lib

MAX_PIXELS, MAX_WINDOW, MAX_PLANES = 1 << 22, 32, 64
FLAG_MISSING, FLAG_DISCONTINUITY = 1, 2
CFG_FIELDS = [f for f, _ in _lib.PlaneSegCfg._fields_]


def default_cfg(width, height, fx, fy, cx, cy, **overrides):
    """eao_plane_seg_cfg_default, then the overrides by field name"""
    c = _lib.PlaneSegCfg()
    _lib.load().eao_plane_seg_cfg_default(C.byref(c), int(width), int(height), float(fx), float(fy), float(cx), float(cy))
    for k, v in overrides.items():
        assert k in CFG_FIELDS, k
        setattr(c, k, v)
    return c


def cfg_from(obj):
    """a PlaneSegCfg from any object that has the fields (the yardstick's configuration)"""
    c = _lib.PlaneSegCfg()
    for k, t in _lib.PlaneSegCfg._fields_:
        setattr(c, k, int(getattr(obj, k)) if t is C.c_int32 else float(getattr(obj, k)))
    return c


class PlaneSegmenter:
    def __init__(self, cfg):
        self.cfg = cfg
        self.h = C.c_void_p()
        self._lib = _lib.load()
        _lib.check(self._lib.eao_plane_seg_create(C.byref(cfg), C.byref(self.h)))

    def run(self, depth):
        """depth: (height, width) float32; rows may be strided"""
        d = np.asarray(depth)
        assert d.dtype == np.float32 and d.ndim == 2 and d.shape == (self.cfg.height, self.cfg.width) and d.strides[1] == 4 and d.strides[0] % 4 == 0
        _lib.check(self._lib.eao_plane_seg_run(self.h, d.ctypes.data, d.strides[0] // 4))
        return self

    def set_profiling(self, on):
        _lib.check(self._lib.eao_plane_seg_set_profiling(self.h, int(bool(on))))

    def last_timing(self):
        """microseconds of the last run's stages: upload, block init + record download, host middle, membership + voxel stage"""
        us = np.zeros(4, np.float64)
        _lib.check(self._lib.eao_plane_seg_last_timing(self.h, _lib.ptr(us)))
        return us

    def info(self):
        a, b, c, d = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int32(0)
        _lib.check(self._lib.eao_plane_seg_info(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return dict(n_planes=int(a.value), n_points=int(b.value), n_blocks=int(c.value), n_claims=int(d.value))

    def planes(self):
        """list of dicts, one per extracted plane in upstream's order"""
        n = self.info()["n_planes"]
        arr = (_lib.PlaneSegPlane * max(n, 1))()
        got = C.c_int32(0)
        _lib.check(self._lib.eao_plane_seg_planes(self.h, n, arr, C.byref(got)))
        return [dict(normal=np.array(p.normal[:], np.float64), center=np.array(p.center[:], np.float64), mse=float(p.mse), curvature=float(p.curvature), N=int(p.N),
                     rid=int(p.rid), coef=np.array(p.coef[:], np.float32), kept=bool(p.kept), cloud_offset=int(p.cloud_offset), cloud_count=int(p.cloud_count),
                     n_pixels=int(p.n_pixels)) for p in arr[:int(got.value)]]

    def cloud(self, plane):
        n = C.c_int32(0)
        _lib.check(self._lib.eao_plane_seg_cloud(self.h, int(plane), 0, None, C.byref(n)))
        xyz = np.zeros((max(int(n.value), 1), 3), np.float32)
        _lib.check(self._lib.eao_plane_seg_cloud(self.h, int(plane), int(n.value), _lib.ptr(xyz), C.byref(n)))
        return xyz[:int(n.value)].copy()

    def membership(self):
        img = np.zeros((self.cfg.height, self.cfg.width), np.int32)
        _lib.check(self._lib.eao_plane_seg_membership(self.h, _lib.ptr(img)))
        return img

    def blocks(self):
        """(n_blocks, 18) float64: flag and N (two int32 in the first 8 bytes), nine sums, centre, normal, mse, curvature"""
        n = self.info()["n_blocks"]
        a = np.zeros((n, 18), np.float64)
        got = C.c_int32(0)
        _lib.check(self._lib.eao_plane_seg_blocks(self.h, n, _lib.ptr(a), C.byref(got)))
        assert got.value == n
        return a

    def middle(self):
        i = self.info()
        blk = np.zeros(i["n_blocks"], np.int32)
        n_old, n_claims = C.c_int32(0), C.c_int32(0)
        _lib.check(self._lib.eao_plane_seg_middle(self.h, None, 0, None, C.byref(n_old), 0, None, C.byref(n_claims)))
        plid, claims = np.zeros(max(n_old.value, 1), np.int32), np.zeros((max(n_claims.value, 1), 2), np.int32)
        _lib.check(self._lib.eao_plane_seg_middle(self.h, _lib.ptr(blk), n_old.value, _lib.ptr(plid), C.byref(n_old), n_claims.value, _lib.ptr(claims), C.byref(n_claims)))
        return dict(blk_map=blk, plidmap=plid[:n_old.value].copy(), claims=claims[:n_claims.value].copy())

    def __del__(self):
        try:
            if self.h:
                self._lib.eao_plane_seg_destroy(self.h)
                self.h = None
        except Exception:
            pass
