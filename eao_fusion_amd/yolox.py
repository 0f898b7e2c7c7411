"""What YOLOX::Detect does around the network (reference src/YOLOX.cc:51-62, :211-274) through the eao_yolox_* entry points (csrc/yolox.hip): the ctypes mirror the
tests and tools/bench_yolox.py use.

A frame is an (h, w, 3) uint8 array (rows may be a view into wider rows); a head output is an (anchors, 5 + classes) float32 array; an object record is the
structured dtype OBJECT (x, y, w, h, prob, label)."""
import ctypes as C

import numpy as np

from . import _lib

OBJECT = np.dtype([("x", "<f4"), ("y", "<f4"), ("w", "<f4"), ("h", "<f4"), ("prob", "<f4"), ("label", "<i4")])
STRIDES = (8, 16, 32)      # src/YOLOX.cc:238


def num_anchors(input_size):
    return sum((input_size // s) ** 2 for s in STRIDES)


def default_cfg():
    c = _lib.YoloxCfg()
    _lib.load().eao_yolox_cfg_default(C.byref(c))
    return c


def _frames(frames):
    """a list of equally sized frames or one (batch, h, w, 3) array -> (array whose rows are `stride` bytes apart, w, h, stride, frame_stride, batch)"""
    a = np.asarray(frames) if not isinstance(frames, np.ndarray) else frames
    if a.ndim == 3:
        a = a[None]
    assert a.ndim == 4 and a.shape[3] == 3 and a.dtype == np.uint8 and a.strides[3] == 1 and a.strides[2] == 3, "frames: (batch, h, w, 3) uint8, pixels contiguous"
    return a, a.shape[2], a.shape[1], a.strides[1], a.strides[0], a.shape[0]


class Yolox:
    def __init__(self, input_size=None, num_classes=None, conf_thresh=None, nms_thresh=None, max_proposals=None, max_batch=None):
        c = default_cfg()
        for k, v in dict(input_size=input_size, num_classes=num_classes, conf_thresh=conf_thresh, nms_thresh=nms_thresh, max_proposals=max_proposals,
                         max_batch=max_batch).items():
            if v is not None:
                setattr(c, k, v)
        self.cfg = c
        self._h = C.c_void_p()
        _lib.check(_lib.load().eao_yolox_create(C.byref(c), C.byref(self._h)))
        self.S, self.A, self.row = c.input_size, num_anchors(c.input_size), 5 + c.num_classes

    def close(self):
        if self._h:
            _lib.load().eao_yolox_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- pre-processing
    def preprocess(self, frames, rgb=False, want_gray=False, gray=None):
        """eao_yolox_preprocess: the blobs (batch, 3, S, S) and, where wanted, the grey images (batch, h, w).  gray: an array to write into instead."""
        a, w, h, stride, fs, batch = _frames(frames)
        if want_gray and gray is None:
            gray = np.zeros((batch, h, w), np.uint8)
        _lib.check(_lib.load().eao_yolox_preprocess(self._h, a.ctypes.data, w, h, stride, fs, batch, 1 if rgb else 0, _lib.ptr(gray), 0 if gray is None else gray.strides[1]))
        blobs = np.stack([self.blob(f) for f in range(batch)])
        return (blobs, gray) if gray is not None else blobs

    def blob(self, frame=0):
        out = np.zeros((3, self.S, self.S), np.float32)
        _lib.check(_lib.load().eao_yolox_blob(self._h, frame, out.ctypes.data))
        return out

    def preprocess_device(self, d_frames, width, height, stride, frame_stride, batch, rgb, d_blob, d_gray=None, gray_stride=0, stream=None):
        """eao_yolox_preprocess_device over raw device addresses (ints)"""
        _lib.check(_lib.load().eao_yolox_preprocess_device(self._h, d_frames, width, height, stride, frame_stride, batch, 1 if rgb else 0, d_blob, d_gray, gray_stride, stream))

    def buffers(self):
        """(d_blob, d_prob, stream) of the handle, as ints"""
        b, p, s = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _lib.check(_lib.load().eao_yolox_buffers(self._h, C.byref(b), C.byref(p), C.byref(s)))
        return b.value, p.value, s.value

    # ---- decode
    def _decode(self, fn, prob_ptr, batch, sizes, cap, out, tail):
        cap = self.cfg.max_proposals if cap is None else cap
        iw = np.ascontiguousarray([s[0] for s in sizes], np.int32)
        ih = np.ascontiguousarray([s[1] for s in sizes], np.int32)
        objs = np.zeros((batch, cap), OBJECT) if out is None else out["objects"]
        n, npr, nt = (np.zeros(batch, np.int32) for _ in range(3)) if out is None else (out["n"], out["n_proposals"], out["n_tied"])
        st = fn(self._h, prob_ptr, batch, _lib.ptr(iw), _lib.ptr(ih), objs.ctypes.data, cap, _lib.ptr(n), _lib.ptr(npr), _lib.ptr(nt), *tail)
        res = dict(status=st, objects=objs, n=n, n_proposals=npr, n_tied=nt)
        return res

    def decode_raw(self, heads, sizes, cap=None, out=None):
        """eao_yolox_decode without raising: dict(status, objects (batch, cap), n, n_proposals, n_tied); out: arrays to write into (to see what a refusal leaves)"""
        p = np.ascontiguousarray(heads, np.float32).reshape(-1, self.A, self.row)
        return self._decode(_lib.load().eao_yolox_decode, p.ctypes.data, len(p), sizes, cap, out, ())

    def decode_device_raw(self, d_prob, batch, sizes, cap=None, out=None, stream=None):
        return self._decode(_lib.load().eao_yolox_decode_device, d_prob, batch, sizes, cap, out, (stream,))

    def decode(self, heads, sizes, cap=None):
        """a list of dict(objects, n_proposals, n_tied) per frame; raises on any status but EAO_OK"""
        r = self.decode_raw(heads, sizes, cap)
        _lib.check(r["status"])
        return [dict(objects=r["objects"][f, :r["n"][f]].copy(), n_proposals=int(r["n_proposals"][f]), n_tied=int(r["n_tied"][f])) for f in range(len(r["n"]))]

    def decode_device(self, d_prob, batch, sizes, cap=None, stream=None):
        r = self.decode_device_raw(d_prob, batch, sizes, cap, None, stream)
        _lib.check(r["status"])
        return [dict(objects=r["objects"][f, :r["n"][f]].copy(), n_proposals=int(r["n_proposals"][f]), n_tied=int(r["n_tied"][f])) for f in range(len(r["n"]))]

    def proposals(self, frame=0):
        n = C.c_int32()
        _lib.check(_lib.load().eao_yolox_proposals(self._h, frame, None, 0, C.byref(n)))
        out = np.zeros(max(n.value, 1), OBJECT)
        _lib.check(_lib.load().eao_yolox_proposals(self._h, frame, out.ctypes.data, len(out), C.byref(n)))
        return out[:n.value]

    # ---- diagnostics
    def set_profiling(self, on):
        _lib.check(_lib.load().eao_yolox_set_profiling(self._h, 1 if on else 0))

    def last_kernel_ms(self):
        """(k_yolox_pre, k_yolox_proposals, k_yolox_rank, k_yolox_mask, k_yolox_scan) in ms, -1 where not measured"""
        ms = (C.c_float * 5)()
        _lib.check(_lib.load().eao_yolox_last_kernel_ms(self._h, ms))
        return tuple(float(v) for v in ms)
