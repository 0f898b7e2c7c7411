"""The detector network (reference src/YOLOX.cc:7-48 the engine, :331-367 DoInference) through the eao_detnet_* entry points (csrc/detnet.hip): a writer of the
model file csrc/detnet_internal.h defines, and the ctypes mirror the tests and tools/bench_detnet.py use.

A model is built op by op with `Model` and serialised with `tobytes()`; `Detnet(model_bytes, input_size, max_batch)` is the handle.  Tensors are NHWC float32;
the head output is an (anchors, 5 + classes) array per frame."""
import ctypes as C
import struct

import numpy as np

from . import _lib

MAGIC = b"EAODNET\0"
VERSION = 1
SCALED, FIXED, BLOB, HEAD, FIXED_INPUT = 0, 1, 2, 3, 4      # tensor kinds
FOCUS, CONV, MAXPOOL, UPSAMPLE2 = 0, 1, 2, 3                # op kinds
NONE, SILU, SIGMOID = 0, 1, 2                               # activations
STRIDES = (8, 16, 32)


def num_anchors(input_size):
    return sum((input_size // s) ** 2 for s in STRIDES)


class Model:
    """The writer: tensor 0 is the blob.  Channel ranges are (tensor, first channel, count) triples; `None` for the count of a whole tensor is not offered --
    the file says what it means."""

    def __init__(self, classes):
        self.classes = classes
        self.tensors = [(3, BLOB, 0, 0)]
        self.ops = []
        self.weights = []      # float32 arrays, in order
        self.n_weights = 0

    # ---- tensors
    def scaled(self, channels, downscale):
        self.tensors.append((channels, SCALED, downscale, 0))
        return len(self.tensors) - 1

    def fixed(self, channels, h, w, caller_input=False):
        self.tensors.append((channels, FIXED_INPUT if caller_input else FIXED, h, w))
        return len(self.tensors) - 1

    def head(self):
        self.tensors.append((5 + self.classes, HEAD, 0, 0))
        return len(self.tensors) - 1

    def _put(self, a):
        a = np.ascontiguousarray(a, np.float32).reshape(-1)
        off = self.n_weights
        self.weights.append(a)
        self.n_weights += a.size
        return off

    # ---- ops
    def _op(self, kind, src, dst, k=0, stride=1, act=NONE, groups=1, res=None, w_off=0, b_off=0):
        self.ops.append(dict(kind=kind, src=src[0], src_c0=src[1], src_c=src[2], dst=dst[0], dst_c0=dst[1], dst_c=dst[2], k=k, stride=stride, act=act, groups=groups,
                             res=-1 if res is None else res[0], res_c0=0 if res is None else res[1], w_off=w_off, b_off=b_off))
        return len(self.ops) - 1

    def focus(self, dst):
        return self._op(FOCUS, (0, 0, 3), dst)

    def conv(self, src, dst, weight, bias, stride=1, act=NONE, res=None, groups=1):
        """weight: (Cout, k, k, Cin) float32 -- [Cout][ky][kx][Cin]; bias: (Cout,)"""
        weight = np.asarray(weight, np.float32)
        assert weight.ndim == 4 and weight.shape[1] == weight.shape[2]
        return self._op(CONV, src, dst, k=weight.shape[1], stride=stride, act=act, groups=groups, res=res, w_off=self._put(weight), b_off=self._put(bias))

    def maxpool(self, src, dst, k):
        return self._op(MAXPOOL, src, dst, k=k)

    def upsample2(self, src, dst):
        return self._op(UPSAMPLE2, src, dst)

    # ---- the file
    def tobytes(self):
        tables = b"".join(struct.pack("<4I", *t) for t in self.tensors)
        tables += b"".join(struct.pack("<11Ii4I", o["kind"], o["src"], o["src_c0"], o["src_c"], o["dst"], o["dst_c0"], o["dst_c"], o["k"], o["stride"], o["act"],
                                       o["groups"], o["res"], o["res_c0"], o["w_off"], o["b_off"], 0) for o in self.ops)
        w_off = (40 + len(tables) + 15) // 16 * 16
        head = MAGIC + struct.pack("<4I2Q", VERSION, self.classes, len(self.tensors), len(self.ops), w_off, self.n_weights)
        body = head + tables
        body += b"\0" * (w_off - len(body))
        return body + b"".join(a.astype("<f4").tobytes() for a in self.weights)

    def shape(self, tensor, input_size):
        """(H, W, C) of an activation tensor at this input size"""
        c, kind, a, b = self.tensors[tensor]
        if kind == SCALED:
            return input_size // a, input_size // a, c
        assert kind in (FIXED, FIXED_INPUT)
        return a, b, c


class Detnet:
    def __init__(self, model, input_size, max_batch=1):
        """model: the bytes of a model file, or a path (str)"""
        self._h = C.c_void_p()
        L = _lib.load()
        if isinstance(model, str):
            _lib.check(L.eao_detnet_create_from_file(model.encode(), input_size, max_batch, C.byref(self._h)))
        else:
            buf = (C.c_char * max(len(model), 1)).from_buffer_copy(model if len(model) else b"\0")
            _lib.check(L.eao_detnet_create(C.cast(buf, C.c_void_p), len(model), input_size, max_batch, C.byref(self._h)))
        d = _lib.DetnetDesc()
        _lib.check(L.eao_detnet_info(self._h, C.byref(d)))
        self.desc = d
        self.S, self.A, self.row = d.input_size, d.anchors, 5 + d.classes

    def close(self):
        if self._h:
            _lib.load().eao_detnet_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        d = self.desc
        return {k: getattr(d, k) for k, _ in d._fields_}

    def forward_raw(self, d_blob, d_prob, batch, stream=None):
        """eao_detnet_forward over raw device addresses (ints), without raising: the status"""
        return _lib.load().eao_detnet_forward(self._h, d_blob, d_prob, batch, stream)

    def forward(self, d_blob, d_prob, batch, stream=None):
        _lib.check(self.forward_raw(d_blob, d_prob, batch, stream))

    def tensor(self, tensor, shape, frame=0):
        out = np.zeros(shape, np.float32)
        _lib.check(_lib.load().eao_detnet_tensor(self._h, tensor, frame, out.ctypes.data))
        return out

    def set_tensor(self, tensor, values, frame=0):
        v = np.ascontiguousarray(values, np.float32)
        _lib.check(_lib.load().eao_detnet_set_tensor(self._h, tensor, frame, v.ctypes.data))

    def set_profiling(self, on):
        _lib.check(_lib.load().eao_detnet_set_profiling(self._h, 1 if on else 0))

    def last_op_ms(self):
        ms = (C.c_float * self.desc.ops)()
        _lib.check(_lib.load().eao_detnet_last_op_ms(self._h, ms, self.desc.ops))
        return np.array(ms[:], np.float32)


# ---------------------------------------------------------------- the YOLOX graph (upstream's yolo_pafpn.py / yolo_head.py; names are upstream's module paths)
class _Graph:
    """Values are (tensor, first channel, channels, downscale).  params(name, cout, k, cin) -> (weight [cout][k][k][cin], bias [cout]): batch norm already folded."""

    def __init__(self, classes, params):
        self.m = Model(classes)
        self.params = params
        self.names = {}      # module path -> the value it writes

    def new(self, channels, downscale):
        return (self.m.scaled(channels, downscale), 0, channels, downscale)

    @staticmethod
    def part(v, c0, c):
        assert c0 + c <= v[2]
        return (v[0], v[1] + c0, c, v[3])

    def conv(self, name, x, cout, k, stride=1, act=SILU, dst=None, res=None):
        if dst is None:
            dst = self.new(cout, x[3] * stride)
        assert dst[2] == cout and (dst[3] is None or dst[3] == x[3] * stride)
        w, b = self.params(name, cout, k, x[2])
        self.m.conv(x[:3], dst[:3], w, b, stride=stride, act=act, res=None if res is None else res[:2])
        self.names[name] = dst
        return dst

    def bottleneck(self, name, x, shortcut, dst=None):
        y = self.conv(name + ".conv1", x, x[2], 1)
        return self.conv(name + ".conv2", y, x[2], 3, dst=dst, res=x if shortcut else None)

    def csp(self, name, x, cout, n, shortcut, dst=None):
        hidden = int(cout * 0.5)
        cat = self.new(2 * hidden, x[3])
        y = self.conv(name + ".conv1", x, hidden, 1, dst=None if n else self.part(cat, 0, hidden))
        for i in range(n):
            y = self.bottleneck("%s.m.%d" % (name, i), y, shortcut, dst=self.part(cat, 0, hidden) if i == n - 1 else None)
        self.conv(name + ".conv2", x, hidden, 1, dst=self.part(cat, hidden, hidden))
        return self.conv(name + ".conv3", cat, cout, 1, dst=dst)

    def spp(self, name, x, cout, ks=(5, 9, 13)):
        hidden = x[2] // 2
        cat = self.new(hidden * (1 + len(ks)), x[3])
        y = self.conv(name + ".conv1", x, hidden, 1, dst=self.part(cat, 0, hidden))
        for i, k in enumerate(ks):
            self.m.maxpool(y[:3], self.part(cat, hidden * (i + 1), hidden)[:3], k)
        return self.conv(name + ".conv2", cat, cout, 1)

    def upsample(self, x, dst):
        assert dst[2] == x[2] and dst[3] * 2 == x[3]
        self.m.upsample2(x[:3], dst[:3])
        return dst


def yolox_graph(depth, width, classes, params):
    """YOLOX (Focus stem, CSPDarknet with SPP, PAFPN, decoupled head) as a Model; returns (Model, names).  A concatenation is a tensor both producers write into."""
    g = _Graph(classes, params)
    bc, bd = int(width * 64), max(round(depth * 3), 1)
    c3, c4, c5 = int(256 * width), int(512 * width), int(1024 * width)
    B = "backbone.backbone."
    f = g.new(12, 2)
    g.m.focus(f[:3])
    x = g.conv(B + "stem.conv", f, bc, 3)
    x = g.conv(B + "dark2.0", x, bc * 2, 3, 2)
    x = g.csp(B + "dark2.1", x, bc * 2, bd, True)
    cat_p3, cat_p4 = g.new(2 * c3, 8), g.new(2 * c4, 16)          # [upsampled, dark3] and [upsampled, dark4]
    cat_n3, cat_n4 = g.new(2 * c3, 16), g.new(2 * c4, 32)         # [bu_conv2, fpn_out1] and [bu_conv1, fpn_out0]
    x = g.conv(B + "dark3.0", x, c3, 3, 2)
    x2 = g.csp(B + "dark3.1", x, c3, bd * 3, True, dst=g.part(cat_p3, c3, c3))
    x = g.conv(B + "dark4.0", x2, c4, 3, 2)
    x1 = g.csp(B + "dark4.1", x, c4, bd * 3, True, dst=g.part(cat_p4, c4, c4))
    x = g.conv(B + "dark5.0", x1, c5, 3, 2)
    x = g.spp(B + "dark5.1", x, c5)
    x0 = g.csp(B + "dark5.2", x, c5, bd, False)
    fpn_out0 = g.conv("backbone.lateral_conv0", x0, c4, 1, dst=g.part(cat_n4, c4, c4))
    g.upsample(fpn_out0, g.part(cat_p4, 0, c4))
    f_out0 = g.csp("backbone.C3_p4", cat_p4, c4, bd, False)
    fpn_out1 = g.conv("backbone.reduce_conv1", f_out0, c3, 1, dst=g.part(cat_n3, c3, c3))
    g.upsample(fpn_out1, g.part(cat_p3, 0, c3))
    pan_out2 = g.csp("backbone.C3_p3", cat_p3, c3, bd, False)
    g.conv("backbone.bu_conv2", pan_out2, c3, 3, 2, dst=g.part(cat_n3, 0, c3))
    pan_out1 = g.csp("backbone.C3_n3", cat_n3, c4, bd, False)
    g.conv("backbone.bu_conv1", pan_out1, c4, 3, 2, dst=g.part(cat_n4, 0, c4))
    pan_out0 = g.csp("backbone.C3_n4", cat_n4, c5, bd, False)
    hid = int(256 * width)
    head = g.m.head()
    for lvl, x in enumerate((pan_out2, pan_out1, pan_out0)):
        s = g.conv("head.stems.%d" % lvl, x, hid, 1)
        cls = g.conv("head.cls_convs.%d.1" % lvl, g.conv("head.cls_convs.%d.0" % lvl, s, hid, 3), hid, 3)
        reg = g.conv("head.reg_convs.%d.1" % lvl, g.conv("head.reg_convs.%d.0" % lvl, s, hid, 3), hid, 3)
        g.conv("head.reg_preds.%d" % lvl, reg, 4, 1, act=NONE, dst=(head, 0, 4, None))
        g.conv("head.obj_preds.%d" % lvl, reg, 1, 1, act=SIGMOID, dst=(head, 4, 1, None))
        g.conv("head.cls_preds.%d" % lvl, cls, classes, 1, act=SIGMOID, dst=(head, 5, classes, None))
    return g.m, g.names
