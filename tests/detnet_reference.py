"""The numpy yardstick of the detector network: the arithmetic of eao_fusion_amd/csrc/detnet_internal.h restated, vectorised over the output elements and never
over K -- every output element is one accumulator that takes its taps in the order ky, kx, ci.

Python 3.10 has no math.fma.  fmaf(x, w, a) is emulated through float64: x * w is exact there (48 significant bits), the sum is rounded to ODD (the float64 sum
with its last bit set when it was inexact) and then to float32.  Rounding to odd keeps the sticky information the second rounding needs, so the result is the
single rounding of the exact x * w + a (Boldo and Melquiond, "Emulation of a FMA and correctly rounded sums", 2008: 53 >= 24 + 2 bits suffice).  Plain double
rounding (fma_double_rounding below) fails where the float64 sum lands on a float32 midpoint; tests/test_detnet_reference_cpu.py plants such cases."""
import numpy as np

F = np.float32
NONE, SILU, SIGMOID = 0, 1, 2
CANONICAL_NAN = np.array([0x7fc00000], np.uint32).view(np.float32)[0]


def fma(x, w, a):
    """fmaf over float32 arrays (broadcast), bit for bit"""
    x, w, a = np.asarray(x, F), np.asarray(w, F), np.asarray(a, F)
    with np.errstate(all="ignore"):
        p = x.astype(np.float64) * w.astype(np.float64)      # exact
        b = a.astype(np.float64)
        s = p + b
        bb = s - p
        err = (p - (s - bb)) + (b - bb)                      # 2Sum: s + err == p + b exactly, where all are finite
        fin = np.isfinite(s) & np.isfinite(err)
        even = (s.view(np.int64) & 1) == 0
        fix = fin & (err != 0) & even
        toward = np.where(err > 0, np.inf, -np.inf)
        s = np.where(fix, np.nextafter(s, toward), s)        # the neighbour on the side of the exact sum: its last bit is set
        return s.astype(F)


def fma_double_rounding(x, w, a):
    """what the emulation must NOT be: the float64 sum rounded to nearest, then rounded again"""
    with np.errstate(all="ignore"):
        return (np.asarray(x, F).astype(np.float64) * np.asarray(w, F).astype(np.float64) + np.asarray(a, F).astype(np.float64)).astype(F)


_EXP_COEF = (1.1470745597729725e-11, 1.6059043836821613e-10, 2.08767569878681e-09, 2.505210838544172e-08, 2.755731922398589e-07, 2.7557319223985893e-06,
             2.48015873015873e-05, 1.984126984126984e-04, 1.388888888888889e-03, 8.333333333333333e-03, 4.1666666666666664e-02, 1.6666666666666666e-01, 0.5, 1.0, 1.0)


def exp_f32(xf):
    """yolox_exp_f32 of yolox_internal.h, operation by operation in float64"""
    xf = np.asarray(xf, F)
    x = xf.astype(np.float64)
    with np.errstate(all="ignore"):
        xs = np.where(np.isnan(x) | (x > 89.0) | (x < -104.0), 0.0, x)
        t = xs * 1.4426950408889634074
        k = np.where(t < 0.0, t - 0.5, t + 0.5).astype(np.int64)      # (int) truncates toward zero, as astype does
        kd = k.astype(np.float64)
        r = (xs - kd * 6.93147180369123816490e-01) - kd * 1.90821492927058770002e-10
        p = np.full_like(r, _EXP_COEF[0])
        for c in _EXP_COEF[1:]:
            p = p * r + c
        s = ((k + 1023) << 52).view(np.float64)
        out = (p * s).astype(F)
    out = np.where(x > 89.0, F(np.inf), out)
    out = np.where(x < -104.0, F(0.0), out)
    return np.where(np.isnan(x), xf, out).astype(F)


def sigmoid(x):
    with np.errstate(all="ignore"):
        return (F(1.0) / (F(1.0) + exp_f32(-np.asarray(x, F)))).astype(F)


def activate(v, act):
    v = np.asarray(v, F)
    if act == SILU:
        with np.errstate(all="ignore"):
            return (v * sigmoid(v)).astype(F)
    if act == SIGMOID:
        return sigmoid(v)
    return v


def conv_pre(x, w, b, stride):
    """the chain before the activation.  x: (H, W, Cin); w: (Cout, k, k, Cin); b: (Cout,) -> (Ho, Wo, Cout)"""
    x, w, b = np.asarray(x, F), np.asarray(w, F), np.asarray(b, F)
    H, W, Ci = x.shape
    Co, k = w.shape[0], w.shape[1]
    p = (k - 1) // 2
    Ho, Wo = (H + 2 * p - k) // stride + 1, (W + 2 * p - k) // stride + 1
    xp = np.zeros((H + 2 * p, W + 2 * p, Ci), F)      # +0.0f outside the map
    xp[p:p + H, p:p + W] = x
    acc = np.broadcast_to(b, (Ho, Wo, Co)).copy()
    for ky in range(k):
        for kx in range(k):
            win = xp[ky:ky + (Ho - 1) * stride + 1:stride, kx:kx + (Wo - 1) * stride + 1:stride]
            for ci in range(Ci):
                acc = fma(win[:, :, ci, None], w[None, None, :, ky, kx, ci], acc)
    return acc


def conv(x, w, b, stride=1, act=NONE, res=None):
    v = activate(conv_pre(x, w, b, stride), act)
    if res is not None:
        with np.errstate(all="ignore"):
            v = (v + np.asarray(res, F)).astype(F)
    return v


def _key(a):
    """an integer order on float32 in which -0 < +0 (NaN apart)"""
    u = np.asarray(a, F).view(np.uint32).astype(np.int64)
    return np.where(u >> 31, -(u & 0x7fffffff) - 1, u)


def maxpool(x, k):
    x = np.asarray(x, F)
    H, W, C = x.shape
    p = k // 2
    keys = np.full((H + 2 * p, W + 2 * p, C), _key(F(-np.inf)), np.int64)
    keys[p:p + H, p:p + W] = _key(x)
    nan = np.zeros((H + 2 * p, W + 2 * p, C), bool)
    nan[p:p + H, p:p + W] = np.isnan(x)
    best, anynan = np.full((H, W, C), np.iinfo(np.int64).min), np.zeros((H, W, C), bool)
    for dy in range(k):
        for dx in range(k):
            best = np.maximum(best, keys[dy:dy + H, dx:dx + W])
            anynan |= nan[dy:dy + H, dx:dx + W]
    u = np.where(best < 0, (-(best + 1)) | 0x80000000, best).astype(np.uint32)
    return np.where(anynan, CANONICAL_NAN, u.view(F)).astype(F)


def upsample2(x):
    return np.repeat(np.repeat(np.asarray(x, F), 2, axis=0), 2, axis=1)


def focus(blob):
    """(3, S, S) CHW -> (S / 2, S / 2, 12): top-left, bottom-left, top-right, bottom-right"""
    b = np.asarray(blob, F)
    parts = [b[:, dy::2, dx::2] for dx in (0, 1) for dy in (0, 1)]
    return np.ascontiguousarray(np.concatenate(parts, 0).transpose(1, 2, 0))


def forward(model, S, blob, inputs=None):
    """one frame through an eao_fusion_amd.detnet.Model: (tensors: id -> (H, W, C) array, head (anchors, 5 + classes) or None).  inputs: id -> array for the
    caller's input tensors."""
    from eao_fusion_amd import detnet as D
    W = np.concatenate([a.reshape(-1) for a in model.weights]) if model.weights else np.zeros(0, F)
    T, head_id, head = {}, None, None
    for t, (c, kind, a, b) in enumerate(model.tensors):
        if kind == D.HEAD:
            head_id, head = t, np.zeros((D.num_anchors(S), c), F)
        elif kind != D.BLOB:
            T[t] = np.zeros(model.shape(t, S), F)
    for t, v in (inputs or {}).items():
        T[t][...] = v
    for o in model.ops:
        sl = slice(o["src_c0"], o["src_c0"] + o["src_c"])
        dl = slice(o["dst_c0"], o["dst_c0"] + o["dst_c"])
        if o["kind"] == D.FOCUS:
            out = focus(blob)
        else:
            x = T[o["src"]][:, :, sl]
            if o["kind"] == D.CONV:
                k, ci, co = o["k"], o["src_c"], o["dst_c"]
                w = W[o["w_off"]:o["w_off"] + co * k * k * ci].reshape(co, k, k, ci)
                res = None if o["res"] < 0 else T[o["res"]][:, :, o["res_c0"]:o["res_c0"] + co]
                out = conv(x, w, W[o["b_off"]:o["b_off"] + co], o["stride"], o["act"], res)
            elif o["kind"] == D.MAXPOOL:
                out = maxpool(x, o["k"])
            else:
                out = upsample2(x)
        if o["dst"] == head_id:
            lvl = D.STRIDES.index(S // out.shape[0])
            a0 = sum((S // s) ** 2 for s in D.STRIDES[:lvl])
            head[a0:a0 + out.shape[0] * out.shape[1], dl] = out.reshape(-1, out.shape[2])
        else:
            T[o["dst"]][:, :, dl] = out
    return T, head
