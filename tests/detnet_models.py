"""Model files for the detector-network tests, generated from seeds in memory: the YOLOX graph (eao_fusion_amd.detnet.yolox_graph with seeded parameters), single-op
graphs over fixed maps, the seeded scenes every implementation is held to, the broken files the loader must refuse, and the helpers that build and run
tools/detnet_walk.cpp."""
import os
import struct
import subprocess
import tempfile

import numpy as np

from eao_fusion_amd import detnet as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def seeded_params(seed):
    """weights ~ N(0, 1 / K) and small biases, so that activations stay of order one through a deep graph"""
    rng = np.random.default_rng(seed)

    def params(name, cout, k, cin):
        w = rng.standard_normal((cout, k, k, cin)) / np.sqrt(k * k * cin)
        return w.astype(F), (0.1 * rng.standard_normal(cout)).astype(F)
    return params


def yolox(depth, width, classes, seed=0):
    """(Model, names) of upstream YOLOX with seeded, already folded parameters"""
    return D.yolox_graph(depth, width, classes, seeded_params(seed))


# the whole networks of the device tests and of tests/golden/detnet (tools/gen_golden_detnet.py): depth, width, classes, seed
NETS = {"w0125": (0.33, 0.125, 80, 21), "w05": (0.33, 0.5, 80, 22)}


def net_inputs(name, S=64):
    """(model, three blobs) of a whole network"""
    depth, width, classes, seed = NETS[name]
    return yolox(depth, width, classes, seed)[0], blob(S, seed + 100, batch=3)


def blob(S, seed, batch=None):
    rng = np.random.default_rng(seed)
    return rng.uniform(-2.0, 2.5, (3, S, S) if batch is None else (batch, 3, S, S)).astype(F)


def single_conv(x, w, b, stride=1, act=D.NONE, res=None, src_total=None, src_c0=0, dst_total=None, dst_c0=0, res_total=None, res_c0=0):
    """one convolution over a fixed map.  x: (H, W, Cin); the source is the channel range src_c0 .. of a caller's tensor of src_total channels, the destination the
    range dst_c0 .. of a tensor of dst_total channels, the residual (Ho, Wo, Cout) the range res_c0 .. of a caller's tensor of res_total channels with 777.0 around
    it.  Returns dict(model, inputs {tensor: array}, src, dst, res, out_shape)."""
    H, W, ci = x.shape
    co, k = w.shape[0], w.shape[1]
    p = (k - 1) // 2
    Ho, Wo = (H + 2 * p - k) // stride + 1, (W + 2 * p - k) // stride + 1
    src_total, dst_total = src_total or ci, dst_total or co
    m = D.Model(1)
    ts = m.fixed(src_total, H, W, caller_input=True)
    td = m.fixed(dst_total, Ho, Wo)
    full = np.full((H, W, src_total), F(777.0))      # (the neighbouring source channels: any use of them shows)
    full[:, :, src_c0:src_c0 + ci] = x
    inputs = {ts: full}
    tr = None
    if res is not None:
        res_total = res_total or co
        tr = m.fixed(res_total, Ho, Wo, caller_input=True)
        inputs[tr] = np.full((Ho, Wo, res_total), F(777.0))
        inputs[tr][:, :, res_c0:res_c0 + co] = res
    m.conv((ts, src_c0, ci), (td, dst_c0, co), w, b, stride=stride, act=act, res=None if tr is None else (tr, res_c0))
    return dict(model=m, inputs=inputs, src=ts, dst=td, res=tr, out_shape=(Ho, Wo, dst_total), S=32)


def single_map_op(kind, x, k=0, src_total=None, src_c0=0, dst_total=None, dst_c0=0):
    """MAXPOOL or UPSAMPLE2 over a fixed map x: (H, W, C), read as the channel range src_c0 .. of a caller's tensor of src_total channels (777.0 around it) and
    written to the range dst_c0 .. of a tensor of dst_total channels"""
    H, W, c = x.shape
    src_total, dst_total = src_total or c, dst_total or c
    m = D.Model(1)
    ts = m.fixed(src_total, H, W, caller_input=True)
    full = np.full((H, W, src_total), F(777.0))
    full[:, :, src_c0:src_c0 + c] = x
    if kind == D.MAXPOOL:
        td = m.fixed(dst_total, H, W)
        m.maxpool((ts, src_c0, c), (td, dst_c0, c), k)
        shape = (H, W, dst_total)
    else:
        td = m.fixed(dst_total, 2 * H, 2 * W)
        m.upsample2((ts, src_c0, c), (td, dst_c0, c))
        shape = (2 * H, 2 * W, dst_total)
    return dict(model=m, inputs={ts: full}, src=ts, dst=td, out_shape=shape, S=32)


def focus_only():
    m = D.Model(1)
    t = m.scaled(12, 2)
    m.focus((t, 0, 12))
    return dict(model=m, inputs={}, dst=t)


def planted_maps(H, W, C, seed):
    """a map with +-0, a NaN, +-inf and subnormals among ordinary values"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((H, W, C)).astype(F)
    flat = x.reshape(-1)
    n = flat.size
    specials = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1e-41, -1e-41], F)
    idx = rng.permutation(n)[:min(n, 3 * len(specials))]
    flat[idx] = np.resize(specials, idx.size)
    return x


# ---------------------------------------------------------------- the scenes of the host tests (small: the numpy yardstick walks every tap)
def scenes():
    rng = np.random.default_rng(4242)
    out = {}

    def rnd(*shape):
        return rng.standard_normal(shape).astype(F)

    out["conv_3x3_s1_silu"] = single_conv(rnd(5, 7, 3), rnd(4, 3, 3, 3), rnd(4), 1, D.SILU)
    out["conv_3x3_s2_odd_map"] = single_conv(rnd(5, 7, 5), rnd(6, 3, 3, 5), rnd(6), 2, D.NONE)
    out["conv_1x1_s2_sigmoid"] = single_conv(rnd(4, 4, 9), rnd(3, 1, 1, 9), rnd(3), 2, D.SIGMOID)
    out["conv_residual_inner_ranges"] = single_conv(rnd(6, 5, 4), rnd(5, 3, 3, 4), rnd(5), 1, D.SILU, res=rnd(6, 5, 5), src_total=9, src_c0=3, dst_total=8, dst_c0=2)
    # a bias of -0.0f, zero inputs and negative weights: every product is -0, the chain stays -0 and a kernel that pads K with (+0) * (+0) turns it into +0
    out["conv_minus_zero_bias"] = single_conv(np.zeros((3, 3, 3), F), -np.abs(rnd(2, 1, 1, 3)) - F(0.5), np.full(2, -0.0, F))
    out["conv_subnormal_weights"] = single_conv(rnd(3, 4, 6), (rnd(4, 3, 3, 6) * F(1e-39)).astype(F), (rnd(4) * F(1e-39)).astype(F))
    out["conv_inf_nan_inputs"] = single_conv(planted_maps(9, 10, 6, 11), rnd(3, 3, 3, 6), rnd(3), 1, D.SILU)
    out["maxpool_5_planted"] = single_map_op(D.MAXPOOL, planted_maps(5, 5, 3, 12), 5)
    out["maxpool_13_2x2"] = single_map_op(D.MAXPOOL, np.array([[[0.0], [-0.0]], [[-0.0], [-0.0]]], F), 13)
    out["upsample"] = single_map_op(D.UPSAMPLE2, planted_maps(3, 2, 5, 13))
    f = focus_only()
    out["focus_32"] = dict(f, S=32, blob=blob(32, 14))
    m, names = yolox(0.33, 0.125, 3, seed=15)
    out["yolox_nano_width_32"] = dict(model=m, inputs={}, S=32, blob=blob(32, 16), names=names)
    return out


# ---------------------------------------------------------------- files the loader must refuse
def _patch_op(data, model, op, field, value):
    """the bytes with one u32 field of op record `op` replaced (fields in the order of OpRec)"""
    fields = ["kind", "src", "src_c0", "src_c", "dst", "dst_c0", "dst_c", "k", "stride", "act", "groups", "res", "res_c0", "w_off", "b_off"]
    at = 40 + 16 * len(model.tensors) + 64 * op + 4 * fields.index(field)
    return data[:at] + struct.pack("<I", value) + data[at + 4:]


def broken_files():
    """name -> (bytes, S, a word the message must contain)"""
    m, _ = yolox(0.33, 0.125, 3, seed=15)
    good = m.tobytes()
    nT = len(m.tensors)
    convs = [i for i, o in enumerate(m.ops) if o["kind"] == D.CONV]
    out = {}
    out["truncated_tables"] = (good[:40 + 16 * nT + 10], 32, "truncated")
    out["truncated_weights"] = (good[:-4], 32, "pass the end")
    w_off = struct.unpack("<Q", good[24:32])[0]
    out["offset_past_the_end"] = (good[:24] + struct.pack("<Q", w_off + (1 << 40)) + good[32:], 32, "pass the end")
    out["weight_offset_past_the_end"] = (_patch_op(good, m, convs[3], "w_off", m.n_weights - 2), 32, "pass the end")
    out["channel_range_outside"] = (_patch_op(good, m, convs[0], "src_c0", 5), 32, "lie outside")
    out["channel_count_wraps"] = (_patch_op(good, m, convs[0], "src_c", 0xfffffff8), 32, "lie outside")
    # a read before a write: the two ops of a bottleneck swapped
    tables = 40 + 16 * nT
    i = next(j for j in convs if m.ops[j + 1]["kind"] == D.CONV and m.ops[j + 1]["src"] == m.ops[j]["dst"])
    a, b = good[tables + 64 * i:tables + 64 * i + 64], good[tables + 64 * i + 64:tables + 64 * i + 128]
    out["read_before_write"] = (good[:tables + 64 * i] + b + a + good[tables + 64 * i + 128:], 32, "before it is written")
    out["double_write"] = (_patch_op(good, m, convs[2], "dst", m.ops[convs[1]]["dst"]), 32, "second time")
    m2, _ = yolox(0.33, 0.125, 3, seed=15)
    last = max(i for i, o in enumerate(m2.ops) if o["dst_c"] == 1)      # an objectness prediction: one head column of one level
    m2.ops.pop(last)
    out["uncovered_output_row"] = (m2.tobytes(), 32, "not covered")
    out["grouped_convolution"] = (_patch_op(good, m, convs[4], "groups", 4), 32, "grouped")
    out["wrong_shape_under_stride"] = (_patch_op(good, m, convs[1], "stride", 1), 32, "map")
    out["bad_magic"] = (b"EAODNEX\0" + good[8:], 32, "magic")
    return out


# ---------------------------------------------------------------- tools/detnet_walk.cpp
_built = {}


def walk_binary(flags=("-O2",)):
    """the path of detnet_walk built with these flags (once per process, in a temporary directory)"""
    key = tuple(flags)
    if key not in _built:
        d = tempfile.mkdtemp(prefix="detnet_walk_")
        exe = os.path.join(d, "detnet_walk")
        subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", *flags, os.path.join(ROOT, "tools", "detnet_walk.cpp"), "-o", exe])
        _built[key] = exe
    return _built[key]


def _layout(stdout):
    """the tensor table detnet_walk prints: id -> (kind, offset, (H, W, C))"""
    t = {}
    for line in stdout.splitlines():
        q = line.split()
        if q and q[0] == "tensor":
            t[int(q[1])] = (int(q[3]), int(q[5]), (int(q[7]), int(q[8]), int(q[9])))
    return t


def walk_check(exe, data, S):
    """(accepted, stdout, return code, stderr) of `detnet_walk check`"""
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "m.bin")
        open(p, "wb").write(data)
        r = subprocess.run([exe, "check", p, str(S)], capture_output=True, text=True)
    return r.stdout.startswith("ok"), r.stdout, r.returncode, r.stderr


def walk_run(exe, model, S, blob_=None, inputs=None):
    """one frame through detnet_walk: (tensors: id -> (H, W, C) array, head or None)"""
    data = model.tobytes()
    with tempfile.TemporaryDirectory() as d:
        pm, pb, po, pa = (os.path.join(d, n) for n in ("m.bin", "blob.bin", "out", "act.bin"))
        open(pm, "wb").write(data)
        chk = subprocess.run([exe, "check", pm, str(S)], capture_output=True, text=True, check=True)
        assert chk.stdout.startswith("ok"), chk.stdout
        lay = _layout(chk.stdout)
        act_floats = int(chk.stdout.split()[6])
        args = [exe, "run", pm, str(S), "-", po]
        if blob_ is not None:
            np.ascontiguousarray(blob_, "<f4").tofile(pb)
            args[4] = pb
        if inputs:
            act = np.zeros(act_floats, F)
            for t, v in inputs.items():
                off, shape = lay[t][1], lay[t][2]
                act[off:off + int(np.prod(shape))] = np.asarray(v, F).reshape(-1)
            act.tofile(pa)
            args.append(pa)
        r = subprocess.run(args, capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, (r.returncode, r.stdout[-400:], r.stderr[-2000:])
        act = np.fromfile(po + ".act", "<f4")
        prob = np.fromfile(po + ".prob", "<f4")
    tensors = {t: act[off:off + int(np.prod(shape))].reshape(shape).copy() for t, (kind, off, shape) in lay.items() if kind in (D.SCALED, D.FIXED, D.FIXED_INPUT)}
    head = prob.reshape(-1, 5 + model.classes) if prob.size else None
    return tensors, head


def walk_forms(exe, model, S, batch):
    """`detnet_walk forms`: one dict per op -- kind (a word), M, Cout, k, stride, res, src_c0, dst_c0, head and, for a convolution, form (the tile form the device
    takes at this batch: "32x32x2", "16x16x4x2" or "16x16x4x1"; None for the other ops)"""
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "m.bin")
        open(p, "wb").write(model if isinstance(model, bytes) else model.tobytes())
        r = subprocess.run([exe, "forms", p, str(S), str(batch)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr and r.stdout.startswith("ok"), (r.returncode, r.stdout[-400:], r.stderr[-2000:])
    ops = []
    for line in r.stdout.splitlines()[1:]:
        q = line.split()
        f = dict(zip(q[2::2], q[3::2]))
        ops.append({k: (v if k in ("kind", "form") else int(v)) for k, v in f.items()})
        ops[-1].setdefault("form", None)
        assert int(q[1]) == len(ops) - 1
    return ops


LARGE = "32x32x2"


def same_bits(a, b):
    """equal bit patterns; a NaN equals any NaN (IEEE 754 leaves the sign and payload of a generated NaN to the implementation: inf - inf is 0xffc00000 on x86 and
    0x7fc00000 on gfx950; maxpool, which defines its NaN, is held to it by its own tests)"""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])
