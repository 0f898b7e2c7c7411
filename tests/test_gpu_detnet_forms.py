"""k_detnet_conv<32, 2>, the 128 x 64 tile on v_mfma_f32_32x32x2_f32 (eao_fusion_amd/csrc/detnet.hip), against the -O2 host walk (tools/detnet_walk.cpp): an M tail,
blocks that straddle the frames of a batch, stride 2, a 3 x 3 kernel over several 64-deep stages, a residual, inner channel ranges, the head as destination and
the -0.0f padding rule; then whole networks at other input sizes and the map ops with inner ranges.  Every float as its bit pattern (detnet_models.same_bits), no
tolerance.  All forms give the same bits, so every case first asks `detnet_walk forms` (conv_form of csrc/detnet_internal.h, the rule launch_op switches on)
which form its convolution takes."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detnet_models as M  # noqa: E402
import detnet_reference as R  # noqa: E402
from test_gpu_detnet import SENTINEL, dev, run_graph  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
NONE, SILU, SIGMOID = 0, 1, 2


@pytest.fixture(scope="module")
def DN():
    import torch  # noqa: F401  (first, so that both runtimes resolve the same libamdhip64)
    from eao_fusion_amd import detnet
    return detnet


def exe():
    return M.walk_binary(("-O2",))


def forms(model, S, batch):
    return M.walk_forms(exe(), model, S, batch)


def walked(sc, inputs):
    """the destination tensor of a graph over fixed maps by the host walk, its other channels holding SENTINEL before the walk"""
    inputs = dict(inputs)
    inputs[sc["dst"]] = np.full(sc["out_shape"], SENTINEL)
    return M.walk_run(exe(), sc["model"], 32, inputs=inputs)[0][sc["dst"]]


# ---------------------------------------------------------------- (a) one convolution per case, every one on the 32 x 32 x 2 form
# Blocks are 128 rows x 64 columns and the form is taken from 256 blocks on.  hw: the input map; inner: the source is the channel range 1 .. of a tensor three
# channels wider (the destination always is the range 2 .., so that its neighbours can be checked); res: 0 none, 1 a tensor of its own, 2 the range 2 .. of a wider one.
LARGE_CASES = {
    # K = 1 (one padded tap per instruction); the second 32-wide tile is wholly masked; M = 32761 = 255 x 128 + 121
    "k1_cout17_tail121": dict(batch=1, hw=(181, 181), ci=1, co=17, k=1, stride=1, act=NONE, res=0, inner=False, blocks=(256, 1)),
    # K = 3; one live column in the second tile
    "k3_cout33_residual": dict(batch=1, hw=(181, 181), ci=3, co=33, k=1, stride=1, act=SILU, res=1, inner=False, blocks=(256, 1)),
    # K = 72 (one stage and 8); a frame has 10920 = 85 x 128 + 40 rows: blocks 85 and 170 straddle two frames; the three frames hold different values
    "k72_batch3_straddle": dict(batch=3, hw=(105, 104), ci=8, co=64, k=3, stride=1, act=SIGMOID, res=2, inner=True, blocks=(256, 1)),
    # K = 189: no tap boundary on a stage boundary; two column blocks, the second with one column; M = 16383 = 127 x 128 + 127; +-0, NaN, +-inf, subnormals
    "k189_planted_cout65": dict(batch=1, hw=(127, 129), ci=21, co=65, k=3, stride=1, act=SILU, res=0, inner=True, planted=True, blocks=(128, 2)),
    # stride 2 from an even and an odd side to 81 x 81; K = 63; five column blocks; M = 6561 = 51 x 128 + 33
    "k63_stride2_cout257": dict(batch=1, hw=(162, 161), ci=7, co=257, k=3, stride=2, act=NONE, res=1, inner=False, blocks=(52, 5)),
    # 1 x 1 at stride 2 to 60 x 60; K is exactly one stage; a frame has 3600 = 28 x 128 + 16 rows
    "k64_1x1_stride2_batch2": dict(batch=2, hw=(119, 120), ci=64, co=257, k=1, stride=2, act=SIGMOID, res=0, inner=False, blocks=(57, 5)),
    # K = 288: four and a half stages of a 3 x 3; three column blocks
    "k288_cout129": dict(batch=1, hw=(105, 104), ci=32, co=129, k=3, stride=1, act=SILU, res=0, inner=False, blocks=(86, 3)),
    # K = 129: two stages and one tap
    "k129_1x1_cout80": dict(batch=1, hw=(127, 129), ci=129, co=80, k=1, stride=1, act=NONE, res=0, inner=False, blocks=(128, 2)),
}


def large_scene(c, seed):
    """(scene, the input tensors of every frame)"""
    rng = np.random.default_rng(seed)
    (H, W), ci, co, k, s = c["hw"], c["ci"], c["co"], c["k"], c["stride"]
    p = (k - 1) // 2
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    w = (rng.standard_normal((co, k, k, ci)) / np.sqrt(k * k * ci)).astype(F)
    b = rng.standard_normal(co).astype(F)

    def maps():
        x = M.planted_maps(H, W, ci, seed) if c.get("planted") else rng.standard_normal((H, W, ci)).astype(F)
        return x, (rng.standard_normal((Ho, Wo, co)).astype(F) if c["res"] else None)

    def scene(x, res):
        return M.single_conv(x, w, b, s, c["act"], res, src_total=ci + 3 if c["inner"] else None, src_c0=1 if c["inner"] else 0, dst_total=co + 3, dst_c0=2,
                             res_total=co + 5 if c["res"] == 2 else None, res_c0=2 if c["res"] == 2 else 0)
    sc = scene(*maps())
    frames = [sc["inputs"]] + [scene(*maps())["inputs"] for _ in range(c["batch"] - 1)]
    return sc, frames


@pytest.mark.parametrize("name", sorted(LARGE_CASES))
def test_large_form_convolution(DN, name):
    c = LARGE_CASES[name]
    sc, frames = large_scene(c, 9100 + sorted(LARGE_CASES).index(name))
    op = forms(sc["model"], 32, c["batch"])[0]
    Ho, Wo, _ = sc["out_shape"]
    assert op["form"] == M.LARGE and op["M"] == c["batch"] * Ho * Wo and (-(-op["M"] // 128), -(-c["co"] // 64)) == c["blocks"], op
    got = run_graph(DN, sc, frames)
    lo, hi = 2, 2 + c["co"]
    for f, inputs in enumerate(frames):
        want = walked(sc, inputs)
        assert (got[f][:, :, :lo] == SENTINEL).all() and (got[f][:, :, hi:] == SENTINEL).all(), "the neighbouring channels were written"
        assert M.same_bits(got[f], want), "%s frame %d" % (name, f)
        if c.get("planted"):
            assert np.isnan(want).any() and np.isinf(want).any(), "the scene is meant to carry NaN and infinities to the output"


# ---------------------------------------------------------------- (b) the -0.0f chain
@pytest.mark.parametrize("K", (1, 3, 5, 63, 65))
def test_minus_zero_bias_on_the_large_form(DN, K):
    """zero inputs, negative weights, a bias of -0.0f: every product is -0 and the chain stays -0; a kernel that pads K with (+0) * (+0) turns it into +0.  K = 1,
    3, 5 end inside an instruction's two taps, 63 and 65 on both sides of the 64-deep stage."""
    rng = np.random.default_rng(30 + K)
    sc = M.single_conv(np.zeros((181, 181, K), F), (-np.abs(rng.standard_normal((33, 1, 1, K))) - 0.5).astype(F), np.full(33, -0.0, F))
    assert forms(sc["model"], 32, 1)[0]["form"] == M.LARGE
    assert (run_graph(DN, sc)[0].view(np.uint32) == 0x80000000).all()


# ---------------------------------------------------------------- (c) the head as destination
def head_model(DN, S, classes):
    """per level one caller-filled map of 6 channels, read at channel 1 with Cin = 4 by three 1 x 1 convolutions that write columns 0 .. 3 (none), 4 (sigmoid) and
    5 .. (sigmoid) of the head.  Returns (model, the three input tensors)."""
    rng = np.random.default_rng(41)
    m = DN.Model(classes)
    maps = [m.fixed(6, S // s, S // s, caller_input=True) for s in DN.STRIDES]
    head = m.head()
    for t in maps:
        for c0, co, act in ((0, 4, NONE), (4, 1, SIGMOID), (5, classes, SIGMOID)):
            m.conv((t, 1, 4), (head, c0, co), (rng.standard_normal((co, 1, 1, 4)) / 2).astype(F), rng.standard_normal(co).astype(F), act=act)
    return m, maps


def test_head_destination_on_the_large_form(DN):
    """124 classes (a row of 129 floats), S = 256, sixteen frames: the class convolution of level 0 has M = 16384 and two column blocks and takes the large form, the
    other eight the small ones; all nine write rows of the head at its stride, frame by frame, and nothing behind the sixteenth frame"""
    import torch
    S, B, classes = 256, 16, 124
    m, maps = head_model(DN, S, classes)
    ops = forms(m, S, B)
    assert [o["form"] for o in ops] == ["16x16x4x1", "16x16x4x1", M.LARGE, "16x16x4x1", "16x16x4x1", "16x16x4x2", "16x16x4x1", "16x16x4x1", "16x16x4x2"]
    assert all(o["head"] for o in ops) and ops[2]["M"] == 16384 and ops[2]["Cout"] == 124
    rng = np.random.default_rng(42)
    inputs = [{t: rng.standard_normal(m.shape(t, S)).astype(F) for t in maps} for _ in range(3)]
    want = [M.walk_run(exe(), m, S, inputs=inputs[i])[1] for i in range(3)]
    net = DN.Detnet(m.tobytes(), S, max_batch=B)
    assert (net.A, net.row) == (1344, 129)
    for f in range(B):
        for t in maps:
            net.set_tensor(t, inputs[f % 3][t], f)
    d_blob = torch.zeros((B, 3, S, S), dtype=torch.float32, device="cuda")
    d_prob = torch.full((B + 1, net.A, net.row), float(SENTINEL), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    net.forward(d_blob.data_ptr(), d_prob.data_ptr(), B)
    torch.cuda.synchronize()
    got = d_prob.cpu().numpy()
    net.close()
    assert (got[B] == SENTINEL).all(), "the frame behind the batch was written"
    assert not M.same_bits(want[0], want[1]) and not M.same_bits(want[1], want[2])
    for f in range(B):
        assert M.same_bits(got[f], want[f % 3]), "frame %d" % f


# ---------------------------------------------------------------- (d), (e) whole networks
_walks = {}


def whole(name, S):
    """(model, three blobs, the walk's (tensors, head) of each) -- computed once"""
    if (name, S) not in _walks:
        model, blobs = M.net_inputs(name, S=S)
        _walks[name, S] = (model, blobs, [M.walk_run(exe(), model, S, blobs[i]) for i in range(3)])
    return _walks[name, S]


def forward_batch(DN, model, S, blobs):
    import torch
    net = DN.Detnet(model.tobytes(), S, max_batch=len(blobs))
    d_blob, d_prob = dev(blobs), torch.zeros((len(blobs), net.A, net.row), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    net.forward(d_blob.data_ptr(), d_prob.data_ptr(), len(blobs))
    torch.cuda.synchronize()
    return net, d_prob.cpu().numpy()


def test_whole_network_with_the_large_form_in_it(DN):
    """YOLOX at width 0.5, S = 128, 32 frames: the stem, dark2's stride-2 3 x 3, its CSP 1 x 1s (one of them into the channel range 32 .. of the concatenation), the
    bottleneck 3 x 3 with its residual and conv3 run on the large form between ops on the small ones"""
    S, B = 128, 32
    model, blobs, walks = whole("w05", S)
    large = [o for o in forms(model, S, B) if o["form"] == M.LARGE]
    assert any(o["stride"] == 2 for o in large) and any(o["res"] >= 0 for o in large) and any(o["dst_c0"] > 0 for o in large)
    assert any(o["k"] == 3 for o in large) and any(o["k"] == 1 for o in large)
    net, heads = forward_batch(DN, model, S, np.stack([blobs[f % 3] for f in range(B)]))
    for f in range(B):
        assert M.same_bits(heads[f], walks[f % 3][1]), "the head of frame %d" % f
    for f in (0, 1, 2, 17, 31):
        tensors = walks[f % 3][0]
        for t in sorted(tensors):
            assert M.same_bits(net.tensor(t, tensors[t].shape, f), tensors[t]), "tensor %d of frame %d" % (t, f)
    net.close()


@pytest.mark.parametrize("S,anchors", ((32, 21), (96, 189)))
def test_whole_network_at_other_input_sizes(DN, S, anchors):
    """S = 32: the level-2 map is 1 x 1; S = 96: it is 3 x 3 (odd) under 12 x 12 and 6 x 6"""
    model, blobs, walks = whole("w0125", S)
    net, heads = forward_batch(DN, model, S, blobs[:2])
    assert net.A == anchors
    for f in range(2):
        tensors, head = walks[f]
        assert M.same_bits(heads[f], head), "the head of frame %d" % f
        for t in sorted(tensors):
            assert M.same_bits(net.tensor(t, tensors[t].shape, f), tensors[t]), "tensor %d of frame %d" % (t, f)
    net.close()


# ---------------------------------------------------------------- (f) the map ops with inner ranges and a batch
@pytest.mark.parametrize("kind", ("maxpool", "upsample2"))
def test_map_op_with_inner_ranges_and_a_batch(DN, kind):
    """channels 1 .. 5 of a 7-channel tensor into channels 2 .. 6 of an 8-channel tensor, two frames of different values"""
    def scene(seed):
        x = M.planted_maps(5, 7, 5, seed)
        return (M.single_map_op(DN.MAXPOOL, x, 5, src_total=7, src_c0=1, dst_total=8, dst_c0=2) if kind == "maxpool" else
                M.single_map_op(DN.UPSAMPLE2, x, src_total=7, src_c0=1, dst_total=8, dst_c0=2)), x
    (sc, x0), (sc1, x1) = scene(60), scene(61)
    op = forms(sc["model"], 32, 2)[0]
    assert (op["kind"], op["src_c0"], op["dst_c0"], op["Cout"], op["form"]) == (kind, 1, 2, 5, None)
    frames = [sc["inputs"], sc1["inputs"]]
    got = run_graph(DN, sc, frames)
    for f, x in enumerate((x0, x1)):
        assert (got[f][:, :, :2] == SENTINEL).all() and (got[f][:, :, 7:] == SENTINEL).all(), "the neighbouring channels were written"
        assert M.same_bits(got[f], walked(sc, frames[f])), "frame %d" % f
        want = R.maxpool(x, 5) if kind == "maxpool" else R.upsample2(x)
        assert M.same_bits(got[f][:, :, 2:7], want) and (kind != "maxpool" or np.array_equal(got[f][:, :, 2:7].view(np.uint32), want.view(np.uint32)))
