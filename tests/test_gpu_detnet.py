"""The detector network on the device (eao_fusion_amd/csrc/detnet.hip through eao_fusion_amd/detnet.py) against the numpy yardstick (tests/detnet_reference.py)
and the host walk (tools/detnet_walk.cpp, -O2): every float as its 32-bit pattern, no tolerance anywhere (a NaN equals a NaN: see detnet_models.same_bits)."""
import os
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detnet_models as M  # noqa: E402
import detnet_reference as R  # noqa: E402
import yolox_reference as Y  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "detnet")
F = np.float32
SENTINEL = F(555.25)


@pytest.fixture(scope="module")
def DN():
    import torch  # noqa: F401  (first, so that both runtimes resolve the same libamdhip64)
    from eao_fusion_amd import detnet
    return detnet


def dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def run_graph(DN, sc, frames=None, S=32):
    """a graph over fixed maps: frames = a list of {tensor: array} (default: the scene's own inputs); the destination's other channels hold SENTINEL before the
    call.  Returns the destination tensor of every frame."""
    import torch
    frames = frames or [sc["inputs"]]
    net = DN.Detnet(sc["model"].tobytes(), S, max_batch=len(frames))
    for f, inputs in enumerate(frames):
        net.set_tensor(sc["dst"], np.full(sc["out_shape"], SENTINEL), f)
        for t, v in inputs.items():
            net.set_tensor(t, v, f)
    d_blob = torch.zeros((len(frames), 3, S, S), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    net.forward(d_blob.data_ptr(), None, len(frames))
    out = [net.tensor(sc["dst"], sc["out_shape"], f) for f in range(len(frames))]
    net.close()
    return out


def expect_graph(sc, inputs=None):
    inputs = dict(inputs or sc["inputs"])
    inputs[sc["dst"]] = np.full(sc["out_shape"], SENTINEL)
    return R.forward(sc["model"], 32, None, inputs)[0][sc["dst"]]


# ---------------------------------------------------------------- 1. one convolution per case
CINS, COUTS, MAPS = (1, 3, 12, 31, 32, 33, 64), (1, 4, 31, 32, 33, 80), ((1, 1), (5, 7), (20, 20), (33, 31))
ACTS = (0, 1, 2)


def conv_cases():
    """every Cin with both k, every Cout on every map; the other parameters rotate so that every value of each meets every value of most others.  Cin 1, 2, 3, 4
    with k = 1 are K = 1 .. 4; Cin 63, 64, 65 and 127, 128, 129 with k = 1 straddle the 64- and 128-deep LDS stages; Cin 12 with k = 3 (K = 108) leaves a remainder."""
    cases, i = [], 0
    for ci in CINS + (2, 4, 63, 65, 127, 128, 129):
        for k in (1, 3):
            cases.append(dict(ci=ci, co=COUTS[i % 6], hw=MAPS[(i // 2) % 4], k=k, stride=1 + (i // 3) % 2, act=ACTS[i % 3], res=i % 4 == 1, batch=1))
            i += 1
    for co in COUTS:
        for hw in MAPS:
            cases.append(dict(ci=CINS[i % 7], co=co, hw=hw, k=(1, 3)[(i // 2) % 2], stride=1 + i % 2, act=ACTS[(i // 2) % 3], res=i % 5 == 0, batch=3 if i % 4 == 0 else 1))
            i += 1
    return cases


CONV_CASES = conv_cases()


def conv_scene(c, seed):
    rng = np.random.default_rng(seed)
    H, W = c["hw"]
    x = rng.standard_normal((H, W, c["ci"])).astype(F)
    w = (rng.standard_normal((c["co"], c["k"], c["k"], c["ci"])) / np.sqrt(c["k"] * c["k"] * c["ci"])).astype(F)
    b = rng.standard_normal(c["co"]).astype(F)
    p = (c["k"] - 1) // 2
    Ho, Wo = (H + 2 * p - c["k"]) // c["stride"] + 1, (W + 2 * p - c["k"]) // c["stride"] + 1
    res = rng.standard_normal((Ho, Wo, c["co"])).astype(F) if c["res"] else None
    # inner channel ranges of wider tensors on both sides
    return M.single_conv(x, w, b, c["stride"], c["act"], res, src_total=c["ci"] + 3, src_c0=1, dst_total=c["co"] + 3, dst_c0=2), rng


@pytest.mark.parametrize("n", range(len(CONV_CASES)))
def test_convolution(DN, n):
    c = CONV_CASES[n]
    sc, rng = conv_scene(c, 9000 + n)
    frames = [sc["inputs"]]
    for _ in range(c["batch"] - 1):
        frames.append({t: (rng.standard_normal(v.shape).astype(F) if t != sc["src"] else
                           np.where(v == F(777.0), v, rng.standard_normal(v.shape).astype(F))) for t, v in sc["inputs"].items()})
    got = run_graph(DN, sc, frames)
    lo, hi = 2, 2 + c["co"]
    for f, inputs in enumerate(frames):
        want = expect_graph(sc, inputs)
        assert (got[f][:, :, :lo] == SENTINEL).all() and (got[f][:, :, hi:] == SENTINEL).all(), "the neighbouring channels were written"
        assert M.same_bits(got[f], want), "%r frame %d" % (c, f)


def large_form(sc, batch=1):
    """whether the device runs the scene's convolution on the 32 x 32 x 2 form (all forms give the same bits: only the rule itself can say)"""
    return M.walk_forms(M.walk_binary(("-O2",)), sc["model"], 32, batch)[0]["form"] == M.LARGE


def test_convolution_takes_the_large_tile_form(DN):
    """128 x 128 outputs over 80 channels: 256 blocks of 128 x 64, the threshold at which the 32 x 32 x 2 form is chosen.  A = the identity (pixel m reads 1 at
    channel m % 64) with an asymmetric B: output (m, co) is W[co][m % 64] = 100 co + m % 64, so a swapped row and column map shows.  Then ordinary values with
    K = 27 (one padded k behind the end) against the host walk."""
    H = W = 128
    x = np.zeros((H * W, 64), F)
    x[np.arange(H * W), np.arange(H * W) % 64] = 1
    w = (100 * np.arange(80)[:, None] + np.arange(64)[None, :]).astype(F).reshape(80, 1, 1, 64)
    sc = M.single_conv(x.reshape(H, W, 64), w, np.zeros(80, F))
    assert large_form(sc)
    got = run_graph(DN, sc)[0].reshape(H * W, 80)
    assert np.array_equal(got, w.reshape(80, 64).T[np.arange(H * W) % 64])
    rng = np.random.default_rng(77)
    sc = M.single_conv(rng.standard_normal((H, W, 3)).astype(F), rng.standard_normal((80, 3, 3, 3)).astype(F), rng.standard_normal(80).astype(F), 1, 1)
    assert large_form(sc)
    want = M.walk_run(M.walk_binary(("-O2",)), sc["model"], 32, inputs=sc["inputs"])[0][sc["dst"]]
    assert M.same_bits(run_graph(DN, sc)[0], want)
    # K = 65: one tap behind the 64-deep stage of this form
    sc = M.single_conv(rng.standard_normal((H, W, 65)).astype(F), rng.standard_normal((80, 1, 1, 65)).astype(F), rng.standard_normal(80).astype(F), 1, 2)
    assert large_form(sc)
    want = M.walk_run(M.walk_binary(("-O2",)), sc["model"], 32, inputs=sc["inputs"])[0][sc["dst"]]
    assert M.same_bits(run_graph(DN, sc)[0], want)


@pytest.mark.parametrize("n", (5, 16, 33))
def test_identity_with_asymmetric_b(DN, n):
    """the small tile forms (Cout <= 16: one 16-wide tile; above: two): a 1 x n map holding the identity, W[co][ci] = 100 co + ci"""
    w = (100 * np.arange(n)[:, None] + np.arange(n)[None, :]).astype(F).reshape(n, 1, 1, n)
    sc = M.single_conv(np.eye(n, dtype=F).reshape(1, n, n), w, np.zeros(n, F))
    assert np.array_equal(run_graph(DN, sc)[0].reshape(n, n), w.reshape(n, n).T)


PLANTED = ["conv_minus_zero_bias", "conv_subnormal_weights", "conv_inf_nan_inputs", "conv_residual_inner_ranges"]


@pytest.mark.parametrize("name", PLANTED)
def test_planted_values(DN, name):
    sc = M.scenes()[name]
    got, want = run_graph(DN, sc)[0], expect_graph(sc)
    assert M.same_bits(got, want)
    if name == "conv_minus_zero_bias":
        assert (got.view(np.uint32) == 0x80000000).all(), "a padded K turned -0.0f into +0.0f"
    if name == "conv_subnormal_weights":
        assert (np.abs(want[want != 0]) < F(1.2e-38)).any(), "the scene is meant to produce subnormal outputs"


def test_minus_zero_bias_on_the_two_small_tile_forms(DN):
    """the -0.0f chain for K = 1, 3, 5, 31, 33 and Cout on both sides of 16: behind K the kernels pad with (+0) * (-0).  A 3 x 3 map (M = 9) stays on the two
    16 x 16 x 4 forms; the 32 x 32 x 2 form has test_minus_zero_bias_on_the_large_form (tests/test_gpu_detnet_forms.py)."""
    rng = np.random.default_rng(3)
    for ci in (1, 3, 5, 31, 33):
        for co in (2, 33):
            sc = M.single_conv(np.zeros((3, 3, ci), F), (-np.abs(rng.standard_normal((co, 1, 1, ci))) - 0.5).astype(F), np.full(co, -0.0, F))
            assert (run_graph(DN, sc)[0].view(np.uint32) == 0x80000000).all(), (ci, co)


# ---------------------------------------------------------------- 2. plain ops
@pytest.mark.parametrize("k", (5, 9, 13))
@pytest.mark.parametrize("hw", ((2, 2), (5, 5), (20, 20)))
def test_maxpool(DN, k, hw):
    x = M.planted_maps(hw[0], hw[1], 5, 100 + k)
    x[np.isinf(x)] = F(-0.0)
    sc = M.single_map_op(DN.MAXPOOL, x, k)
    got = run_graph(DN, sc)[0]
    assert np.array_equal(got.view(np.uint32), R.maxpool(x, k).view(np.uint32)) and (got.view(np.uint32) == 0x7fc00000).any()
    z = M.single_map_op(DN.MAXPOOL, np.array([[[0.0, -0.0], [-0.0, -0.0]], [[-0.0, -0.0], [-0.0, -0.0]]], F), k)
    gz = run_graph(DN, z)[0]
    assert (gz[:, :, 0].view(np.uint32) == 0).all() and (gz[:, :, 1].view(np.uint32) == 0x80000000).all()


@pytest.mark.parametrize("S", (32, 64))
def test_upsample_and_focus(DN, S):
    import torch
    x = M.planted_maps(S // 4, S // 4 - 1, 7, S)
    sc = M.single_map_op(DN.UPSAMPLE2, x)
    assert M.same_bits(run_graph(DN, sc)[0], R.upsample2(x))
    f = M.focus_only()
    blobs = M.blob(S, 5, batch=2)
    net = DN.Detnet(f["model"].tobytes(), S, max_batch=2)
    d = dev(blobs)
    net.forward(d.data_ptr(), None, 2)
    for n in range(2):
        assert M.same_bits(net.tensor(f["dst"], (S // 2, S // 2, 12), n), R.focus(blobs[n]))
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 3. whole networks at S = 64
NETS = M.NETS
_nets = {}


def whole(name):
    """(model, blobs (3 frames), the walk's tensors and head of every frame) -- computed once"""
    if name not in _nets:
        model, blobs = M.net_inputs(name)
        exe = M.walk_binary(("-O2",))
        _nets[name] = (model, blobs, [M.walk_run(exe, model, 64, blobs[f]) for f in range(3)])
    return _nets[name]


def forward_heads(DN, model, blobs, max_batch, stream=None):
    import torch
    net = DN.Detnet(model.tobytes(), 64, max_batch=max_batch)
    d_blob, d_prob = dev(blobs), torch.zeros((len(blobs), net.A, net.row), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    net.forward(d_blob.data_ptr(), d_prob.data_ptr(), len(blobs), stream)
    torch.cuda.synchronize()
    return net, d_prob.cpu().numpy()


@pytest.mark.parametrize("name", sorted(NETS))
def test_whole_network(DN, name):
    model, blobs, walked = whole(name)
    net, heads = forward_heads(DN, model, blobs[:1], 1)
    assert net.A == 84 and net.info()["flops"] > 0 and net.info()["activation_bytes"] > 0
    tensors, head = walked[0]
    for t in sorted(tensors):
        assert M.same_bits(net.tensor(t, tensors[t].shape), tensors[t]), "tensor %d" % t
    assert M.same_bits(heads[0], head)
    z = np.load(os.path.join(GOLDEN, "yolox_%s_s64.npz" % name))
    assert heads[0].tobytes() == z["head"].view(F).tobytes(), "the head differs from the recorded one"


# ---------------------------------------------------------------- 4. batch and determinism
def test_batch_equals_single_calls_and_repeats(DN):
    model, blobs, walked = whole("w0125")
    net, heads = forward_heads(DN, model, blobs, 3)
    for f in range(3):
        assert M.same_bits(heads[f], walked[f][1]), "frame %d of the batch" % f
        for t in sorted(walked[f][0]):
            assert M.same_bits(net.tensor(t, walked[f][0][t].shape, f), walked[f][0][t]), "tensor %d of frame %d" % (t, f)
    _, again = forward_heads(DN, model, blobs, 3)
    assert heads.tobytes() == again.tobytes()
    for f in range(3):
        assert forward_heads(DN, model, blobs[f:f + 1], 1)[1].tobytes() == heads[f:f + 1].tobytes()


def test_four_threads_on_four_handles(DN):
    import torch
    model, blobs, walked = whole("w0125")
    out, errors = [None] * 4, []

    def work(i):
        try:
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                out[i] = forward_heads(DN, model, blobs[i % 3:i % 3 + 1], 1, s.cuda_stream)[1]
            s.synchronize()
        except Exception as e:      # noqa: BLE001
            errors.append(e)
    threads = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for i in range(4):
        assert M.same_bits(out[i][0], walked[i % 3][1])


# ---------------------------------------------------------------- 5. the chain
def test_preprocess_forward_decode_chain(DN):
    """eao_yolox_preprocess -> eao_detnet_forward on the handle's buffers and stream -> eao_yolox_decode_device: the objects of the host's literal decode (the
    device's tie rule) over the walk's head of the same blob"""
    from eao_fusion_amd import yolox
    model, _, _ = whole("w05")
    yx = yolox.Yolox(input_size=64, max_proposals=8192)
    img = np.random.RandomState(8).randint(0, 256, (37, 51, 3)).astype(np.uint8)
    blob = yx.preprocess(img)[0]
    d_blob, d_prob, stream = yx.buffers()
    net = DN.Detnet(model.tobytes(), 64, 1)
    net.forward(d_blob, d_prob, 1, stream)
    got = yx.decode_device(d_prob, 1, [(51, 37)], cap=8192, stream=stream)[0]
    head = M.walk_run(M.walk_binary(("-O2",)), model, 64, blob)[1]
    want = Y.decode_literal(head, 64, 51, 37, stable=True)
    assert got["n_proposals"] == len(want["proposals"]) > 0 and len(want["objects"]) > 0
    assert Y.same_records(got["objects"], want["objects"])


# ---------------------------------------------------------------- 6. refusals
def test_refusals_leave_their_outputs(DN):
    import torch
    from eao_fusion_amd import _lib
    for name, (data, S, word) in M.broken_files().items():
        with pytest.raises(_lib.EaoError) as e:
            DN.Detnet(data, S, 1)
        assert e.value.status == _lib.EAO_ERR_INVALID and word in str(e.value), name
    model, blobs, walked = whole("w0125")
    net = DN.Detnet(model.tobytes(), 64, max_batch=2)
    d_blob = dev(blobs[:2])
    d_prob = torch.full((2, net.A, net.row), 7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for args in ((d_blob.data_ptr(), d_prob.data_ptr(), 3), (d_blob.data_ptr(), d_prob.data_ptr(), 0), (None, d_prob.data_ptr(), 1), (d_blob.data_ptr(), None, 1)):
        assert net.forward_raw(*args) == _lib.EAO_ERR_INVALID, args[2]
    torch.cuda.synchronize()
    assert (d_prob.cpu().numpy() == 7.0).all()
    out = np.full((32, 32, 12), 9.0, F)
    L = _lib.load()
    for tensor, frame in ((0, 0), (len(model.tensors), 0), (model.tensors.index((85, DN.HEAD, 0, 0)), 0), (1, 2), (1, -1)):
        assert L.eao_detnet_tensor(net._h, tensor, frame, out.ctypes.data) == _lib.EAO_ERR_INVALID and (out == 9.0).all()
    ms = np.full(len(model.ops), -5.0, F)
    assert L.eao_detnet_last_op_ms(net._h, ms.ctypes.data, len(ms)) == _lib.EAO_ERR_INVALID and (ms == -5.0).all()
    net.set_profiling(True)
    net.forward(d_blob.data_ptr(), d_prob.data_ptr(), 2)
    assert L.eao_detnet_last_op_ms(net._h, ms.ctypes.data, len(ms) - 1) == _lib.EAO_ERR_INVALID and (ms == -5.0).all()
    got = net.last_op_ms()
    assert len(got) == len(model.ops) and (got >= 0).all()
    assert M.same_bits(d_prob.cpu().numpy()[1], walked[1][1])


# ---------------------------------------------------------------- 7. the adapter
def test_adapter_from_an_engine_file(DN, tmp_path):
    """include/eaofusion/YOLOXNet.h on the device (tests/cpp/detnet/detnet_driver.cpp linked with the library): YOLOXEngine(path) detects on a frame what the
    reference's order of the host decode gives over the walk's head of the library's own blob"""
    import subprocess
    from eao_fusion_amd import yolox
    exe = str(tmp_path / "detnet_adapter_gpu")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "detnet", "detnet_driver.cpp"),
                           os.path.join(ROOT, "eao_fusion_amd", "libeaofusion_hip.so"), "-Wl,-rpath," + os.path.join(ROOT, "eao_fusion_amd"), "-Wl,-rpath,/opt/rocm/lib",
                           "-L/opt/rocm/lib", "-lamdhip64", "-lpthread", "-o", exe])
    model, _, _ = whole("w05")
    (tmp_path / "yolox.detnet").write_bytes(model.tobytes())
    img = np.random.RandomState(9).randint(0, 256, (40, 57, 3)).astype(np.uint8)
    (tmp_path / "frame.bin").write_bytes(img.tobytes())
    out = subprocess.run([exe, str(tmp_path / "yolox.detnet"), "64", "8192", "57", "40", str(tmp_path / "frame.bin")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-1000:] + out.stderr[-2000:]
    lines = out.stdout.strip().split("\n")
    blob = yolox.Yolox(input_size=64).preprocess(img)[0]
    head = M.walk_run(M.walk_binary(("-O2",)), model, 64, blob)[1]
    want = Y.decode_literal(head, 64, 57, 40)["objects"]
    rows = ["%s %d" % (" ".join("%08x" % v for v in np.array([o["x"], o["y"], o["w"], o["h"], o["prob"]], F).view(np.uint32)), o["label"]) for o in want]
    assert lines[0] == "engine classes 80 anchors 84" and lines[1].startswith("result 1 path ") and lines[2] == "objects %d" % len(want) and len(want) > 0
    assert lines[3:] == rows
