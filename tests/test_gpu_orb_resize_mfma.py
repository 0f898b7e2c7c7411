"""The chained pyramid on the matrix cores (k_resize_mfma, eao_fusion_amd/csrc/orb_resize_mfma.hip) against the 11-bit fixed-point bilinear formula, byte for byte.

Reference: a numpy restatement of the formula (H = S[sx] a0 + S[sx + 1] a1 with clamped columns and zeroed edge weights; out = ((b0 (H[sy0] >> 4)) >> 16 +
(b1 (H[sy1] >> 4)) >> 16 + 2) >> 2 with rows clamped at the load and their weights kept) applied to the level BELOW as read back from the device, so every level of
every frame is judged on its own.

Frames are 320 x 240 in the default configuration: level widths 320, 267, 222, 185, 154, 129, 107, 89 -- every kind of right-edge remainder of the 32-pixel column
strips, 129 = 4 * 32 + 1 among them.  Every batch holds a synthetic frame, an all-0 frame, an all-255 frame (the largest H), a 0 / 255 checkerboard, 0 / 255 noise and
vertical 0 / 255 stripes (the largest column excursions).  The chained pyramid runs only above 32 frames: 40 frames have the frame -> XCD affinity and the plain
schedule, 35 have no affinity, 48 have FAST of levels 1-2 waiting on the level-2 resize.  A layout with pitch W + 3 and base + 1 sends level 1 through k_resize inside
the same call and levels 2-7 through the matrix cores; a 96 x 76 handle with two levels at 33 frames has a top level (80 x 63) smaller than a tile row of 96 pixels.
EAO_ORB_RESIZE_MFMA=0 in a fresh process gives the same raw levels, blurred levels, keypoints and descriptors."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = (1000, 1.2, 8, 20, 7)
H, W = 240, 320
LEVEL_SIZES = [(320, 240), (267, 200), (222, 167), (185, 139), (154, 116), (129, 96), (107, 80), (89, 67)]
SMALL = dict(cfg=(300, 1.2, 2, 20, 7), W=96, H=76, sizes=[(96, 76), (80, 63)])
KINDS = ("synthetic", "zeros", "full", "checker", "noise", "stripes")


def numpy_resize(src, dw, dh):
    sh, sw = src.shape

    def coef(dn, sn):
        inv = 1.0 / (float(dn) / sn)
        f = ((np.arange(dn) + 0.5) * inv - 0.5).astype(np.float32)
        i = np.floor(f).astype(np.int64)
        return i, (f - i.astype(np.float32)).astype(np.float32)

    def weights(f):
        return np.rint((np.float32(1) - f) * np.float32(2048)).astype(np.int64), np.rint(f * np.float32(2048)).astype(np.int64)

    ix, fx = coef(dw, sw)
    fx[ix < 0] = 0
    ix[ix < 0] = 0
    fx[ix >= sw - 1] = 0
    ix[ix >= sw - 1] = sw - 1
    iy, fy = coef(dh, sh)
    (a0, a1), (b0, b1) = weights(fx), weights(fy)
    S = src.astype(np.int64)
    Hh = S[:, ix] * a0 + S[:, np.minimum(ix + 1, sw - 1)] * a1
    y0, y1 = np.clip(iy, 0, sh - 1), np.clip(iy + 1, 0, sh - 1)
    v = (((b0[:, None] * (Hh[y0] >> 4)) >> 16) + ((b1[:, None] * (Hh[y1] >> 4)) >> 16) + 2) >> 2
    assert v.min() >= 0 and v.max() <= 255      # (weights >= 0, pairs sum to 2048: the formula needs no clamp)
    return v.astype(np.uint8)


def frame(kind, w=W, h=H, seed=0):
    from eao_fusion_amd import synth
    if kind == "synthetic":
        return synth.synth_frame(73000 + seed, w, h)
    if kind == "zeros":
        return np.zeros((h, w), np.uint8)
    if kind == "full":
        return np.full((h, w), 255, np.uint8)
    if kind == "checker":
        return (((np.add.outer(np.arange(h), np.arange(w)) + seed) & 1) * 255).astype(np.uint8)
    if kind == "stripes":
        return np.broadcast_to((((np.arange(w) + seed) & 1) * 255).astype(np.uint8), (h, w)).copy()
    return (np.random.default_rng(74000 + seed).integers(0, 2, (h, w)) * 255).astype(np.uint8)


def batch(n, w=W, h=H):
    """n frames: the six kinds, again and again with other seeds."""
    return np.stack([frame(KINDS[i % len(KINDS)], w, h, seed=i // len(KINDS)) for i in range(n)])


def run_device(ext, imgs, pitch=None, shift=0):
    """One eao_orb_extract_batch_device call on frames laid out with `pitch` and `shift`; returns (keypoints, descriptors, keeper of the device image)."""
    import torch
    B, h, w = imgs.shape
    pitch = pitch or w
    fstride = h * pitch + (3 if shift else 0)
    host = np.zeros(shift + (B - 1) * fstride + h * pitch + 8, np.uint8)
    for f in range(B):
        o = shift + f * fstride
        host[o:o + h * pitch].reshape(h, pitch)[:, :w] = imgs[f]
    d_img = torch.from_numpy(host).cuda()
    cap = ext.max_keypoints(w, h)
    d_k = torch.zeros((B, cap, 28), dtype=torch.uint8, device="cuda")
    d_d = torch.zeros((B, cap, 32), dtype=torch.uint8, device="cuda")
    d_n = torch.zeros(B, dtype=torch.int32, device="cuda")
    ext.extract_batch_device(d_img.data_ptr() + shift, w, h, pitch, fstride, B, d_k.data_ptr(), d_d.data_ptr(), cap, d_n.data_ptr(),
                             torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    n, k, d = d_n.cpu().numpy(), d_k.cpu().numpy(), d_d.cpu().numpy()
    return [k[f, :n[f]].copy() for f in range(B)], [d[f, :n[f]].copy() for f in range(B)], d_img


def levels(ext, B, nlevels, blurred):
    return [[ext.level_image(l, f, blurred=blurred) for l in range(nlevels)] for f in range(B)]


def assert_pyramid(ext, imgs, nlevels, sizes, what):
    B = len(imgs)
    raw = levels(ext, B, nlevels, False)
    assert [r.shape[::-1] for r in raw[0]] == sizes, [r.shape for r in raw[0]]
    assert all(np.array_equal(raw[f][0], imgs[f]) for f in range(B)), "%s: level 0 is not the input" % what
    bad = [(f, l) for f in range(B) for l in range(1, nlevels) if not np.array_equal(raw[f][l], numpy_resize(raw[f][l - 1], *sizes[l]))]
    assert not bad, "%s: (frame, level) %s differ from the formula applied to the level below" % (what, bad)
    return raw


if __name__ != "__main__":
    pytestmark = pytest.mark.gpu

    @pytest.fixture(scope="module")
    def gpu():
        import torch  # noqa: F401  (before the library loads, so that both resolve the same HIP runtime)
        import eao_fusion_amd as E
        assert E.load().eao_device_check() == 0, E.load().eao_last_error()
        assert os.environ.get("EAO_ORB_RESIZE_MFMA", "1") != "0", "this module tests the matrix-core resize: EAO_ORB_RESIZE_MFMA=0 is set"
        return E


def test_numpy_resize_extremes(gpu):
    """The reference itself: constant images stay constant at every level size (every weight pair sums to 2048)."""
    for w, h in LEVEL_SIZES[1:]:
        assert (numpy_resize(np.full((H, W), 255, np.uint8), w, h) == 255).all() and (numpy_resize(np.zeros((H, W), np.uint8), w, h) == 0).all()


@pytest.mark.parametrize("n,what", [(40, "40 frames: affinity, plain schedule"), (35, "35 frames: no affinity"), (48, "48 frames: FAST of levels 1-2 behind evMid")],
                         ids=["batch40", "batch35", "batch48"])
def test_chained_pyramid(gpu, n, what):
    imgs = batch(n)
    ext = gpu.ORBextractor(*CFG)
    keep = run_device(ext, imgs)      # (the level taps read level 0 from the device image)
    assert_pyramid(ext, imgs, CFG[2], LEVEL_SIZES, what)
    del keep


def test_unaligned_level0(gpu):
    """Pitch W + 3, base shifted by one byte, frame stride odd: level 1 reads the caller's image and takes k_resize, levels 2-7 the matrix cores, in one call."""
    imgs = batch(33)
    ext = gpu.ORBextractor(*CFG)
    keep = run_device(ext, imgs, W + 3, 1)
    assert_pyramid(ext, imgs, CFG[2], LEVEL_SIZES, "33 frames, unaligned")
    del keep


def test_top_level_smaller_than_a_tile_row(gpu):
    """96 x 76, two levels, 33 frames: level 1 is 80 x 63 -- three column strips, the last one half empty, two row blocks, the last one a row short."""
    w, h = SMALL["W"], SMALL["H"]
    imgs = batch(33, w, h)
    ext = gpu.ORBextractor(*SMALL["cfg"])
    keep = run_device(ext, imgs)
    assert_pyramid(ext, imgs, 2, SMALL["sizes"], "96 x 76")
    del keep


def test_switch_changes_no_result(gpu, tmp_path):
    """The batch of 40 with EAO_ORB_RESIZE_MFMA=0 in a fresh process (the switch is read once): identical raw and blurred levels, keypoints, descriptors."""
    imgs = batch(40)
    ext = gpu.ORBextractor(*CFG)
    kps, desc, keep = run_device(ext, imgs)
    raw, blr = levels(ext, len(imgs), CFG[2], False), levels(ext, len(imgs), CFG[2], True)
    out = str(tmp_path / "valu.npz")
    env = dict(os.environ, EAO_ORB_RESIZE_MFMA="0", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    run = subprocess.run([sys.executable, os.path.abspath(__file__), out], capture_output=True, text=True, timeout=300, env=env)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    z = np.load(out)
    assert sum(len(k) for k in kps) > 100, "the batch holds too few keypoints to say anything"
    for f in range(len(imgs)):
        assert np.array_equal(z["kps%d" % f], kps[f]) and np.array_equal(z["desc%d" % f], desc[f]), "frame %d: keypoints or descriptors differ" % f
        for l in range(CFG[2]):
            assert np.array_equal(z["raw%d_%d" % (f, l)], raw[f][l]), "raw level %d of frame %d differs" % (l, f)
            assert np.array_equal(z["blur%d_%d" % (f, l)], blr[f][l]), "blurred level %d of frame %d differs" % (l, f)


if __name__ == "__main__":      # the child of test_switch_changes_no_result
    import torch  # noqa: F401
    import eao_fusion_amd as E
    assert os.environ.get("EAO_ORB_RESIZE_MFMA") == "0"
    imgs = batch(40)
    ext = E.ORBextractor(*CFG)
    kps, desc, keep = run_device(ext, imgs)
    raw, blr = levels(ext, len(imgs), CFG[2], False), levels(ext, len(imgs), CFG[2], True)
    arrays = {}
    for f in range(len(imgs)):
        arrays["kps%d" % f], arrays["desc%d" % f] = kps[f], desc[f]
        for l in range(CFG[2]):
            arrays["raw%d_%d" % (f, l)], arrays["blur%d_%d" % (f, l)] = raw[f][l], blr[f][l]
    np.savez(sys.argv[1], **arrays)
