"""The 7 x 7 blur on the matrix cores (k_blur7_mfma, eao_fusion_amd/csrc/orb.hip) against the plain integer blur, byte for byte.

Reference: the numpy blur of tests/test_oracle_orb.py::test_gaussian_blur_vs_numpy applied to the RAW level read back from the device, so every
level of every frame is held, whether it holds keypoints or not, and the resize chain plays no part in the verdict.

Frames are 320 x 240 in the default configuration: level widths 320, 267, 222, 185, 154, 129, 107, 89 -- every kind of right-edge remainder of the
32-pixel column strips, 129 = 4 * 32 + 1 among them -- and heights 240 ... 67.  Every batch holds a synthetic frame, an all-0 frame, an all-255 frame
(the only input whose sum reaches 257 before the saturation), a 0 / 255 checkerboard and 0 / 255 noise (the largest signed excursions of both products).
Batch 8 has the frame -> XCD affinity, batch 3 has none (two calls hold the five inputs); batch 3 in a layout that is not 4-byte aligned sends
level 0 through the VALU strips inside the same launch and levels 1-7 through the matrix cores; a 96 x 76 frame with two levels has its top level
(80 x 63) below the 64-row source window: level 0 on the matrix cores, level 1 on the VALU strips.  (72 x 60 with two levels is refused by the
handle: its 60 x 50 top level holds no FAST cell.)  EAO_ORB_BLUR_MFMA=0 in a fresh process gives the same blurred levels, keypoints and descriptors."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = (1000, 1.2, 8, 20, 7)
H, W = 240, 320
SMALL = dict(cfg=(300, 1.2, 2, 20, 7), W=96, H=76, sizes=[(96, 76), (80, 63)])
KINDS = ("synthetic", "zeros", "full", "checker", "noise")


def numpy_blur(img):
    k = np.array([18, 34, 49, 55, 49, 34, 18], np.int64)
    h, w = img.shape
    pad = np.pad(img.astype(np.int64), 3, mode="reflect")      # numpy 'reflect' == BORDER_REFLECT_101
    rows = sum(k[t] * pad[:, t:t + w] for t in range(7))
    out = sum(k[t] * rows[t:t + h, :] for t in range(7))
    return np.clip((out + 32768) >> 16, 0, 255).astype(np.uint8)


def frame(kind, w=W, h=H, seed=0):
    from eao_fusion_amd import synth
    if kind == "synthetic":
        return synth.synth_frame(71000 + seed, w, h)
    if kind == "zeros":
        return np.zeros((h, w), np.uint8)
    if kind == "full":
        return np.full((h, w), 255, np.uint8)
    if kind == "checker":
        return (((np.add.outer(np.arange(h), np.arange(w))) & 1) * 255).astype(np.uint8)
    return (np.random.default_rng(72000 + seed).integers(0, 2, (h, w)) * 255).astype(np.uint8)


def batch8():
    return np.stack([frame(k) for k in KINDS] + [frame("noise", seed=1), frame("synthetic", seed=1), frame("checker")[::-1].copy()])


def run_device(E, ext, imgs, pitch=None, shift=0):
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


def assert_blur(ext, imgs, nlevels, sizes, what):
    B = len(imgs)
    raw, blr = levels(ext, B, nlevels, False), levels(ext, B, nlevels, True)
    assert [r.shape[::-1] for r in raw[0]] == sizes, [r.shape for r in raw[0]]
    assert all(np.array_equal(raw[f][0], imgs[f]) for f in range(B)), "%s: level 0 is not the input" % what
    bad = [(f, l) for f in range(B) for l in range(nlevels) if not np.array_equal(blr[f][l], numpy_blur(raw[f][l]))]
    assert not bad, "%s: blurred (frame, level) %s differ from the integer blur of the raw level" % (what, bad)
    return blr


LEVEL_SIZES = [(320, 240), (267, 200), (222, 167), (185, 139), (154, 116), (129, 96), (107, 80), (89, 67)]

if __name__ != "__main__":
    pytestmark = pytest.mark.gpu

    @pytest.fixture(scope="module")
    def gpu():
        import torch  # noqa: F401  (before the library loads, so that both resolve the same HIP runtime)
        import eao_fusion_amd as E
        assert E.load().eao_device_check() == 0, E.load().eao_last_error()
        assert os.environ.get("EAO_ORB_BLUR_MFMA", "1") != "0", "this module tests the matrix-core blur: EAO_ORB_BLUR_MFMA=0 is set"
        return E


def test_numpy_blur_saturates(gpu):
    """The reference itself: an all-255 image sums to 257 before the clamp, the taps sum to 257."""
    assert (numpy_blur(np.full((9, 9), 255, np.uint8)) == 255).all() and (numpy_blur(np.zeros((9, 9), np.uint8)) == 0).all()
    assert ((257 * 257 * 255 + 32768) >> 16) == 257


def test_batch8_frame_affinity(gpu):
    imgs = batch8()
    ext = gpu.ORBextractor(*CFG)
    keep = run_device(gpu, ext, imgs)      # (the level taps read level 0 from the device image)
    assert_blur(ext, imgs, CFG[2], LEVEL_SIZES, "batch 8")
    del keep


@pytest.mark.parametrize("unaligned", [False, True], ids=["aligned", "unaligned-level0"])
def test_batch3_no_affinity(gpu, unaligned):
    """Two calls on one handle hold the five inputs.  Unaligned: pitch W + 3, base shifted by one byte, frame stride odd -- level 0 takes the VALU strips
    of the same launch, levels 1-7 the matrix cores."""
    ext = gpu.ORBextractor(*CFG)
    for kinds in (KINDS[:3], KINDS[3:] + ("synthetic",)):
        imgs = np.stack([frame(k, seed=2) for k in kinds])
        keep = run_device(gpu, ext, imgs, *((W + 3, 1) if unaligned else ()))      # (the level taps read level 0 from the device image)
        assert_blur(ext, imgs, CFG[2], LEVEL_SIZES, "batch 3 %s %s" % ("unaligned" if unaligned else "aligned", kinds))


def test_top_level_below_source_window(gpu):
    """96 x 76, two levels: level 1 is 80 x 63, lower than the 64-row source window -> VALU strips; level 0 on the matrix cores."""
    w, h = SMALL["W"], SMALL["H"]
    imgs = np.stack([frame(k, w, h, seed=3) for k in KINDS])
    ext = gpu.ORBextractor(*SMALL["cfg"])
    keep = run_device(gpu, ext, imgs)      # (the level taps read level 0 from the device image)
    assert_blur(ext, imgs, 2, SMALL["sizes"], "96 x 76")


def test_switch_changes_no_result(gpu, tmp_path):
    """The same batch of eight with EAO_ORB_BLUR_MFMA=0 in a fresh process (the switch is read once): identical blurred levels, keypoints, descriptors."""
    imgs = batch8()
    ext = gpu.ORBextractor(*CFG)
    kps, desc, keep = run_device(gpu, ext, imgs)
    blr = levels(ext, len(imgs), CFG[2], True)
    out = str(tmp_path / "valu.npz")
    env = dict(os.environ, EAO_ORB_BLUR_MFMA="0", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    run = subprocess.run([sys.executable, os.path.abspath(__file__), out], capture_output=True, text=True, timeout=300, env=env)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    z = np.load(out)
    assert sum(len(k) for k in kps) > 100, "the batch holds too few keypoints to say anything"
    for f in range(len(imgs)):
        assert np.array_equal(z["kps%d" % f], kps[f]) and np.array_equal(z["desc%d" % f], desc[f]), "frame %d: keypoints or descriptors differ" % f
        for l in range(CFG[2]):
            assert np.array_equal(z["blur%d_%d" % (f, l)], blr[f][l]), "blurred level %d of frame %d differs" % (l, f)


if __name__ == "__main__":      # the child of test_switch_changes_no_result
    import torch  # noqa: F401
    import eao_fusion_amd as E
    assert os.environ.get("EAO_ORB_BLUR_MFMA") == "0"
    imgs = batch8()
    ext = E.ORBextractor(*CFG)
    kps, desc, keep = run_device(E, ext, imgs)
    blr = levels(ext, len(imgs), CFG[2], True)
    arrays = {}
    for f in range(len(imgs)):
        arrays["kps%d" % f], arrays["desc%d" % f] = kps[f], desc[f]
        for l in range(CFG[2]):
            arrays["blur%d_%d" % (f, l)] = blr[f][l]
    np.savez(sys.argv[1], **arrays)
