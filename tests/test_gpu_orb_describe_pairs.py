"""GPU parity of k_orient_describe's two-keypoints-per-wavefront layout on irregular level counts.

The kernel (eao_fusion_amd/csrc/orb.hip) gives a wavefront the keypoints 2p and 2p + 1 of ONE level, one per half-wave: a level
with an odd count leaves the upper half of its last wave idle, a level with one keypoint is that case alone, an empty level
below a populated one moves the pair -> level map, and a flat frame has no pair at all.  The frames here are sparse on purpose
(a few small rectangles on a flat background) so that a four-level pyramid with a small nfeatures holds such counts; which
counts it holds is asserted on the CPU ORACLE's keypoints before the GPU runs, so no case depends on the GPU for its premise.

Every call is held to the oracle bit for bit.  Batches 1, 3 and 8: 3 has no frame -> XCD affinity, 8 has it.  Frames of
320 x 240 and of 107 x 107, the smallest size this configuration accepts (its top level is then one 30 px FAST cell plus borders).
Each case runs X, Y, X on one handle (the handle's level-keypoint scratch is never cleared), and the device-API cases poison
the output arrays before every call: a half-wave that silently stored nothing leaves the poison (or the previous call's row) behind."""
import numpy as np
import pytest
import torch  # (before the library loads, so that both resolve the same HIP runtime)

pytestmark = pytest.mark.gpu

CFG = (60, 1.2, 4, 20, 7)                # (nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST)
NLEVELS = CFG[2]
BIG, SMALLEST = (240, 320), (107, 107)   # (height, width)

# sparse_frame recipes: (rectangles, smallest edge, largest edge, smallest contrast, largest contrast, 3x3 box blurs)
DOTS, SPECKS, BLOBS, MIXED = (3, 1, 2, 25, 40, 0), (6, 2, 6, 30, 120, 0), (4, 8, 20, 30, 100, 2), (10, 1, 10, 25, 150, 1)
ONE = (1, 1, 3, 25, 60, 0)
# the frames that fill a batch of eight next to the ones chosen by their level counts (Inputs.roles): (seed, recipe)
OTHERS = [(0, MIXED), (2, SPECKS), (2, DOTS), (6, MIXED), (3, DOTS), (1, SPECKS)]
SEARCH = 64                              # seeds tried per recipe when a frame is chosen by its level counts


def sparse_frame(shape, seed, recipe):
    """A flat background (96) with a few axis-aligned rectangles at least 20 px from the border, box-blurred `blur` times."""
    h, w = shape
    n, smin, smax, cmin, cmax, blur = recipe
    rng = np.random.default_rng(seed)
    img = np.full((h, w), 96, np.int32)
    for _ in range(n):
        bw, bh = rng.integers(smin, smax + 1, 2)
        x, y = rng.integers(20, w - 20 - bw), rng.integers(20, h - 20 - bh)
        c = int(rng.integers(cmin, cmax + 1)) * (1 if rng.integers(0, 2) else -1)
        img[y:y + bh, x:x + bw] = 96 + c
    for _ in range(blur):
        pad = np.pad(img, 1, mode="edge")
        acc = np.zeros_like(img)
        for dy in range(3):
            for dx in range(3):
                acc += pad[dy:dy + h, dx:dx + w]
        img = (acc + 4) // 9
    return np.clip(img, 0, 255).astype(np.uint8)


def batch_ids(roles, B, which):
    """Frame ids of batch X (which = 0) or Y (1): the two differ in every frame."""
    o = OTHERS
    if B == 1:
        return [roles["all4"]] if which == 0 else [roles["alt"]]
    if B == 3:
        return [roles["all4"], "flat", roles["single"]] if which == 0 else [roles["single"], roles["alt"], "flat"]
    assert B == 8
    return [roles["all4"], "flat", roles["single"]] + o[:5] if which == 0 else [o[5], roles["alt"], "flat", roles["single"]] + o[:4]


class Inputs:
    """Frames by (shape, width kept, id) and the oracle's results on them, each computed once per module."""

    def __init__(self, oracle):
        self.orc = oracle.OrbOracle(*CFG)
        self.frames, self.refs, self.chosen = {}, {}, {}

    def frame(self, shape, crop, fid):
        key = (shape, crop, fid)
        if key not in self.frames:
            h, w = shape
            img = np.full((h, w), 96, np.uint8) if fid == "flat" else sparse_frame(shape, *fid)
            self.frames[key] = np.ascontiguousarray(img[:, :w - crop])
        return self.frames[key]

    def ref(self, shape, crop, fid):
        key = (shape, crop, fid)
        if key not in self.refs:
            kps, desc = self.orc.extract(self.frame(shape, crop, fid))
            self.refs[key] = (kps.copy(), desc.copy())
        return self.refs[key]

    def counts(self, shape, crop, fid):
        return np.bincount(self.ref(shape, crop, fid)[0]["octave"], minlength=NLEVELS)

    def roles(self, shape, crop):
        """The frames chosen by the ORACLE's level counts, on the CPU: `all4` holds an empty level below populated ones, a level of exactly
        one keypoint, an even and an odd (>= 3) level in ONE frame; `alt` is another such frame with a different total; `single` keeps
        all its keypoints on one level.  The first seeds that qualify; none within SEARCH seeds fails the test (it is not skipped)."""
        key = (shape, crop)
        if key not in self.chosen:
            cands = [(seed, r) for seed in range(SEARCH) for r in (SPECKS, DOTS) if (seed, r) not in OTHERS]
            full = [fid for fid in cands if all(level_count_properties([self.counts(shape, crop, fid)])[k] for k in ("odd", "even", "one", "hole"))]
            assert full, "no frame with an odd, an even, a one-keypoint and an empty level within %d seeds" % SEARCH
            alt = [fid for fid in full[1:] if self.counts(shape, crop, fid).sum() != self.counts(shape, crop, full[0]).sum()]
            single = [(seed, ONE) for seed in range(SEARCH) if level_count_properties([self.counts(shape, crop, (seed, ONE))])["single"]]
            assert alt and single, "no second irregular frame / no one-level frame within %d seeds" % SEARCH
            self.chosen[key] = dict(all4=full[0], alt=alt[0], single=single[0])
        return self.chosen[key]


def level_count_properties(per_frame):
    """What the per-level keypoint counts of a batch's frames (a list of arrays) offer the kernel."""
    levels = [int(c) for cnt in per_frame for c in cnt]
    return dict(odd=any(c % 2 == 1 and c > 1 for c in levels),
                even=any(c % 2 == 0 and c > 0 for c in levels),
                one=any(c == 1 for c in levels),
                hole=any(cnt[l] == 0 and cnt[l + 1:].sum() > 0 for cnt in per_frame for l in range(NLEVELS - 1)),
                flat=any(cnt.sum() == 0 for cnt in per_frame),
                single=any(cnt.sum() > 0 and (cnt > 0).sum() == 1 for cnt in per_frame))


def assert_preconditions(inputs, shape, crop, B):
    """On the ORACLE's counts: batch X holds an odd level (three or more), an even one, a level of exactly one keypoint and an empty
    level below a populated one; from three frames on also a flat frame and a frame whose keypoints are all on one level.  (A single
    frame cannot be flat and hold keypoints: batch 1 runs the flat and the single-level frame as calls of their own.)"""
    roles = inputs.roles(shape, crop)
    X, Y = batch_ids(roles, B, 0), batch_ids(roles, B, 1)
    assert len(X) == len(Y) == B and all(x != y for x, y in zip(X, Y))
    prop = level_count_properties([inputs.counts(shape, crop, fid) for fid in X])
    need = ["odd", "even", "one", "hole"] + (["flat", "single"] if B >= 3 else [])
    assert all(prop[k] for k in need), "inputs do not hold the level counts this test is about: %s" % prop
    # X and Y differ in the rows a call leaves behind: some frame slot has MORE keypoints in X than in Y and some slot fewer
    nx = [len(inputs.ref(shape, crop, fid)[0]) for fid in X]
    ny = [len(inputs.ref(shape, crop, fid)[0]) for fid in Y]
    assert any(a != b for a, b in zip(nx, ny))
    extra = [roles["single"], "flat"] if B == 1 else []
    if extra:
        pe = level_count_properties([inputs.counts(shape, crop, fid) for fid in extra])
        assert pe["flat"] and pe["single"], pe
    return X, Y, extra


@pytest.fixture(scope="module")
def gpu():
    import eao_fusion_amd as E
    assert E.load().eao_device_check() == 0, E.load().eao_last_error()
    return E


@pytest.fixture(scope="module")
def inputs(oracle):
    return Inputs(oracle)


def _check(kps, desc, refs, what):
    bad = [f for f, (okps, odesc) in enumerate(refs)
           if not (len(kps[f]) == len(okps) and np.array_equal(kps[f], okps) and np.array_equal(desc[f], odesc))]
    assert not bad, "%s: frames %s of %d differ from the oracle" % (what, bad, len(refs))


def _calls(X, Y, extra):
    return [("X", X), ("Y", Y), ("X again", X)] + [("extra %d" % i, [fid]) for i, fid in enumerate(extra)]


def test_smallest_size_is_the_smallest(gpu):
    """107 x 107 is accepted; one pixel less in either direction is not (the top level would be smaller than one FAST cell plus borders)."""
    h, w = SMALLEST
    assert gpu.ORBextractor(*CFG).max_keypoints(w, h) > 0
    for ww, hh in ((w - 1, h), (w, h - 1)):
        with pytest.raises(Exception):
            gpu.ORBextractor(*CFG).max_keypoints(ww, hh)


@pytest.mark.parametrize("B", [1, 3, 8])
@pytest.mark.parametrize("shape", [BIG, SMALLEST], ids=["320x240", "107x107"])
def test_irregular_level_counts(gpu, inputs, shape, B):
    """Odd, even, single-keypoint and empty levels, a flat frame and a one-level frame through the host API: X, Y, X on one handle."""
    X, Y, extra = assert_preconditions(inputs, shape, 0, B)
    ext = gpu.ORBextractor(*CFG)
    for what, ids in _calls(X, Y, extra):
        imgs = np.stack([inputs.frame(shape, 0, fid) for fid in ids])
        kps, desc = ext.extract_batch(imgs)
        _check(kps, desc, [inputs.ref(shape, 0, fid) for fid in ids], "%dx%d batch %d, %s" % (shape[1], shape[0], B, what))


def _device_calls(gpu, inputs, shape, crop, B, pitch, shift, fstride_extra, what0):
    X, Y, extra = assert_preconditions(inputs, shape, crop, B)
    h, w = shape[0], shape[1] - crop
    fstride = h * pitch + fstride_extra
    ext = gpu.ORBextractor(*CFG)
    cap = ext.max_keypoints(w, h)
    d_k = torch.empty((B, cap, 28), dtype=torch.uint8, device="cuda")
    d_d = torch.empty((B, cap, 32), dtype=torch.uint8, device="cuda")
    d_n = torch.empty(B, dtype=torch.int32, device="cuda")
    for what, ids in _calls(X, Y, extra):
        nb = len(ids)
        host = np.zeros(shift + (nb - 1) * fstride + h * pitch + 8, np.uint8)
        for f, fid in enumerate(ids):
            o = shift + f * fstride
            host[o:o + h * pitch].reshape(h, pitch)[:, :w] = inputs.frame(shape, crop, fid)
        d_img = torch.from_numpy(host).cuda()
        d_k.fill_(0xAB); d_d.fill_(0xAB); d_n.fill_(-1)      # poison: a row that was not stored is not a row of the oracle's
        torch.cuda.synchronize()
        ext.extract_batch_device(d_img.data_ptr() + shift, w, h, pitch, fstride, nb, d_k.data_ptr(), d_d.data_ptr(), cap, d_n.data_ptr(),
                                 torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        n, k, d = d_n.cpu().numpy(), d_k.cpu().numpy(), d_d.cpu().numpy()
        assert (n[:nb] >= 0).all() and (n[:nb] <= cap).all(), n
        kps = [k[f, :n[f]].reshape(-1).view(gpu.KP_DTYPE) for f in range(nb)]
        _check(kps, [d[f, :n[f]] for f in range(nb)], [inputs.ref(shape, crop, fid) for fid in ids], "%s, batch %d, %s" % (what0, B, what))
        # ... and nothing was stored past a frame's count
        assert all((k[f, n[f]:] == 0xAB).all() and (d[f, n[f]:] == 0xAB).all() for f in range(nb)), "%s, batch %d, %s: rows past the count" % (what0, B, what)


@pytest.mark.parametrize("B", [1, 3, 8])
@pytest.mark.parametrize("shape,crop", [(BIG, 1), (SMALLEST, 0)], ids=["319x240", "107x107"])
def test_irregular_level_counts_unaligned_input(gpu, inputs, shape, crop, B):
    """The same through eao_orb_extract_batch_device on frames in the caller's layout -- an odd width and pitch, a base pointer and a frame
    stride that are not 4-byte aligned: level 0's raw window is then staged with byte loads."""
    w = shape[1] - crop
    assert w % 2 == 1
    _device_calls(gpu, inputs, shape, crop, B, pitch=w + 2, shift=1, fstride_extra=3, what0="unaligned device API %dx%d" % (w, shape[0]))


@pytest.mark.parametrize("B", [1, 3, 8])
def test_no_stale_rows_behind_idle_half_waves(gpu, inputs, B):
    """X, Y, X through the device API on aligned frames with poisoned outputs: every row up to a frame's count is the oracle's (not the poison,
    not the previous call's), and no row past it was touched."""
    _device_calls(gpu, inputs, BIG, 0, B, pitch=BIG[1], shift=0, fstride_extra=0, what0="aligned device API")
