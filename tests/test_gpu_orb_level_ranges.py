"""GPU parity of the ORB blur and description level by level, on either side of every batch-size boundary of the launch schedule.

enqueue() (eao_fusion_amd/csrc/orb.hip) picks a stream schedule from the batch size: the one-launch pyramid up to 32 frames, the k_resize
chain above, FAST and the quad-trees of levels 0-2 on the handle's side stream from 48 to 96 frames, profiled calls with every stage alone.
k_orient_describe finds a pair's level from the per-level keypoint counts and takes a level range; a schedule that blurs and describes
levels 0-2 on the side stream and levels 3-7 on the caller's was measured and rejected (DESIGN_HISTORY.md A0), so every schedule makes one
launch of each over all levels.  The tests are written against the results alone and hold for either form.

Frames are 320 x 240, the smallest size at which all eight levels of the default configuration keep a detection area inside the
19-pixel border.  Which level counts a frame holds is asserted on the CPU ORACLE's keypoints before the GPU runs.  Every comparison
is byte for byte.

An output capacity below a frame's keypoint count cannot be reached through the C ABI: eao_orb_extract_batch_device refuses a
capacity below eao_orb_max_keypoints (the sum of the level capacities) with EAO_ERR_CAPACITY, and a frame never holds more
keypoints than that.  test_split_description_against_oracle asserts the refusal and runs at the smallest capacity accepted, with
poisoned outputs: every byte beyond a frame's count keeps the poison."""
import numpy as np
import pytest
import torch  # (before the library loads, so that both resolve the same HIP runtime)

from eao_fusion_amd import synth

pytestmark = pytest.mark.gpu

CFG = (1000, 1.2, 8, 20, 7)              # (nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST)
NLEVELS, MID = CFG[2], 3                 # levels below MID: FAST and quad-trees on the side stream from 48 to 96 frames
H, W = 240, 320
SEED0 = 61000
SPARSE_SEED0, SEARCH = 62000, 64         # sparse frames (12 large, 30 small rectangles) searched for odd counts on levels 0-2
POISON = 0xAB


def _frame(fid):
    if fid == "flat":
        return np.full((H, W), 77, np.uint8)
    if fid == "corner":      # noise in the top-left 32 x 32 pixels: from level 3 on the patch lies inside the border
        img = np.full((H, W), 77, np.uint8)
        img[:32, :32] = np.random.default_rng(5).integers(0, 256, (32, 32), dtype=np.uint8)
        return img
    if isinstance(fid, tuple):
        return synth.synth_frame(SPARSE_SEED0 + fid[1], W, H, 12, 30)
    return synth.synth_frame(fid, W, H)


class Inputs:
    """Frames by id and the oracle's keypoints, descriptors and blurred levels on them, each computed once per module."""

    def __init__(self, oracle):
        self.orc = oracle.OrbOracle(*CFG)
        self.frames, self.refs, self._odd = {}, {}, None

    def frame(self, fid):
        if fid not in self.frames:
            self.frames[fid] = _frame(fid)
        return self.frames[fid]

    def ref(self, fid):
        """(keypoints, descriptors, blurred levels): a level without keypoints is not blurred by the oracle (None)."""
        if fid not in self.refs:
            kps, desc = self.orc.extract(self.frame(fid))
            self.refs[fid] = (kps.copy(), desc.copy(), [self.orc.level_image(l, blurred=True) for l in range(NLEVELS)])
        return self.refs[fid]

    def counts(self, fid):
        return np.bincount(self.ref(fid)[0]["octave"], minlength=NLEVELS)

    def odd(self):
        """The first sparse frame whose counts on levels 0, 1 and 2 are all odd (none within SEARCH seeds fails the test)."""
        if self._odd is None:
            found = [("sparse", s) for s in range(SEARCH) if (self.counts(("sparse", s))[:MID] % 2 == 1).all()]
            assert found, "no frame with odd counts on levels 0-%d within %d seeds" % (MID - 1, SEARCH)
            self._odd = found[0]
        return self._odd

    def ids(self, B, which=0):
        """Frame ids of batch X (which = 0) or Y (1): textured frames of distinct seeds; from eight frames on a flat frame, the corner frame
        and the odd frame at places that differ between X and Y; the last frame of X is the odd one."""
        ids = [SEED0 + which * 1000 + i for i in range(B)]
        if B >= 8:
            if which == 0:
                ids[1], ids[2], ids[B - 1] = "flat", "corner", self.odd()
            else:
                ids[0], ids[1], ids[2] = self.odd(), "corner", "flat"
        return ids

    def batch(self, ids):
        return np.stack([self.frame(fid) for fid in ids])


@pytest.fixture(scope="module")
def gpu():
    import eao_fusion_amd as E
    assert E.load().eao_device_check() == 0, E.load().eao_last_error()
    return E


@pytest.fixture(scope="module")
def inputs(oracle):
    return Inputs(oracle)


def _check(kps, desc, refs, frames, what):
    bad = [f for f in frames
           if not (len(kps[f]) == len(refs[f][0]) and np.array_equal(kps[f], refs[f][0]) and np.array_equal(desc[f], refs[f][1]))]
    assert not bad, "%s: frames %s differ from the oracle" % (what, bad)


class DeviceCall:
    """eao_orb_extract_batch_device on frames in the caller's layout, outputs poisoned before every call."""

    def __init__(self, gpu, ext, B, cap, pitch=W, shift=0, fstride_extra=0):
        self.gpu, self.ext, self.B, self.cap = gpu, ext, B, cap
        self.pitch, self.shift, self.fstride = pitch, shift, H * pitch + fstride_extra
        self.d_k = torch.empty((B, cap, 28), dtype=torch.uint8, device="cuda")
        self.d_d = torch.empty((B, cap, 32), dtype=torch.uint8, device="cuda")
        self.d_n = torch.empty(B, dtype=torch.int32, device="cuda")
        self.d_img = None

    def upload(self, imgs):
        host = np.zeros(self.shift + (self.B - 1) * self.fstride + H * self.pitch + 8, np.uint8)
        for f in range(self.B):
            o = self.shift + f * self.fstride
            host[o:o + H * self.pitch].reshape(H, self.pitch)[:, :W] = imgs[f]
        self.d_img = torch.from_numpy(host).cuda()      # (kept: the level taps read level 0 from it)

    def run(self):
        """One call; returns the raw output arrays (n, keypoint bytes, descriptor bytes) on the host."""
        self.d_k.fill_(POISON); self.d_d.fill_(POISON); self.d_n.fill_(-1)
        torch.cuda.synchronize()
        self.ext.extract_batch_device(self.d_img.data_ptr() + self.shift, W, H, self.pitch, self.fstride, self.B, self.d_k.data_ptr(),
                                      self.d_d.data_ptr(), self.cap, self.d_n.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return self.d_n.cpu().numpy(), self.d_k.cpu().numpy(), self.d_d.cpu().numpy()

    def split(self, out):
        n, k, d = out
        assert (n >= 0).all() and (n <= self.cap).all(), n
        return [k[f, :n[f]].reshape(-1).view(self.gpu.KP_DTYPE) for f in range(self.B)], [d[f, :n[f]] for f in range(self.B)]


def _assert_poison_beyond_count(out, what):
    n, k, d = out
    bad = [f for f in range(len(n)) if not ((k[f, n[f]:] == POISON).all() and (d[f, n[f]:] == POISON).all())]
    assert not bad, "%s: frames %s have bytes stored beyond their count" % (what, bad)


# ------------------------------------------------------------------------------------------------------------------- blur ranges
BLUR_CASES = [("b48-timed", 48, False, False), ("b48-profiled", 48, True, False), ("b3-unaligned", 3, False, True), ("b8", 8, False, False)]


@pytest.mark.parametrize("name,B,profiled,unaligned", BLUR_CASES, ids=[c[0] for c in BLUR_CASES])
def test_blurred_levels_match_oracle(gpu, inputs, name, B, profiled, unaligned):
    """Every blurred level of every frame, read back through eao_orb_level(which = 1).  Batch 48 timed: the blur on the side stream behind
    the lower levels' quad-trees; batch 48 profiled: alone on the side stream; batch 3 has no frame -> XCD affinity and a level-0 source that
    is not 4-byte aligned (base pointer, pitch and frame stride), batch 8 has the affinity."""
    ids = [SEED0 + i for i in range(B)]      # textured frames: the oracle blurs only the levels that hold keypoints
    refs = [inputs.ref(fid) for fid in ids]
    assert all(b is not None for r in refs for b in r[2]), "a frame has a level without keypoints: the oracle did not blur it"
    ext = gpu.ORBextractor(*CFG)
    ext.set_profiling(profiled)
    call = DeviceCall(gpu, ext, B, ext.max_keypoints(W, H), *((W + 3, 1, 3) if unaligned else ()))
    call.upload(inputs.batch(ids))
    kps, desc = call.split(call.run())
    bad = [(f, l) for f in range(B) for l in range(NLEVELS) if not np.array_equal(ext.level_image(l, f, blurred=True), refs[f][2][l])]
    assert not bad, "%s: blurred (frame, level) %s differ from the oracle" % (name, bad)
    _check(kps, desc, refs, range(B), name)


# ------------------------------------------------------------------------------------------- description by level, frame by frame
@pytest.mark.parametrize("B", [48, 64])
def test_split_description_against_oracle(gpu, inputs, B):
    """Every frame of batches X, Y and X again on one handle against the oracle, at the smallest output capacity the call accepts and with
    poisoned outputs.  The batches hold a flat frame (no pair at all), a frame with keypoints on levels 0-2 only (the side stream's levels:
    nothing above them but the count), a frame with odd counts on levels 0, 1 and 2 (an idle half-wave at the end of each) and textured frames."""
    X, Y = inputs.ids(B, 0), inputs.ids(B, 1)
    cf, cc, co = inputs.counts("flat"), inputs.counts("corner"), inputs.counts(inputs.odd())
    assert cf.sum() == 0 and cc[:MID].sum() > 0 and cc[MID:].sum() == 0 and (co[:MID] % 2 == 1).all() and co[MID:].sum() > 0, (cf, cc, co)
    assert all(x != y for x, y in zip(X, Y))
    ext = gpu.ORBextractor(*CFG)
    cap = ext.max_keypoints(W, H)
    call = DeviceCall(gpu, ext, B, cap)
    call.upload(inputs.batch(X))
    with pytest.raises(gpu._lib.EaoError) as err:      # a capacity that could cut a frame's keypoints short is refused
        ext.extract_batch_device(call.d_img.data_ptr(), W, H, W, H * W, B, call.d_k.data_ptr(), call.d_d.data_ptr(), cap - 1, call.d_n.data_ptr(),
                                 torch.cuda.current_stream().cuda_stream)
    assert err.value.status == gpu._lib.EAO_ERR_CAPACITY
    for what, ids in (("X", X), ("Y", Y), ("X again", X)):
        refs = [inputs.ref(fid) for fid in ids]
        call.upload(inputs.batch(ids))
        out = call.run()
        kps, desc = call.split(out)
        _check(kps, desc, refs, range(B), "batch %d, %s" % (B, what))
        _assert_poison_beyond_count(out, "batch %d, %s" % (B, what))


# ------------------------------------------------------------------------------------------------------ profiled against timed
@pytest.mark.parametrize("B", [48, 64])
def test_profiled_and_timed_calls_agree(gpu, inputs, B):
    """The same batch by the timed schedule, by a profiled call (stages one after the other) and by two
    more timed calls on the same handle, whose scratch is reused: the same bytes in d_n, d_kps and d_desc every time (the outputs are
    poisoned before each call, so the arrays are compared whole), and the oracle's in the first and the last frame."""
    X, Y = inputs.ids(B, 0), inputs.ids(B, 1)
    ext = gpu.ORBextractor(*CFG)
    call = DeviceCall(gpu, ext, B, ext.max_keypoints(W, H))
    call.upload(inputs.batch(Y))
    call.run()                                 # (another batch first: X's results are not what the scratch already holds)
    call.upload(inputs.batch(X))
    timed = call.run()
    ext.set_profiling(True)
    profiled = call.run()
    ext.set_profiling(False)
    again = [call.run(), call.run()]
    for what, out in [("profiled", profiled), ("second timed", again[0]), ("third timed", again[1])]:
        for name, a, b in zip(("d_n", "d_kps", "d_desc"), out, timed):
            assert np.array_equal(a, b), "batch %d: %s of the %s call differs from the first timed call's" % (B, name, what)
    _assert_poison_beyond_count(timed, "batch %d" % B)
    kps, desc = call.split(timed)
    _check(kps, desc, [inputs.ref(fid) if f in (0, B - 1) else None for f, fid in enumerate(X)], (0, B - 1), "batch %d, timed" % B)


# ------------------------------------------------------------------------------------------------------- schedule boundaries
@pytest.mark.parametrize("B", [32, 40, 47, 48, 96, 104])
def test_either_side_of_schedule_boundaries(gpu, inputs, B):
    """32 / 40: the one-launch pyramid and the k_resize chain; 47 / 48: the first batch with levels 0-2 on the side stream; 96 / 104: the last
    one.  The first frame (textured) and the last (odd counts on levels 0-2) against the oracle, batches X, Y, X on one handle."""
    X, Y = inputs.ids(B, 0), inputs.ids(B, 1)
    ext = gpu.ORBextractor(*CFG)
    for what, ids in (("X", X), ("Y", Y), ("X again", X)):
        kps, desc = ext.extract_batch(inputs.batch(ids))
        refs = [inputs.ref(fid) if f in (0, B - 1) else None for f, fid in enumerate(ids)]
        _check(kps, desc, refs, (0, B - 1), "batch %d, %s" % (B, what))
