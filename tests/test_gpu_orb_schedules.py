"""GPU parity of every ORB launch schedule, frame by frame.

enqueue() (eao_fusion_amd/csrc/orb.hip) does not run one pipeline: from the batch size, the level count, whether the one-launch
pyramid fits (build_geometry, orb_host.hip) and whether the call is profiled it picks a stream schedule, each with its own
cross-stream events and its own split of the FAST cells and of the quad-tree levels between the caller's stream and the handle's
side stream; launch_quadtree (orb_quadtree.hip) picks the k_quadtree workgroup size from the batch.  CASES reaches every schedule
and both sides of every switch.

Each case runs two batches X and Y of the same size and of different frames, then X again, on ONE handle: the scratch arrays
(pyramid, cell counts and candidates, level keypoints and counts) are never cleared, so a stage that silently did not run, or ran
on the wrong frames, leaves the previous call's results behind, and those differ from this call's in every frame.  Every frame's
keypoints and descriptors are held to the CPU oracle bit for bit, and the FAST candidates of the first, a middle and the last frame
level by level.  A batch holds distinct textured frames, one flat frame (no corner at all) and one pure-noise frame (every pixel a
FAST candidate: more candidates on a level than k_quadtree keeps in LDS)."""
import math
import threading
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch  # (before the library loads, so that both resolve the same HIP runtime)

from eao_fusion_amd import synth

pytestmark = pytest.mark.gpu

DEFAULT = (1000, 1.2, 8, 20, 7)          # (nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST)
ONE_LEVEL = (1000, 1.2, 1, 20, 7)
VGA = (480, 640)                         # (height, width)
RICH, SPARSE = (400, 1000), (40, 1000)   # synth_frame textures: (n_rect, n_small)
ORACLE_THREADS = 16

Case = namedtuple("Case", "name cfg shape tex batch path where")
CASES = [
    # -- the one-launch pyramid (k_pyramid_fused) serves batches up to 32 when its tiles fit
    Case("b1", DEFAULT, VGA, RICH, 1, "fused pyramid; level-0 FAST and quad-tree on the side stream; k_quadtree<1024>",
         "orb.hip:1221, orb_quadtree.hip:445"),
    Case("b32", DEFAULT, VGA, RICH, 32, "last fused batch", "orb.hip:1221"),
    # -- the k_resize chain
    Case("b33", DEFAULT, VGA, RICH, 33, "first chain batch: level-0 FAST on the side stream (early0), mid = 0, every quad-tree behind evFast0",
         "orb.hip:1178, 1197, 1300"),
    Case("b35", DEFAULT, VGA, RICH, 35, "chain, last batch of k_quadtree<1024>", "orb_quadtree.hip:445"),
    Case("b36", DEFAULT, VGA, RICH, 36, "chain, first batch of k_quadtree<256>", "orb_quadtree.hip:445"),
    Case("b47", DEFAULT, VGA, RICH, 47, "chain, last batch with mid = 0", "orb.hip:1197"),
    Case("b48", DEFAULT, VGA, RICH, 48, "first batch with mid = 3 and qtEarly: FAST and quad-trees of levels 0-2 on the side stream",
         "orb.hip:1197, 1202"),
    Case("b96", DEFAULT, VGA, RICH, 96, "last batch with qtEarly", "orb.hip:1202"),
    Case("b97", DEFAULT, VGA, RICH, 97, "mid = 3 without qtEarly: every quad-tree on the main stream behind evFast0", "orb.hip:1202, 1300"),
    # -- no fused pyramid at a small batch: each of the three reasons
    Case("sf2.5-b4", (1000, 2.5, 3, 20, 7), VGA, RICH, 4, "chain at a small batch: scale factor above 2", "orb_host.hip:150"),
    Case("odd-sf2-b5", (1000, 2.0, 3, 20, 7), (481, 641), RICH, 5, "chain at a small batch: 641 -> 320 px is a step beyond 2 (invX > 2)",
         "orb_host.hip:151-152"),
    Case("16lev-b4", (1000, 1.1, 16, 20, 7), VGA, RICH, 4, "16 levels (kMaxLevels): chain at a small batch, the pyramid tiles need more than 64 KB of LDS",
         "orb_host.hip:150"),
    Case("16lev-b48", (1000, 1.1, 16, 20, 7), VGA, RICH, 48, "16 levels, mid = 3 and qtEarly", "orb.hip:1197, 1202"),
    # -- level counts: one level (no early0, no resize, no fused pyramid), two and three (early0 without mid), four (mid = 3 with one level above it)
    Case("1lev-b1", ONE_LEVEL, VGA, RICH, 1, "one level: every stage on the caller's stream", "orb.hip:1178, orb_host.hip:93"),
    Case("1lev-b48", ONE_LEVEL, VGA, RICH, 48, "one level at a large batch: no early0, so no mid", "orb.hip:1178, 1197"),
    Case("2lev-b48", (500, 1.2, 2, 20, 7), VGA, RICH, 48, "early0 without mid (nlevels <= 3)", "orb.hip:1197"),
    Case("3lev-b64", (300, 1.5, 3, 30, 10), (240, 320), RICH, 64, "early0 without mid (nlevels <= 3), frame -> XCD affinity", "orb.hip:1197"),
    Case("sf1.1-4lev-b48", (1200, 1.1, 4, 15, 5), (480, 752), RICH, 48, "mid = 3 and qtEarly with a single level on the main stream",
         "orb.hip:1197, 1202"),
    Case("kitti-b48", (2000, 1.2, 8, 20, 7), (376, 1241), RICH, 48, "KITTI-wide frames (several initial quad-tree nodes), mid = 3 and qtEarly",
         "orb_host.hip:67, orb.hip:1197"),
    # -- quad-tree node lists in the global workspace (test_thousands_of_features_on_few_levels' configurations)
    Case("qtglobal-2lev-b48", (3000, 1.5, 2, 20, 3), (353, 989), RICH, 48, "global quad-tree workspace, early0 without mid", "orb_host.hip:180"),
    Case("qtglobal-sf2-b48", (3000, 2.0, 2, 50, 3), (502, 714), SPARSE, 48, "global quad-tree workspace, sparse texture", "orb_host.hip:180"),
    Case("qtglobal-3lev-b48", (5000, 1.2, 3, 20, 7), VGA, RICH, 48, "global quad-tree workspace, three levels", "orb_host.hip:180"),
]

# profiled calls (eao_orb_set_profiling): early0 off, every stage alone on the caller's stream, events ev[0..9] around them
PROFILED = [("b1", DEFAULT, 1), ("b40", DEFAULT, 40), ("b64", DEFAULT, 64), ("b104", DEFAULT, 104), ("1lev-b48", ONE_LEVEL, 48)]

SEED0 = 60000


def _ids(batch, which):
    """Frame ids of batch X (which = 0) or Y (which = 1): distinct seeds, a flat and a pure-noise frame at places that differ
    between X and Y.  A single frame: X a textured frame, Y pure noise."""
    ids = [SEED0 + which * batch + i for i in range(batch)]
    if batch == 1:
        return ids if which == 0 else ["noise1"]
    if which == 0:
        ids[1], ids[-1] = "flat", "noise0"
    else:
        ids[0], ids[-1] = "noise1", "flat"
    return ids


class Inputs:
    """Frames by id and the oracle's results on them, each computed once per module (the oracle in a pool of threads, one
    OrbOracle per thread and configuration)."""

    def __init__(self, oracle):
        self.O = oracle
        self.frames, self.refs = {}, {}
        self.tl = threading.local()

    def frame(self, shape, tex, fid):
        key = (shape, tex, fid)
        img = self.frames.get(key)
        if img is None:
            h, w = shape
            if fid == "flat":
                img = np.full((h, w), 77, np.uint8)
            elif isinstance(fid, str):
                img = np.random.default_rng(7700 + int(fid[5:])).integers(0, 256, (h, w), dtype=np.uint8)
            else:
                img = synth.synth_frame(fid, w, h, *tex)
            self.frames[key] = img
        return img

    def batch(self, shape, tex, ids):
        return np.stack([self.frame(shape, tex, fid) for fid in ids])

    def _one(self, cfg, shape, tex, fid, stages):
        orcs = self.tl.__dict__.setdefault("orcs", {})
        orc = orcs.get(cfg)
        if orc is None:
            orc = orcs[cfg] = self.O.OrbOracle(*cfg)
        kps, desc = orc.extract(self.frame(shape, tex, fid))
        return kps, desc, [orc.level_candidates(l) for l in range(cfg[2])] if stages else None

    def oracle(self, cfg, shape, tex, ids, stage_ids=()):
        """(keypoints, descriptors, per-level FAST candidates or None) of every frame of `ids`; candidates for `stage_ids`."""
        need = [fid for fid in dict.fromkeys(list(ids) + list(stage_ids))
                if (cfg, shape, tex, fid) not in self.refs or (fid in stage_ids and self.refs[(cfg, shape, tex, fid)][2] is None)]
        if need:
            with ThreadPoolExecutor(ORACLE_THREADS) as ex:
                out = list(ex.map(lambda fid: self._one(cfg, shape, tex, fid, fid in stage_ids), need))
            for fid, r in zip(need, out):
                self.refs[(cfg, shape, tex, fid)] = r
        return [self.refs[(cfg, shape, tex, fid)] for fid in ids]


@pytest.fixture(scope="module")
def gpu():
    import eao_fusion_amd as E
    assert E.load().eao_device_check() == 0, E.load().eao_last_error()
    return E


@pytest.fixture(scope="module")
def inputs(oracle):
    return Inputs(oracle)


def _check(kps, desc, refs, what):
    bad = [f for f, (okps, odesc, _) in enumerate(refs)
           if not (len(kps[f]) == len(okps) and np.array_equal(kps[f], okps) and np.array_equal(desc[f], odesc))]
    assert not bad, "%s: frames %s of %d differ from the oracle" % (what, bad, len(refs))


def _same(a, b, what):
    (ka, da), (kb, db) = a, b
    assert len(ka) == len(kb), what
    bad = [f for f in range(len(ka)) if not (np.array_equal(ka[f], kb[f]) and np.array_equal(da[f], db[f]))]
    assert not bad, "%s: frames %s differ" % (what, bad)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_schedule_matches_oracle_frame_by_frame(gpu, inputs, case):
    B = case.batch
    X, Y = _ids(B, 0), _ids(B, 1)
    stage = sorted({0, B // 2, B - 1})
    rx = inputs.oracle(case.cfg, case.shape, case.tex, X, [X[f] for f in stage])
    ry = inputs.oracle(case.cfg, case.shape, case.tex, Y)
    if B > 1:      # the noise frame holds more candidates on a level than k_quadtree can keep in LDS (qtLdsCand: at most this bound)
        assert max(len(c) for c in rx[B - 1][2]) > min(8192, max(2048, (case.cfg[0] * 4 + 63) & ~63))
    imgs_x, imgs_y = inputs.batch(case.shape, case.tex, X), inputs.batch(case.shape, case.tex, Y)
    ext = gpu.ORBextractor(*case.cfg)
    for what, imgs, refs in (("X", imgs_x, rx), ("Y", imgs_y, ry), ("X again", imgs_x, rx)):
        kps, desc = ext.extract_batch(imgs)
        _check(kps, desc, refs, "%s (%s), batch %s" % (case.name, case.path, what))
    # FAST candidates of the last call, level by level: a FAST or quad-tree fault shows here before the description
    for f in stage:
        for l in range(case.cfg[2]):
            got, want = ext.level_candidates(l, f), rx[f][2][l]
            assert got.shape == want.shape and np.array_equal(got, want), "%s: frame %d, level %d FAST candidates" % (case.name, f, l)


@pytest.mark.parametrize("B", [48, 96, 97])
def test_device_api_odd_width_and_frame_stride(gpu, inputs, B):
    """The mid = 3 schedules through eao_orb_extract_batch_device on frames in the caller's layout: an odd width and pitch, a frame
    stride that is not a multiple of 4 and a base pointer that is not 4-byte aligned take the byte-wise variants of the resize, the
    FAST staging, the blur and the orientation loads (X, Y, X on one handle, as above)."""
    h, w = 480, 639
    pitch, shift = 641, 1
    fstride = h * pitch + 3
    cfg, tex = DEFAULT, RICH
    X, Y = _ids(B, 0), _ids(B, 1)
    rx, ry = inputs.oracle(cfg, (h, w), tex, X), inputs.oracle(cfg, (h, w), tex, Y)
    ext = gpu.ORBextractor(*cfg)
    cap = ext.max_keypoints(w, h)
    d_k = torch.zeros((B, cap, 28), dtype=torch.uint8, device="cuda")
    d_d = torch.zeros((B, cap, 32), dtype=torch.uint8, device="cuda")
    d_n = torch.zeros(B, dtype=torch.int32, device="cuda")
    for what, ids, refs in (("X", X, rx), ("Y", Y, ry), ("X again", X, rx)):
        host = np.zeros(shift + (B - 1) * fstride + h * pitch + 8, np.uint8)
        for f, fid in enumerate(ids):
            o = shift + f * fstride
            host[o:o + h * pitch].reshape(h, pitch)[:, :w] = inputs.frame((h, w), tex, fid)
        d_img = torch.from_numpy(host).cuda()
        torch.cuda.synchronize()
        ext.extract_batch_device(d_img.data_ptr() + shift, w, h, pitch, fstride, B, d_k.data_ptr(), d_d.data_ptr(), cap, d_n.data_ptr(),
                                 torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        n, k, d = d_n.cpu().numpy(), d_k.cpu().numpy(), d_d.cpu().numpy()
        kps = [k[f, :n[f]].reshape(-1).view(gpu.KP_DTYPE) for f in range(B)]
        _check(kps, [d[f, :n[f]] for f in range(B)], refs, "device API, batch %d, %s" % (B, what))


@pytest.mark.parametrize("name,cfg,B", PROFILED, ids=[p[0] for p in PROFILED])
def test_profiled_calls_match_unprofiled(gpu, inputs, name, cfg, B):
    """Profiled calls (what bench.py --full's per-stage run makes) compute what unprofiled ones do: bit-identical to the
    unprofiled call on the same handle and to the oracle, with six finite, non-negative stage times; switching profiling off
    gives the unprofiled schedule back."""
    X, Y = _ids(B, 0), _ids(B, 1)
    rx, ry = inputs.oracle(cfg, VGA, RICH, X), inputs.oracle(cfg, VGA, RICH, Y)
    imgs_x, imgs_y = inputs.batch(VGA, RICH, X), inputs.batch(VGA, RICH, Y)
    ext = gpu.ORBextractor(*cfg)
    plain_x = ext.extract_batch(imgs_x)
    _check(*plain_x, rx, "%s unprofiled X" % name)
    ext.set_profiling(True)
    prof_y = ext.extract_batch(imgs_y)
    _check(*prof_y, ry, "%s profiled Y" % name)
    prof_x = ext.extract_batch(imgs_x)
    _check(*prof_x, rx, "%s profiled X" % name)
    _same(prof_x, plain_x, "%s profiled X vs unprofiled X" % name)
    t = ext.last_timing()
    assert len(t) == 6 and all(math.isfinite(v) and v >= 0 for v in t.values()) and t["total"] > 0, t
    ext.set_profiling(False)
    plain_y = ext.extract_batch(imgs_y)
    _check(*plain_y, ry, "%s unprofiled Y after profiling" % name)
    _same(plain_y, prof_y, "%s unprofiled Y vs profiled Y" % name)
