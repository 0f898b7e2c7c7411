"""GPU parity of k_quadtree's register-form passes, its hand-over to the general form and the set-up of a level with one initial node.

While a node list holds at most 64 entries, wave 0 of k_quadtree (eao_fusion_amd/csrc/orb_quadtree.hip) keeps one entry per lane and takes
ranks and prefixes from ballots, a DPP scan and, in a careful pass, a loop of readlanes; a pass entered with more than 64 entries takes the
general form over the index arrays in LDS, and a tree goes from the first form to the second, never back.  A level with ONE initial node
builds that node from the geometry and counts the first child histogram while the gather stores the keys; a level with several keeps the
initial assignment and its sweep.  A wrong rank, prefix or histogram shows as a different node list, so every frame's keypoints and
descriptors are held to the CPU oracle bit for bit, and the FAST candidates of the first and the last frame level by level (the gather now
also counts).

As in test_gpu_orb_quadtree_passes.py each case runs two batches X and Y of different frames and then X again on ONE handle.  Batches 1 and
35 take the 1024-thread form of the kernel, 36 the 256-thread one.  A batch holds textured synth_frames and a flat frame (no corner at all),
a "dot" frame (one bright pixel: a level with exactly one candidate, the M = 1 leaf) and a noise frame (every pixel random).

Shapes.  320 x 240 with 8 levels at 1.2 (one initial node on every level), and 320 x 176, whose border-cropped extent is 288 x 144 = 2:1,
hence TWO initial nodes on level 0: the path of several initial nodes then runs beside the new set-up in one suite.  320 x 176 takes 6 levels
at 1.2, the deepest pyramid the extractor and the oracle admit (7 levels: "unsupported image geometry", asserted for the oracle).

What the nfeatures values are there for (quotas asserted against the oracle's tables()["quota"]; test_every_handover_is_reached counts the
(frame, level) pairs of the textured synth_frames of all cases, first call of X and Y each, on the oracle's output alone):
  (a) nfeatures 200 and 300 at 320 x 240: quotas 43 .. 13 and 65 .. 19.  Levels with a quota in 17..64 that return exactly their quota: the
      careful pass in register form stopped in the middle of its list.
  (b) nfeatures 2000 at 320 x 240: quotas 434, 362, 302 on levels 0-2.  Levels that return more than 256 keypoints: trees of five or more
      passes (a pass at most quadruples the list), entered with more than 64 entries at the latest in the fifth -- the register form has
      handed over to the general one.
  (c) levels that return fewer keypoints than their quota although they had candidates: ended on S2 == S, nothing left to split.
  (d) the noise frames at nfeatures 300, 1000 and 2000 (quota of level 0: 65, 217 and 434, all > 64): level 0 returns at least its quota, so
      the tree met a list of 64 multi-key entries on its way (4 -> 16 -> 64, every node of a noise frame holds hundreds of keys).
The seeds below give (a) 376, (b) 201, (c) 68 pairs and (d) 6 frames; the floors are 20, 20, 20 and 1."""
import threading
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch  # noqa: F401  (before the library loads, so that both resolve the same HIP runtime)

from eao_fusion_amd import synth

pytestmark = pytest.mark.gpu

QVGA, TWO_TO_ONE = (240, 320), (176, 320)      # (height, width)
ORACLE_THREADS = 16
SEED0 = 83000

Case = namedtuple("Case", "name cfg shape batch")
CASES = [
    Case("qvga-8lev-n200-b36", (200, 1.2, 8, 20, 7), QVGA, 36),
    Case("qvga-8lev-n300-b35", (300, 1.2, 8, 20, 7), QVGA, 35),
    Case("qvga-8lev-n2000-b36", (2000, 1.2, 8, 20, 7), QVGA, 36),
    Case("qvga-8lev-n1000-b35", (1000, 1.2, 8, 20, 7), QVGA, 35),
    Case("qvga-8lev-n2000-b1", (2000, 1.2, 8, 20, 7), QVGA, 1),
    Case("2to1-6lev-n200-b36", (200, 1.2, 6, 20, 7), TWO_TO_ONE, 36),
    Case("2to1-6lev-n1000-b35", (1000, 1.2, 6, 20, 7), TWO_TO_ONE, 35),
    Case("2to1-6lev-n300-b1", (300, 1.2, 6, 20, 7), TWO_TO_ONE, 1),
]
QUOTAS = {   # the oracle's tables()["quota"], asserted in test_every_handover_is_reached
    (200, 1.2, 8, 20, 7): [43, 36, 30, 25, 21, 17, 15, 13],
    (300, 1.2, 8, 20, 7): [65, 54, 45, 38, 31, 26, 22, 19],
    (1000, 1.2, 8, 20, 7): [217, 181, 151, 126, 105, 87, 73, 60],
    (2000, 1.2, 8, 20, 7): [434, 362, 302, 251, 209, 175, 145, 122],
}


def _ids(batch, which):
    """Frame ids of batch X (which = 0) or Y (which = 1).  A single frame: X a textured frame, Y the dot."""
    if batch == 1:
        return [SEED0] if which == 0 else ["dot"]
    ids = [SEED0 + which * batch + i for i in range(batch)]
    if which == 0:
        ids[1], ids[2], ids[-1] = "flat", "dot", "noise0"
    else:
        ids[0], ids[-2], ids[-1] = "noise1", "dot", "flat"
    return ids


def _frame(shape, fid):
    h, w = shape
    if fid == "flat":
        return np.full((h, w), 77, np.uint8)
    if fid == "dot":
        img = np.full((h, w), 77, np.uint8)
        img[h // 2, w // 3] = 255
        return img
    if isinstance(fid, str):       # "noise<i>"
        return np.random.default_rng(7900 + int(fid[5:])).integers(0, 256, (h, w), dtype=np.uint8)
    return synth.synth_frame(fid, w, h)


class Inputs:
    """Frames by id and the oracle's results on them, each computed once per module and left unchanged."""

    def __init__(self, oracle):
        self.O = oracle
        self.frames, self.refs = {}, {}
        self.tl = threading.local()

    def frame(self, shape, fid):
        img = self.frames.get((shape, fid))
        if img is None:
            img = self.frames[(shape, fid)] = _frame(shape, fid)
        return img

    def batch(self, shape, ids):
        return np.stack([self.frame(shape, fid) for fid in ids])

    def _one(self, cfg, shape, fid):
        orcs = self.tl.__dict__.setdefault("orcs", {})
        orc = orcs.get(cfg)
        if orc is None:
            orc = orcs[cfg] = self.O.OrbOracle(*cfg)
        kps, desc = orc.extract(self.frame(shape, fid))
        return kps, desc, [orc.level_candidates(l) for l in range(cfg[2])]

    def oracle(self, cfg, shape, ids):
        """(keypoints, descriptors, per-level FAST candidates) of every frame of `ids`."""
        need = [fid for fid in dict.fromkeys(ids) if (cfg, shape, fid) not in self.refs]
        if need:
            with ThreadPoolExecutor(ORACLE_THREADS) as ex:
                out = list(ex.map(lambda fid: self._one(cfg, shape, fid), need))
            for fid, r in zip(need, out):
                self.refs[(cfg, shape, fid)] = r
        return [self.refs[(cfg, shape, fid)] for fid in ids]

    def quota(self, cfg):
        return [int(q) for q in self.O.OrbOracle(*cfg).tables()["quota"]]


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


def _n_ini(shape):
    """Initial quad-tree nodes of level 0 (src/ORBextractor.cc:543: nIni = round(width / height) of the border-cropped extent; EDGE_THRESHOLD 19)."""
    h, w = shape
    return int(round(((w - 19 + 3) - 16) / ((h - 19 + 3) - 16)))


def handovers(inputs):
    """(a, b, c, d) of the module docstring: (frame, level) pairs of the textured synth_frames of the 320 x 240 cases for a-c, noise frames for d."""
    a = b = c = d = 0
    for case in CASES:
        if case.shape != QVGA:
            continue
        quota = inputs.quota(case.cfg)
        for which in (0, 1):
            ids = _ids(case.batch, which)
            for fid, (okps, _, cands) in zip(ids, inputs.oracle(case.cfg, case.shape, ids)):
                per = np.bincount(okps["octave"], minlength=case.cfg[2])
                if isinstance(fid, str):
                    d += fid.startswith("noise") and quota[0] > 64 and per[0] >= quota[0]
                    continue
                for l in range(case.cfg[2]):
                    if len(cands[l]) == 0:
                        continue
                    a += 17 <= quota[l] <= 64 and per[l] == quota[l]
                    b += per[l] > 256
                    c += per[l] < quota[l]
    return int(a), int(b), int(c), int(d)


def test_every_handover_is_reached(inputs):
    for cfg, want in QUOTAS.items():
        assert inputs.quota(cfg) == want, (cfg, inputs.quota(cfg))
    assert _n_ini(QVGA) == 1 and _n_ini(TWO_TO_ONE) == 2
    with pytest.raises(Exception, match="unsupported image geometry"):       # 320 x 176 admits no seventh level
        inputs.O.OrbOracle(200, 1.2, 7, 20, 7).extract(inputs.frame(TWO_TO_ONE, SEED0))
    a, b, c, d = handovers(inputs)
    print("hand-overs: (a) %d exact with quota 17..64, (b) %d above 256 keypoints, (c) %d fewer than quota, (d) %d full noise frames" % (a, b, c, d))
    assert a >= 20 and b >= 20 and c >= 20 and d >= 1, (a, b, c, d)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_register_passes_match_oracle(gpu, inputs, case):
    B = case.batch
    X, Y = _ids(B, 0), _ids(B, 1)
    rx, ry = inputs.oracle(case.cfg, case.shape, X), inputs.oracle(case.cfg, case.shape, Y)
    # what the special frames are there for, on the oracle's output alone
    dot = inputs.oracle(case.cfg, case.shape, ["dot"])[0]
    assert 1 in [len(c) for c in dot[2]], "dot frame: no level with exactly one candidate"
    if B > 1:
        assert all(len(c) == 0 for c in rx[1][2]) and len(rx[1][0]) == 0, "flat frame has candidates"
    if case.shape == TWO_TO_ONE:   # both initial nodes of level 0 hold candidates of the first frame
        hx = np.float32(288) / np.float32(2)
        assert set(np.minimum((rx[0][2][0][:, 0] / hx).astype(np.int32), 1)) == {0, 1}
    imgs_x, imgs_y = inputs.batch(case.shape, X), inputs.batch(case.shape, Y)
    ext = gpu.ORBextractor(*case.cfg)
    for what, imgs, refs in (("X", imgs_x, rx), ("Y", imgs_y, ry), ("X again", imgs_x, rx)):
        kps, desc = ext.extract_batch(imgs)
        _check(kps, desc, refs, "%s, batch %s" % (case.name, what))
    for f in sorted({0, B - 1}):
        for l in range(case.cfg[2]):
            got, want = ext.level_candidates(l, f), rx[f][2][l]
            assert got.shape == want.shape and np.array_equal(got, want), "%s: frame %d, level %d FAST candidates" % (case.name, f, l)
