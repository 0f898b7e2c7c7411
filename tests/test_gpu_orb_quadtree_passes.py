"""GPU parity of k_quadtree's passes on small frames: one candidate sweep and two barriers per pass.

A pass of k_quadtree (eao_fusion_amd/csrc/orb_quadtree.hip) is wave 0's list logic and then ONE sweep of the whole workgroup over the
candidates (rehome_and_count): it moves every candidate to its new node and counts it in the NEXT pass's child histogram, which lives in
the second of two buffers; the sweep that assigns the initial nodes counts the first histogram the same way, once the empty initial
nodes are dropped.  What can go wrong is a histogram that is stale, not zeroed or counted under the wrong split point, and it shows
as a different node list, so every frame's keypoints and descriptors are held to the CPU oracle bit for bit, and the FAST candidates
of the first and the last frame level by level.

As in test_gpu_orb_schedules.py each case runs two batches X and Y of different frames and then X again on ONE handle.  Batches 1 and 35
take the 1024-thread form of the kernel, 36 the 256-thread one.  A batch holds textured synth_frames and
  - "flat": no corner at all (M = 0 on every level);
  - "dot": one bright pixel on a flat ground, so that a level holds exactly one candidate (asserted);
  - "gap": a textured frame whose middle third is flat -- on the wide frames several of the initial nodes are then empty (asserted)
    while the others hold hundreds of candidates;
  - "noise": every pixel random; at 320 x 240 with nfeatures 200 level 0 holds more candidates than k_quadtree keeps in LDS
    (qtLdsCand; asserted), so the keys and node indices of that workgroup live in the global arrays.

Shapes.  Frames of 160 x 120, 320 x 240 and the wide 640 x 96 (ten initial nodes); nfeatures 30, 200 and 1000.  The two pyramids, 8 levels
at 1.2 and 3 levels at 1.5, run at 320 x 240.  Neither fits the two smaller frames: their top level would be smaller than one 30 px FAST
cell plus borders, which the extractor and the oracle both refuse ("unsupported image geometry").  Those frames take the deepest pyramids
they admit: 160 x 120 four levels at 1.2 and two at 1.5, 640 x 96 three levels at 1.2.

Both ways a tree ends are reached (test_both_endings_are_reached, on the oracle's output alone).  Among the (frame, level) pairs of the
textured synth_frames of all cases, first call of X and Y each, the seeds below give
  - 758 pairs that return exactly their quota N (ended in a full or a careful pass with S >= N; 1070 more end the same way above N), and
  - 248 pairs that return fewer keypoints than N although they had candidates (ended on S2 == S: no entry left to split)."""
import threading
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch  # noqa: F401  (before the library loads, so that both resolve the same HIP runtime)

from eao_fusion_amd import synth

pytestmark = pytest.mark.gpu

QVGA, QQVGA, WIDE = (240, 320), (120, 160), (96, 640)      # (height, width)
ORACLE_THREADS = 16
SEED0 = 81000

Case = namedtuple("Case", "name cfg shape batch")
CASES = [
    Case("qvga-8lev-n1000-b36", (1000, 1.2, 8, 20, 7), QVGA, 36),     # upper levels hold fewer candidates than their quota asks for
    Case("qvga-8lev-n200-b35", (200, 1.2, 8, 20, 7), QVGA, 35),       # the noise frame's level 0 exceeds qtLdsCand
    Case("qvga-3lev-n30-b1", (30, 1.5, 3, 20, 7), QVGA, 1),
    Case("qvga-3lev-n1000-b35", (1000, 1.5, 3, 20, 7), QVGA, 35),
    Case("qqvga-4lev-n200-b36", (200, 1.2, 4, 20, 7), QQVGA, 36),
    Case("qqvga-2lev-n30-b1", (30, 1.5, 2, 20, 7), QQVGA, 1),
    Case("qqvga-4lev-n1000-b35", (1000, 1.2, 4, 20, 7), QQVGA, 35),   # every level holds fewer candidates than its quota asks for
    Case("wide-3lev-n1000-b35", (1000, 1.2, 3, 20, 7), WIDE, 35),
    Case("wide-3lev-n200-b36", (200, 1.2, 3, 20, 7), WIDE, 36),
    Case("wide-3lev-n30-b1", (30, 1.2, 3, 20, 7), WIDE, 1),
]


def _ids(batch, which):
    """Frame ids of batch X (which = 0) or Y (which = 1).  A single frame: X the gap frame, Y the dot."""
    if batch == 1:
        return ["gap0"] if which == 0 else ["dot"]
    ids = [SEED0 + which * batch + i for i in range(batch)]
    if which == 0:
        ids[1], ids[2], ids[3], ids[-1] = "flat", "dot", "gap0", "noise0"
    else:
        ids[0], ids[2], ids[-2], ids[-1] = "noise1", "gap1", "dot", "flat"
    return ids


def _frame(shape, fid):
    h, w = shape
    if fid == "flat":
        return np.full((h, w), 77, np.uint8)
    if fid == "dot":
        img = np.full((h, w), 77, np.uint8)
        img[h // 2, w // 3] = 255
        return img
    if isinstance(fid, str) and fid.startswith("noise"):
        return np.random.default_rng(7700 + int(fid[5:])).integers(0, 256, (h, w), dtype=np.uint8)
    if isinstance(fid, str):       # "gap<i>"
        img = synth.synth_frame(SEED0 - 1 - int(fid[3:]), w, h)
        img[:, w // 3:2 * w // 3] = 77
        return img
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
        return self.O.OrbOracle(*cfg).tables()["quota"]


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


def _ini_nodes(cand_level0, shape):
    """Occupied initial quad-tree nodes of level 0 (src/ORBextractor.cc:543-553: nIni = round(width / height) columns of width hX)."""
    h, w = shape
    width, height = (w - 19 + 3) - 16, (h - 19 + 3) - 16      # (maxBorderX - minBorderX, maxBorderY - minBorderY; EDGE_THRESHOLD 19)
    n_ini = int(round(width / height))
    hx = np.float32(width) / np.float32(n_ini)
    occupied = np.unique(np.minimum((cand_level0[:, 0] / hx).astype(np.int32), n_ini - 1))
    return n_ini, occupied


def endings(inputs):
    """(exact, over, fewer): (frame, level) pairs of the textured synth_frames of all cases whose level returned exactly its quota, more
    (the last pass overshot), or fewer although it had candidates."""
    exact = over = fewer = 0
    for case in CASES:
        quota = inputs.quota(case.cfg)
        for which in (0, 1):
            ids = _ids(case.batch, which)
            for fid, (okps, _, cands) in zip(ids, inputs.oracle(case.cfg, case.shape, ids)):
                if isinstance(fid, str):
                    continue
                per = np.bincount(okps["octave"], minlength=case.cfg[2])
                for l in range(case.cfg[2]):
                    if len(cands[l]) == 0:
                        continue
                    exact += per[l] == quota[l]
                    over += per[l] > quota[l]
                    fewer += per[l] < quota[l]
    return int(exact), int(over), int(fewer)


def test_both_endings_are_reached(inputs):
    exact, over, fewer = endings(inputs)
    print("endings: %d exact, %d over, %d fewer" % (exact, over, fewer))
    assert exact >= 100 and fewer >= 100, (exact, over, fewer)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_passes_match_oracle(gpu, inputs, case):
    B = case.batch
    X, Y = _ids(B, 0), _ids(B, 1)
    rx, ry = inputs.oracle(case.cfg, case.shape, X), inputs.oracle(case.cfg, case.shape, Y)
    # what the special frames are there for, on the oracle's output alone
    dot = inputs.oracle(case.cfg, case.shape, ["dot"])[0]
    assert 1 in [len(c) for c in dot[2]], "dot frame: no level with exactly one candidate"
    if B > 1:
        assert all(len(c) == 0 for c in rx[1][2]) and len(rx[1][0]) == 0, "flat frame has candidates"
    if case.shape == WIDE:
        n_ini, occ = _ini_nodes(rx[0 if B == 1 else 3][2][0], case.shape)
        assert n_ini >= 8 and 2 <= len(occ) < n_ini, "gap frame: initial nodes %s of %d occupied" % (occ, n_ini)
    if case.name == "qvga-8lev-n200-b35":
        assert len(rx[B - 1][2][0]) > min(8192, max(2048, (case.cfg[0] * 4 + 63) & ~63)), "noise frame fits qtLdsCand"
    imgs_x, imgs_y = inputs.batch(case.shape, X), inputs.batch(case.shape, Y)
    ext = gpu.ORBextractor(*case.cfg)
    for what, imgs, refs in (("X", imgs_x, rx), ("Y", imgs_y, ry), ("X again", imgs_x, rx)):
        kps, desc = ext.extract_batch(imgs)
        _check(kps, desc, refs, "%s, batch %s" % (case.name, what))
    for f in sorted({0, B - 1}):
        for l in range(case.cfg[2]):
            got, want = ext.level_candidates(l, f), rx[f][2][l]
            assert got.shape == want.shape and np.array_equal(got, want), "%s: frame %d, level %d FAST candidates" % (case.name, f, l)
