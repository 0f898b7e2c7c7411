"""Which tile form of k_detnet_conv a convolution takes (conv_form of eao_fusion_amd/csrc/detnet_internal.h, the rule launch_op switches on), read through
`detnet_walk forms`: the rule at its edges on single-convolution models, and the forms of YOLOX-s at S = 640 against a table written here."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detnet_models as M  # noqa: E402
from eao_fusion_amd import detnet as D  # noqa: E402

F = np.float32
ONE, TWO, LARGE = "16x16x4x1", "16x16x4x2", "32x32x2"


@pytest.fixture(scope="module")
def walk():
    return M.walk_binary(("-O2",))


def conv_model(H, W, cout):
    """a 1 x 1 convolution of one channel over an H x W map: M = H * W per frame"""
    return M.single_conv(np.zeros((H, W, 1), F), np.zeros((cout, 1, 1, 1), F), np.zeros(cout, F))["model"]


# (H, W, batch, Cout) -> the form.  M = H * W * batch; the large form from 256 blocks of 128 x 64 on, and never for Cout <= 16
EDGES = [
    ((1, 1, 1, 16), ONE), ((1, 1, 1, 17), TWO),
    ((2048, 2048, 1, 16), ONE),                                       # 32768 x 1 blocks: Cout <= 16 comes first
    ((255, 128, 1, 17), TWO), ((4096, 8, 1, 17), LARGE),              # one column block: M = 32640 (255 blocks), 32768 (256 blocks)
    # ... and an M tail.  (A side is at most 4096 and 32641 = 7 x 4663, 16257 = 3 x 5419 have no such factors: the first M past the edge that has is taken.)
    ((4080, 8, 1, 33), TWO), ((859, 38, 1, 33), LARGE),               # M = 32640 (255 blocks), 32642 (255 blocks and two rows: 256)
    ((4080, 8, 1, 64), TWO), ((859, 38, 1, 64), LARGE),               # Cout = 64 is still one column block
    ((127, 128, 1, 65), TWO), ((739, 22, 1, 65), LARGE),              # two column blocks: M = 16256 (127 x 2 = 254), 16258 (128 x 2 = 256)
    ((4064, 1, 4, 65), TWO), ((739, 11, 2, 65), LARGE),               # the batch counts: 4 x 4064 = 16256, 2 x 8129 = 16258
    ((1, 1, 1, 65536), LARGE), ((1, 1, 1, 16321), LARGE), ((1, 1, 1, 16320), TWO),      # one row block: 1024, 256 and 255 column blocks
]


@pytest.mark.parametrize("case,form", EDGES)
def test_conv_form_at_its_edges(walk, case, form):
    H, W, batch, cout = case
    ops = M.walk_forms(walk, conv_model(H, W, cout), 32, batch)
    assert len(ops) == 1 and ops[0]["kind"] == "conv" and ops[0]["M"] == H * W * batch and ops[0]["Cout"] == cout
    assert ops[0]["form"] == form


def test_forms_lists_every_op_with_its_parameters():
    walk = M.walk_binary(("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))      # (the build tests/test_detnet_host_cpu.py runs the walk under)
    sc = M.single_conv(np.zeros((6, 5, 4), F), np.zeros((5, 3, 3, 4), F), np.zeros(5, F), 2, D.SILU, res=np.zeros((3, 3, 5), F), src_total=9, src_c0=3, dst_total=8,
                       dst_c0=2, res_total=7, res_c0=1)
    assert M.walk_forms(walk, sc["model"], 32, 3) == [dict(kind="conv", M=27, Cout=5, k=3, stride=2, res=sc["res"], src_c0=3, dst_c0=2, head=0, form=ONE)]
    mp = M.single_map_op(D.MAXPOOL, np.zeros((5, 7, 4), F), 5, src_total=7, src_c0=1, dst_total=8, dst_c0=2)
    assert M.walk_forms(walk, mp["model"], 32, 2) == [dict(kind="maxpool", M=70, Cout=4, k=5, stride=1, res=-1, src_c0=1, dst_c0=2, head=0, form=None)]
    m, _ = M.yolox(0.33, 0.125, 3, seed=15)
    ops = M.walk_forms(walk, m, 64, 1)
    assert [o["kind"] for o in ops] == [("focus", "conv", "maxpool", "upsample2")[o["kind"]] for o in m.ops]
    assert [o["M"] for o in ops if o["head"]] == [64, 64, 64, 16, 16, 16, 4, 4, 4] and all((o["form"] is None) == (o["kind"] != "conv") for o in ops)


# ---------------------------------------------------------------- YOLOX-s (depth 0.33, width 0.5, 80 classes) at S = 640
# The 83 convolutions by upstream's module path.  LARGE_1 / LARGE_8: the ones on the 32 x 32 x 2 form at batch 1 / batch 8; SMALL_ONE: Cout <= 16 at any batch;
# every other one is on the two-tile 16 x 16 x 4 form.  M per frame is (640 / downscale)^2: 102400 for the stem, 25600 for dark2, 6400, 1600 and 400 below.
B = "backbone.backbone."
LARGE_1 = {B + "stem.conv"}                                  # 800 x 1 blocks; dark2's are 200 x 1: below 256
LARGE_8 = LARGE_1 | {B + "dark2.0", B + "dark2.1.conv1", B + "dark2.1.m.0.conv1", B + "dark2.1.m.0.conv2", B + "dark2.1.conv2", B + "dark2.1.conv3",      # 1600 x 1
                     B + "dark3.0", B + "dark3.1.conv3", "backbone.C3_p3.conv3",                                                              # M = 51200, Cout 128: 400 x 2
                     B + "dark3.1.conv1", B + "dark3.1.conv2", "backbone.C3_p3.conv1", "backbone.C3_p3.conv2",                                # Cout 64: 400 x 1
                     B + "dark3.1.m.0.conv1", B + "dark3.1.m.0.conv2", B + "dark3.1.m.1.conv1", B + "dark3.1.m.1.conv2", B + "dark3.1.m.2.conv1", B + "dark3.1.m.2.conv2",
                     "backbone.C3_p3.m.0.conv1", "backbone.C3_p3.m.0.conv2",
                     B + "dark4.0", B + "dark4.1.conv3", "backbone.C3_p4.conv3", "backbone.C3_n3.conv3",                                      # M = 12800, Cout 256: 100 x 4
                     "head.stems.0", "head.cls_convs.0.0", "head.cls_convs.0.1", "head.reg_convs.0.0", "head.reg_convs.0.1", "head.cls_preds.0"}      # 400 x 2
SMALL_ONE = {"head.%s_preds.%d" % (p, l) for p in ("reg", "obj") for l in range(3)}


@pytest.mark.parametrize("batch,large", ((1, LARGE_1), (8, LARGE_8)))
def test_forms_of_yolox_s_at_640(walk, batch, large):
    m, names = M.yolox(0.33, 0.5, 80)
    convs = [i for i, o in enumerate(m.ops) if o["kind"] == D.CONV]
    paths = list(names)      # (a dict keeps the order in which the graph wrote its convolutions)
    assert len(convs) == len(paths) == 83 and len(m.ops) == 89 and large <= set(paths) and SMALL_ONE <= set(paths)
    ops = M.walk_forms(walk, m, 640, batch)
    assert len(ops) == 89
    for i, path in zip(convs, paths):
        want = ONE if path in SMALL_ONE else LARGE if path in large else TWO
        side = 640 // names[path][3] if names[path][3] else ops[i]["M"]
        assert ops[i]["form"] == want, (path, ops[i])
        assert ops[i]["Cout"] == names[path][2] and (ops[i]["head"] or ops[i]["M"] == batch * side * side), (path, ops[i])
    assert len(large) == {1: 1, 8: 32}[batch]
