"""tools/export_detnet.py: a torch YOLOX with random batch-norm statistics, exported and walked by the numpy yardstick, against torch's own float64 forward.  Let
E32 be the largest difference between torch's float32 and float64 forwards over the head; the yardstick stays below 8 x E32 (a sequential chain accumulates more
error than torch's blocked sums; a wiring or folding error is of order one)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import detnet_models as M  # noqa: E402
import detnet_reference as R  # noqa: E402
import detnet_torch as T  # noqa: E402
import export_detnet as X  # noqa: E402


def test_exported_model_against_torch_float64():
    import copy
    import torch
    net = T.randomised(0.33, 0.25, 7, seed=31)
    assert X.infer(net.state_dict()) == (1 / 3.0, 0.25, 7)
    model = X.export(net)
    blob = M.blob(64, 32)
    with torch.no_grad():
        x = torch.from_numpy(blob)[None]
        h32 = net(x)[0].numpy().astype(np.float64)
        h64 = copy.deepcopy(net).double()(x.double())[0].numpy()
    head = R.forward(model, 64, blob)[1]
    assert head.shape == h64.shape == (84, 12)
    e32, ours = np.abs(h32 - h64).max(), np.abs(head.astype(np.float64) - h64).max()
    print("E32 = %.3e, yardstick = %.3e" % (e32, ours))
    assert 0 < e32 < 1e-4, "the float32 forward itself is off: the scene proves nothing"
    assert ours < 8 * e32
    # the same through the file and the host walk: the bytes the yardstick gives
    assert M.same_bits(M.walk_run(M.walk_binary(("-O2",)), model, 64, blob)[1], head)


def test_state_dict_with_explicit_sizes_and_a_depthwise_refusal():
    import pytest
    net = T.randomised(0.33, 0.125, 3, seed=33)
    sd = net.state_dict()
    assert X.export(sd, 0.33, 0.125, 3).tobytes() == X.export(net).tobytes()
    sd = dict(sd)
    w = sd["backbone.backbone.dark2.0.conv.weight"]
    sd["backbone.backbone.dark2.0.conv.weight"] = w[:, :1]      # a depthwise layer has one input channel per group
    with pytest.raises(ValueError, match="depthwise"):
        X.export(sd)
