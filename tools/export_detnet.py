"""Turns a YOLOX in torch into the model file eao_detnet_create reads (eao_fusion_amd/csrc/detnet_internal.h): the stand-in for the reference's serialised TensorRT
engine (src/YOLOX.cc:7-48).

    python tools/export_detnet.py <checkpoint.pth> <out.detnet> [--depth D --width W --classes C]

export(module) or export(state_dict, depth, width, classes) -> eao_fusion_amd.detnet.Model.  The keys are upstream YOLOX's (backbone.backbone.stem.conv.conv.weight,
head.cls_preds.0.bias, ...); depth, width and the class count are read off the tensor shapes when not given.  Batch norm is folded in float64 -- w' = w * gamma /
sqrt(var + eps), b' = beta - mean * gamma / sqrt(var + eps), eps = 1e-3 as upstream sets it -- and every number is rounded to float32 once.  Depthwise models
(YOLOX-nano, YOLOX-tiny with depthwise=True) are not supported.  No official checkpoint was at hand when this was written: the key names follow upstream's source
and tests/detnet_torch.py, and are unverified against a released file."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from eao_fusion_amd import detnet as D  # noqa: E402

BN_EPS = 1e-3


def infer(sd):
    """(depth, width, classes) from the shapes of a state_dict"""
    bc = sd["backbone.backbone.stem.conv.conv.weight"].shape[0]
    n = len({k.split(".")[5] for k in sd if k.startswith("backbone.backbone.dark2.1.m.")})
    return n / 3.0, bc / 64.0, sd["head.cls_preds.0.weight"].shape[0]


def export(model, depth=None, width=None, classes=None, bn_eps=BN_EPS):
    sd = model.state_dict() if hasattr(model, "state_dict") else model
    sd = {k: v.detach().cpu().double().numpy() for k, v in sd.items() if hasattr(v, "detach") and v.ndim > 0}
    d, w, c = infer(sd)
    depth, width, classes = d if depth is None else depth, w if width is None else width, c if classes is None else classes

    def params(name, cout, k, cin):
        if name + ".conv.weight" in sd:      # BaseConv: a convolution without bias and its batch norm
            wt = sd[name + ".conv.weight"]
            scale = sd[name + ".bn.weight"] / np.sqrt(sd[name + ".bn.running_var"] + bn_eps)
            bias = sd[name + ".bn.bias"] - sd[name + ".bn.running_mean"] * scale
            wt = wt * scale[:, None, None, None]
        else:
            wt, bias = sd[name + ".weight"], sd[name + ".bias"]
        if wt.shape != (cout, cin, k, k):
            raise ValueError("%s has shape %s, the graph needs %s (a depthwise or grouped model is not supported)" % (name, wt.shape, (cout, cin, k, k)))
        return wt.transpose(0, 2, 3, 1).astype(np.float32), bias.astype(np.float32)

    return D.yolox_graph(depth, width, classes, params)[0]


def main(argv):
    import argparse
    import torch
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("checkpoint")
    ap.add_argument("out")
    ap.add_argument("--depth", type=float)
    ap.add_argument("--width", type=float)
    ap.add_argument("--classes", type=int)
    a = ap.parse_args(argv)
    ck = torch.load(a.checkpoint, map_location="cpu")
    sd = ck.get("model", ck) if isinstance(ck, dict) else ck
    m = export(sd, a.depth, a.width, a.classes)
    data = m.tobytes()
    with open(a.out, "wb") as f:
        f.write(data)
    print("%s: %d tensors, %d ops, %d weights, %d bytes" % (a.out, len(m.tensors), len(m.ops), m.n_weights, len(data)))


if __name__ == "__main__":
    main(sys.argv[1:])
