"""The yolox entry points at the drop-in boundary, without a device: the header declares them, the shared object exports them, the ctypes table binds them, the
structs have the layout the Python mirror and the host header assume, the defaults are the reference's literals (tests/golden/yolox_constants.json), and a
handle cannot be made without a device."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import reference_literals as RL  # noqa: E402

NAMES = ["eao_yolox_cfg_default", "eao_yolox_create", "eao_yolox_destroy", "eao_yolox_preprocess", "eao_yolox_preprocess_device", "eao_yolox_decode",
         "eao_yolox_decode_device", "eao_yolox_buffers", "eao_yolox_head", "eao_yolox_blob", "eao_yolox_proposals", "eao_yolox_set_profiling", "eao_yolox_last_kernel_ms"]


@pytest.fixture(scope="module")
def built():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "eao_fusion_amd", "csrc")])
    from eao_fusion_amd import _lib
    return _lib


def test_symbols_declared_exported_and_bound(built):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "eao_fusion.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(eao_yolox_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(NAMES)
    L = built.load()
    for name in NAMES:
        assert hasattr(L, name) and built.SYMBOLS[name] is not None, name


def test_defaults_are_the_reference_literals(built):
    lit = RL.literals("yolox")
    c = built.YoloxCfg()
    built.load().eao_yolox_cfg_default(C.byref(c))
    assert (c.input_size, c.num_classes) == (int(lit["INPUT_W"]), int(lit["NUM_CLASS"])) and int(lit["INPUT_H"]) == c.input_size
    assert c.conf_thresh == np.float32(float(lit["BBOX_CONF_THRESH"])) and c.nms_thresh == np.float32(float(lit["NMS_THRESH"]))
    assert (c.max_proposals, c.max_batch) == (4096, 1)
    hdr = open(os.path.join(ROOT, "include", "eao_fusion.h")).read()
    assert "#define EAO_YOLOX_INPUT_SIZE %s " % lit["INPUT_W"] in hdr and "#define EAO_YOLOX_NUM_CLASSES %s " % lit["NUM_CLASS"] in hdr
    assert "#define EAO_YOLOX_PAD %s " % lit["PAD"] in hdr


def test_the_yardstick_and_the_host_header_hold_the_literals():
    import yolox_reference as Y
    lit = RL.literals("yolox")
    assert [float(lit[k]) for k in ("MEAN_R", "MEAN_G", "MEAN_B")] == [0.485, 0.456, 0.406] and tuple(np.float32(float(lit[k])) for k in ("MEAN_R", "MEAN_G", "MEAN_B")) == Y.MEAN
    assert tuple(np.float32(float(lit[k])) for k in ("STD_R", "STD_G", "STD_B")) == Y.STD
    assert Y.STRIDES == tuple(int(lit[k]) for k in ("STRIDE_0", "STRIDE_1", "STRIDE_2")) and Y.PAD == int(lit["PAD"])
    assert Y.TRACKING_MIN_PROB == float(lit["TRACKING_MIN_PROB"]) and Y.TRACKING_CLASSES == tuple(int(lit["TRACKING_CLASS_%d" % k]) for k in range(14))
    assert Y.CONF == np.float32(float(lit["BBOX_CONF_THRESH"])) and Y.NMS == np.float32(float(lit["NMS_THRESH"]))
    h = open(os.path.join(ROOT, "eao_fusion_amd", "csrc", "yolox_internal.h")).read()
    for text in ("kMean[3] = {(float)%s, (float)%s, (float)%s}" % tuple(lit[k] for k in ("MEAN_R", "MEAN_G", "MEAN_B")),
                 "kStd[3] = {(float)%s, (float)%s, (float)%s}" % tuple(lit[k] for k in ("STD_R", "STD_G", "STD_B")),
                 "kStrides[3] = {%s, %s, %s}" % tuple(lit[k] for k in ("STRIDE_0", "STRIDE_1", "STRIDE_2")),
                 "kConfThresh = (float)%s;" % lit["BBOX_CONF_THRESH"], "kNmsThresh = (float)%s;" % lit["NMS_THRESH"], "kPad = %s;" % lit["PAD"],
                 "kTrackingMinProb = %s;" % lit["TRACKING_MIN_PROB"],
                 "kTrackingClasses[14] = {%s}" % ", ".join(lit["TRACKING_CLASS_%d" % k] for k in range(14))):
        assert text in h, text


def test_record_layouts(built):
    from eao_fusion_amd import yolox
    assert C.sizeof(built.YoloxCfg) == 24 and yolox.OBJECT.itemsize == 24
    assert [yolox.OBJECT.fields[k][1] for k in ("x", "y", "w", "h", "prob", "label")] == [0, 4, 8, 12, 16, 20]
    assert yolox.num_anchors(640) == 8400 and yolox.num_anchors(64) == 84


def test_no_handle_without_a_device(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from eao_fusion_amd import yolox
    with pytest.raises(built.EaoError) as e:
        yolox.Yolox()
    assert e.value.status == built.EAO_ERR_NO_DEVICE
    with pytest.raises(built.EaoError) as e:
        yolox.Yolox(input_size=100)      # (arguments are checked first)
    assert e.value.status == built.EAO_ERR_INVALID
