"""The detector-network entry points at the drop-in boundary, without a device: the header declares them, the shared object exports them, the ctypes table binds
them, the record has the layout the Python mirror assumes, and a handle is refused for a bad file (EAO_ERR_INVALID) before the device is asked for
(EAO_ERR_NO_DEVICE for a good one)."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detnet_models as M  # noqa: E402

NAMES = ["eao_detnet_create", "eao_detnet_create_from_file", "eao_detnet_destroy", "eao_detnet_info", "eao_detnet_forward", "eao_detnet_tensor",
         "eao_detnet_set_tensor", "eao_detnet_set_profiling", "eao_detnet_last_op_ms"]


@pytest.fixture(scope="module")
def built():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "eao_fusion_amd", "csrc")])
    from eao_fusion_amd import _lib
    return _lib


def test_symbols_declared_exported_and_bound(built):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "eao_fusion.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(eao_detnet_[a-z0-9_]+)\s*\(", hdr)) == set(NAMES)
    L = built.load()
    for name in NAMES:
        assert hasattr(L, name) and built.SYMBOLS[name] is not None, name
    assert "#define EAO_ABI_VERSION 6" in open(os.path.join(ROOT, "include", "eao_fusion.h")).read() and L.eao_abi_version() == 6


def test_record_layout(built):
    d = built.DetnetDesc
    assert C.sizeof(d) == 48 and [getattr(d, k).offset for k in ("classes", "anchors", "tensors", "ops", "input_size", "max_batch", "weight_bytes", "activation_bytes",
                                                                  "flops")] == [0, 4, 8, 12, 16, 20, 24, 32, 40]


def test_every_entry_cites_the_reference():
    hdr = open(os.path.join(ROOT, "include", "eao_fusion.h")).read()
    sec = hdr[hdr.index("/* ---- The detector network"):hdr.index("/* The value of EAO_ABI_VERSION")]
    assert "src/YOLOX.cc:7-48" in sec and ":331-367" in sec and "include/YOLOX.h:92" in sec and ":359" in sec


def test_files_are_checked_before_the_device(built, tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from eao_fusion_amd import detnet
    good = M.scenes()["yolox_nano_width_32"]["model"].tobytes()
    with pytest.raises(built.EaoError) as e:
        detnet.Detnet(good, 64, 2)
    assert e.value.status == built.EAO_ERR_NO_DEVICE
    p = tmp_path / "model.bin"
    p.write_bytes(good)
    with pytest.raises(built.EaoError) as e:
        detnet.Detnet(str(p), 64, 2)
    assert e.value.status == built.EAO_ERR_NO_DEVICE
    for args in ((good, 48, 1), (good, 64, 0), (good, 64, 100000), (b"", 64, 1), (str(tmp_path / "missing.bin"), 64, 1)):
        with pytest.raises(built.EaoError) as e:
            detnet.Detnet(*args)
        assert e.value.status == built.EAO_ERR_INVALID, args[1:]
    for name, (data, S, word) in M.broken_files().items():
        with pytest.raises(built.EaoError) as e:
            detnet.Detnet(data, S, 1)
        assert e.value.status == built.EAO_ERR_INVALID and word in str(e.value), name
