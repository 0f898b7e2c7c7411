"""Writes tests/golden/detnet/: the head output of the whole networks of the device tests (tests/detnet_models.py NETS, frame 0 at S = 64), computed by the numpy
yardstick (tests/detnet_reference.py) and checked against the host walk (tools/detnet_walk.cpp, -O2) before it is written.  The files hold recorded outputs
only; the models come from seeds.

    python tools/gen_golden_detnet.py [--check]      --check: compare with the files instead of writing them"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import detnet_models as M  # noqa: E402
import detnet_reference as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "detnet")


def main():
    check = "--check" in sys.argv[1:]
    os.makedirs(OUT, exist_ok=True)
    exe = M.walk_binary(("-O2",))
    for name in sorted(M.NETS):
        model, blobs = M.net_inputs(name)
        head = R.forward(model, 64, blobs[0])[1]
        walked = M.walk_run(exe, model, 64, blobs[0])[1]
        assert not np.isnan(head).any() and head.view(np.uint32).tobytes() == walked.view(np.uint32).tobytes(), "%s: the yardstick and the walk differ" % name
        path = os.path.join(OUT, "yolox_%s_s64.npz" % name)
        if check:
            assert np.load(path)["head"].tobytes() == head.view(np.uint32).tobytes(), path
            print("ok", path)
        else:
            np.savez_compressed(path, head=head.view(np.uint32), depth_width_classes_seed=np.array(M.NETS[name], np.float64))
            print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
