"""One problem of sim3_scenes.CALL_ORDER through eao_optimize_sim3 in a process of its own (tests/test_gpu_sim3.py starts it with
subprocess: a library that has never run anything else), the result printed as hex.

    python tests/sim3_child.py INDEX
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def result_bytes(o):
    """Every output of eao_optimize_sim3, bit for bit."""
    return (np.asarray(o["q"], np.float64).tobytes() + np.asarray(o["t"], np.float64).tobytes() + np.float64(o["s"]).tobytes()
            + np.asarray(o["removed"], np.uint8).tobytes() + np.asarray(o["iters"], np.int32).tobytes()
            + bytes([int(o["n_inliers"]) & 255, int(o["n_inliers"]) >> 8 & 255, int(o["n_inliers"]) >> 16 & 255, int(bool(o["early_exit"]))]))


def main():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import sim3_scenes as SC
    from eao_fusion_amd.optimizer import optimize_sim3
    kw, edit = SC.CALL_ORDER[int(sys.argv[1])]
    sys.stdout.write(result_bytes(optimize_sim3(SC.irregular_scene(kw, edit))).hex() + "\n")


if __name__ == "__main__":
    main()
