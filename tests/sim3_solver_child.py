"""One family of sim3_solver_scenes through eao_sim3_solver_iterate in a process of its own (tests/test_gpu_sim3_solver.py starts it with
subprocess: a library that has never run anything else), every output printed as hex.

    python tests/sim3_solver_child.py FAMILY
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def result_bytes(o):
    """Every output of eao_sim3_solver_iterate (the inspection arrays where present), bit for bit."""
    s = o["state"]
    parts = [np.array([o["returned"], o["n_inliers"], int(o["no_more"]), s["iterations"], s["best_inliers"]], np.int32), np.asarray(o["T12"], np.float32),
             np.asarray(o["inlier"], np.uint8), np.asarray(s["best_T12"], np.float32), np.asarray(s["best_R"], np.float32), np.asarray(s["best_t"], np.float32),
             np.float32(s["best_s"])]
    for k in ("hyp_inliers", "hyp_T12", "hyp_T21", "hyp_inlier"):
        if k in o:
            parts.append(np.ascontiguousarray(o[k]))
    return b"".join(np.ascontiguousarray(p).tobytes() for p in parts)


def family(name):
    import sim3_solver_scenes as SC
    return dict(SC.all_families())[name]()


def main():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from eao_fusion_amd.sim3_solver import sim3_solver_iterate
    prob, triples = family(sys.argv[1])
    sys.stdout.write(result_bytes(sim3_solver_iterate(prob, None, triples, inspect=True)).hex() + "\n")


if __name__ == "__main__":
    main()
