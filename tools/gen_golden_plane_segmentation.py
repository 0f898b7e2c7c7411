#!/usr/bin/env python3
"""Writes tests/golden/plane_segmentation/<scene>.npz from the yardstick (tests/plane_segmentation_reference.py) over tests/plane_segmentation_scenes.py: the
files in full for the small scenes; for the VGA room the plane table and the small tables as they are and a SHA-256 of the block records, the membership image,
the claims and the clouds.  No device and no library is involved.  tests/test_plane_segmentation_reference_cpu.py holds the files to the yardstick."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import plane_segmentation_reference as R  # noqa: E402
import plane_segmentation_scenes as S  # noqa: E402


def golden_of(name, scene):
    big = name not in S.SMALL
    a = R.result_arrays(R.run(scene["cfg"], scene["depth"], vectorised=big))
    if big:
        for k in R.BULK:
            a["sha256_" + k] = R.digest(a.pop(k))
    return a


def main():
    out = os.path.join(ROOT, "tests", "golden", "plane_segmentation")
    os.makedirs(out, exist_ok=True)
    for name, scene in S.scenes().items():
        np.savez_compressed(os.path.join(out, name + ".npz"), **golden_of(name, scene))
        print(name, os.path.getsize(os.path.join(out, name + ".npz")))


if __name__ == "__main__":
    main()
