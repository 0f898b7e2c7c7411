#!/usr/bin/env python3
"""Writes tests/golden/plane_association/<scene>.npz from the yardstick (tests/plane_association_reference.py) on scenes of tests/plane_association_scenes.py:
the inputs as the library takes them and the outputs it must return, bit for bit.  tests/test_gpu_plane_association.py replays them on the device.

    python tools/gen_golden_plane_association.py            # writes the fixtures
    python tools/gen_golden_plane_association.py --check    # compares, writes nothing
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import plane_association_reference as Y  # noqa: E402
import plane_association_scenes as SC  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "plane_association")
NAMES = ["room_0", "three_sets", "sizes", "nan_point", "tie_ba", "scaled_sim3", "same_id_twice"]


def pack(name):
    sc, r = SC.get(name), SC.reference(name)
    planes = sc["planes"]
    start = np.concatenate([[0], np.cumsum([len(p[2]) for p in planes])]).astype(np.int64)
    world_xyz = [Y.transform_cloud(p[2], p[3]) for p in planes]      # the literal loop, not the vectorised form
    return dict(
        plane_id=np.array([p[0] for p in planes], np.uint64), plane_world=np.array([p[1] for p in planes], np.float32).reshape(-1, 4),
        cloud_start=start, cloud_xyz=np.concatenate([p[2] for p in planes] + [np.zeros((0, 3), np.float32)]).astype(np.float32),
        has_Tcw=np.array([p[3] is not None for p in planes], np.uint8),
        Tcw=np.array([np.eye(4, dtype=np.float32) if p[3] is None else p[3] for p in planes], np.float32).reshape(-1, 4, 4),
        M=sc["M"], set_start=sc["set_start"], coef=sc["coef"], has_cand=np.uint8(sc["cand_id"] is not None),
        cand_id=np.array(sc["cand_id"] or [], np.uint64), dis_th=np.float32(sc["dis_th"]), angle_th=np.float32(sc["angle_th"]),
        expect_world_xyz=np.concatenate(world_xyz + [np.zeros((0, 3), np.float32)]).astype(np.float32),
        expect_world_coef=r["world_coef"], expect_gated=r["gated"], expect_dis=r["dis"], expect_match=r["match"], expect_match_dis=r["match_dis"])


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def main():
    check = "--check" in sys.argv
    os.makedirs(OUT, exist_ok=True)
    for name in NAMES:
        got, path = pack(name), os.path.join(OUT, name + ".npz")
        if check:
            want = np.load(path)
            bad = [k for k in got if not same(got[k], want[k])]
            if bad or set(want.files) != set(got):
                raise SystemExit("%s differs: %s" % (name, bad))
        else:
            np.savez_compressed(path, **got)
            print("wrote", path, os.path.getsize(path))
    if check:
        print("ok")


if __name__ == "__main__":
    main()
