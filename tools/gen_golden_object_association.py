#!/usr/bin/env python3
"""Writes tests/golden/object_association/np.npz and rect.npz: what the yardstick (tests/object_association_reference.py, the literal transcription of
Object_2D::NoParaDataAssociation and Object_Map::ComputeProjectRectFrame) computes on every scene of tests/object_association_scenes.py.  The scenes are seeded and
rebuilt by the tests, so the files hold a digest of each scene's inputs and the results: per scene m, n, step, the nine counts, w and r as float32, the
verdict; u and v per point, the rect and its status.

    python tools/gen_golden_object_association.py          # writes the fixtures
    python tools/gen_golden_object_association.py --check  # compares, writes nothing
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import object_association_reference as Y      # noqa: E402
import object_association_scenes as SC        # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "object_association")
CAM = ("fx", "fy", "cx", "cy", "cols", "rows")


def digest(*arrays):
    """the bytes of a scene's inputs, so that a drifting scene generator shows as that and not as a wrong result"""
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return np.frombuffer(h.digest(), np.uint8).copy()


def compute():
    nps, rect = {}, {}
    for name, s in SC.np_scenes().items():
        g = Y.np_literal(s["det"], s["map"], s["S"])
        nps[name + ".mns"] = np.array([g["m"], g["n"], g["step"]], np.int32)
        nps[name + ".counts"] = g["counts"].astype(np.uint32)
        nps[name + ".w"] = g["w"].astype(np.float32)
        nps[name + ".r"] = g["r"].astype(np.float32)
        nps[name + ".verdict"] = np.int32(g["verdict"])
        nps[name + ".inputs"] = digest(s["det"], s["map"], np.int32(s["S"]))
    for name, s in SC.rect_scenes().items():
        st, rc, uv = Y.rect_literal(s["points"], s["Tcw"], **{k: s[k] for k in CAM})
        rect[name + ".status"] = np.uint8(st)
        rect[name + ".rect"] = np.zeros(4, np.int32) if rc is None else rc.astype(np.int32)
        rect[name + ".uv"] = uv.astype(np.float32)
        rect[name + ".inputs"] = digest(s["points"], s["Tcw"], np.array([s[k] for k in CAM], np.float32))
    return {"np": nps, "rect": rect}


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def main():
    got = compute()
    if "--check" in sys.argv:
        for stem, arrays in got.items():
            z = np.load(os.path.join(GOLD, stem + ".npz"))
            if sorted(z.files) != sorted(arrays) or not all(same(z[k], v) for k, v in arrays.items()):
                raise SystemExit("%s.npz and the yardstick differ" % stem)
        print("ok")
        return
    os.makedirs(GOLD, exist_ok=True)
    for stem, arrays in got.items():
        np.savez_compressed(os.path.join(GOLD, stem + ".npz"), **arrays)
        print("wrote", os.path.join(GOLD, stem + ".npz"))


if __name__ == "__main__":
    main()
