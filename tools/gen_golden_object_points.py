#!/usr/bin/env python3
"""Writes tests/golden/object_points/results.npz from the yardstick (tests/object_points_reference.py, the device's form) over every scene of
tests/object_points_scenes.py.  Per scene: the record as bytes, every output array, and `variant` (whether the alternative readings of OpenCV give another
result).  The scenes are seeded, so the file holds results only.

    python tools/gen_golden_object_points.py            # writes
    python tools/gen_golden_object_points.py --check    # compares, writes nothing
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import object_points_reference as Y  # noqa: E402
import object_points_scenes as SC  # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "object_points", "results.npz")
ARRAYS = ("gate", "target", "count", "list", "erased", "survivors", "points")


def unpack(z, name):
    """a recorded scene -> (result, variant)"""
    res = dict(rec=np.frombuffer(z[name + ".record"].tobytes(), Y.RECORD_DTYPE)[0])
    if res["rec"]["status"] == Y.DONE:
        for k in ARRAYS:
            res[k] = z[name + "." + k]
    return res, bool(z[name + ".variant"])


def build(results, scenes):
    out = {}
    for name, res in sorted(results.items()):
        out[name + ".record"] = np.frombuffer(res["rec"].tobytes(), np.uint8)
        out[name + ".variant"] = np.uint8(Y.variant(scenes[name]))
        for k in ARRAYS:
            if k in res:
                out[name + "." + k] = res[k]
    return out


def same_as_recorded(z, out):
    """the keys that differ: floats bit for bit with a NaN as a NaN, everything else by value"""
    if set(z.files) != set(out):
        return sorted(set(z.files) ^ set(out))
    bad = []
    for k in out:
        if k.endswith(".record"):
            ok = Y.same_record(np.frombuffer(z[k].tobytes(), Y.RECORD_DTYPE)[0], np.frombuffer(out[k].tobytes(), Y.RECORD_DTYPE)[0])
        elif k.endswith(".points"):
            ok = Y.same_float(z[k], out[k])
        else:
            ok = np.array_equal(z[k], out[k])
        if not ok:
            bad.append(k)
    return bad


def main():
    scenes = SC.scenes()
    out = build({name: Y.device(s) for name, s in scenes.items()}, scenes)
    if "--check" in sys.argv:
        bad = same_as_recorded(np.load(PATH), out)
        if bad:
            raise SystemExit("differs: %s" % ", ".join(bad[:10]))
        print("ok")
        return
    os.makedirs(os.path.dirname(PATH), exist_ok=True)
    np.savez_compressed(PATH, **out)
    print("wrote", PATH, os.path.getsize(PATH), "bytes")


if __name__ == "__main__":
    main()
