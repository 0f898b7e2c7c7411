#!/usr/bin/env python3
"""Writes tests/golden/object_chain/results.npz from the yardstick (tests/object_chain_reference.py, the device's form) over every scene of
tests/object_chain_scenes.py.  Per scene: the three records as bytes and every output array behind the points' own (those are a function of the seeded scene
that tests/golden/object_points already pins by kind; here only the final list onwards is kept, and the forest's flags packed).  The scenes are seeded, so the
file holds results only.

    python tools/gen_golden_object_chain.py            # writes
    python tools/gen_golden_object_chain.py --check    # compares, writes nothing
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import object_chain_reference as Y  # noqa: E402
import object_chain_scenes as SC  # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "object_chain", "results.npz")
POINTS_ARRAYS = ("gate", "target", "count", "erased")


def unpack(z, name):
    """a recorded scene -> the part of a result that is recorded"""
    res = dict(rec=np.frombuffer(z[name + ".record"].tobytes(), Y.OP.RECORD_DTYPE)[0])
    if res["rec"]["status"] == Y.OP.DONE:
        for k in POINTS_ARRAYS:
            res[k] = z[name + "." + k]
        res["chain"] = np.frombuffer(z[name + ".chain"].tobytes(), Y.RECORD_DTYPE)[0]
        res["cuboid"] = np.frombuffer(z[name + ".cuboid"].tobytes(), Y.OC.RECORD_DTYPE)[0]
        nf = int(res["chain"]["n_final"])
        res["final"] = z[name + ".final"].astype(np.int32).reshape(-1, 2)
        res["forest_flags"] = np.unpackbits(z[name + ".forest_flags"])[:nf]
        res["scores"] = z[name + ".scores"]
    return res


def recorded_part(res):
    """the same part of a full result, for differences()"""
    keep = ("rec",) + POINTS_ARRAYS + ("chain", "cuboid", "final", "forest_flags", "scores")
    return {k: v for k, v in res.items() if k in keep}


def build(results):
    out = {}
    for name, res in sorted(results.items()):
        out[name + ".record"] = np.frombuffer(res["rec"].tobytes(), np.uint8)
        if "chain" not in res:
            continue
        for k in POINTS_ARRAYS:
            out[name + "." + k] = res[k]
        out[name + ".chain"] = np.frombuffer(res["chain"].tobytes(), np.uint8)
        out[name + ".cuboid"] = np.frombuffer(res["cuboid"].tobytes(), np.uint8)
        out[name + ".final"] = res["final"].astype(np.uint8 if res["final"].size and res["final"].max() < 256 else np.uint16 if res["final"].size else np.uint8)
        out[name + ".forest_flags"] = np.packbits(res["forest_flags"])
        out[name + ".scores"] = res["scores"]
    return out


def main():
    scenes = SC.scenes()
    results = {name: Y.chain(s, "device") for name, s in scenes.items()}
    out = build(results)
    if "--check" in sys.argv:
        z = np.load(PATH)
        bad = sorted(set(z.files) ^ set(out)) or [n for n in scenes if Y.differences(recorded_part(results[n]), unpack(z, n))]
        if bad:
            raise SystemExit("differs: %s" % ", ".join(bad[:10]))
        print("ok")
        return
    os.makedirs(os.path.dirname(PATH), exist_ok=True)
    np.savez_compressed(PATH, **out)
    print("wrote", PATH, os.path.getsize(PATH), "bytes")


if __name__ == "__main__":
    main()
