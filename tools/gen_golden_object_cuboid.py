#!/usr/bin/env python3
"""Writes tests/golden/object_cuboid/results.npz from the yardstick (tests/object_cuboid_reference.py, the device's form -- the one whose zero signs the device
shares) over every scene of tests/object_cuboid_scenes.py.  Per object scene: the record as bytes, `variant` (whether the alternative readings give other bits)
and `zero_sign` (the names of the fields in which a tie between -0.0f and +0.0f at an extremum shows).  Per overlap scene: the verdict matrix and the extents.
The scenes are seeded, so the file holds results only.

    python tools/gen_golden_object_cuboid.py            # writes
    python tools/gen_golden_object_cuboid.py --check    # compares, writes nothing
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import object_cuboid_reference as Y  # noqa: E402
import object_cuboid_scenes as SC  # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "object_cuboid", "results.npz")


def unpack(z, name):
    """a recorded object scene -> (record, variant, zero-sign field names)"""
    rec = np.frombuffer(z[name + ".record"].tobytes(), Y.RECORD_DTYPE)[0]
    return rec, bool(z[name + ".variant"]), [s for s in str(z[name + ".zero_sign"]).split(",") if s]


def unpack_overlaps(z, name):
    return z["overlap." + name + ".verdict"], z["overlap." + name + ".extents"]


def same_as_recorded(z, out):
    """records with a NaN by isnan (its sign and payload are nobody's contract), everything else by value"""
    if set(z.files) != set(out):
        return sorted(set(z.files) ^ set(out))
    bad = []
    for k in out:
        if k.endswith(".record"):
            a, b = np.frombuffer(z[k].tobytes(), Y.RECORD_DTYPE)[0], np.frombuffer(out[k].tobytes(), Y.RECORD_DTYPE)[0]
            ok = Y.same_records(a, b)
        elif k.endswith(".extents"):
            ok = np.array_equal(z[k].view(np.uint32), out[k].view(np.uint32))
        else:
            ok = np.array_equal(z[k], out[k])
        if not ok:
            bad.append(k)
    return bad


def build():
    out = {}
    for name, o in sorted(SC.scenes().items()):
        out[name + ".record"] = np.frombuffer(Y.device(o).tobytes(), np.uint8)
        out[name + ".variant"] = np.uint8(Y.variant(o))
        out[name + ".zero_sign"] = np.array(",".join(Y.zero_sign_fields(o)))
    for name, (rows, eligible) in sorted(SC.overlap_scenes().items()):
        verdict, extents = Y.overlaps_literal(rows, eligible)
        out["overlap." + name + ".verdict"], out["overlap." + name + ".extents"] = verdict, extents
    return out


def main():
    out = build()
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
