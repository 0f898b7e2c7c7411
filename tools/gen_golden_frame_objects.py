#!/usr/bin/env python3
"""Writes tests/golden/frame_objects/results.npz from the yardstick (tests/frame_objects_reference.py, the compact form -- the one whose zero signs the device
shares) over every scene of tests/frame_objects_scenes.py.  Per scene: the records as bytes, both lists in CSR form, and `variant`: per box whether plain IEEE
sum / (float)n gives another _Pos than the convertTo reading.  The scenes are seeded, so the file holds results only.

    python tools/gen_golden_frame_objects.py            # writes
    python tools/gen_golden_frame_objects.py --check    # compares, writes nothing
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import frame_objects_reference as Y  # noqa: E402
import frame_objects_scenes as SC  # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "frame_objects", "results.npz")


def csr(lists):
    start = np.zeros(len(lists) + 1, np.int32)
    start[1:] = np.cumsum([len(l) for l in lists])
    return start, np.concatenate([np.asarray(l, np.int32) for l in lists] + [np.zeros(0, np.int32)])


def pack(name, res):
    sa, la = csr(res["assigned"])
    sk, lk = csr(res["kept"])
    return {name + ".records": np.frombuffer(res["records"].tobytes(), np.uint8), name + ".assigned_start": sa, name + ".assigned": la,
            name + ".kept_start": sk, name + ".kept": lk, name + ".variant": np.asarray(res["variant"], np.uint8)}


def unpack(z, name):
    """a recorded scene -> the yardstick's result form"""
    rec = np.frombuffer(z[name + ".records"].tobytes(), Y.RECORD_DTYPE)
    sa, la, sk, lk = (z[name + k] for k in (".assigned_start", ".assigned", ".kept_start", ".kept"))
    return dict(records=rec, assigned=[la[sa[k]:sa[k + 1]] for k in range(len(rec))], kept=[lk[sk[k]:sk[k + 1]] for k in range(len(rec))],
                variant=[bool(v) for v in z[name + ".variant"]])


def main():
    out = {}
    for name, (fr, _reaches) in sorted(SC.scenes().items()):
        out.update(pack(name, Y.compact(fr)))
    if "--check" in sys.argv:
        z = np.load(PATH)
        bad = [k for k in out if k not in z.files or not np.array_equal(z[k], out[k])]
        if bad or set(z.files) != set(out):
            raise SystemExit("differs: %s" % ", ".join(bad[:10]))
        print("ok")
        return
    os.makedirs(os.path.dirname(PATH), exist_ok=True)
    np.savez_compressed(PATH, **out)
    print("wrote", PATH, os.path.getsize(PATH), "bytes")


if __name__ == "__main__":
    main()
