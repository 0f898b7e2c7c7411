#!/usr/bin/env python3
"""Records what the REFERENCE's own include/isolation_forest.h computes on the scenes of tests/isolation_forest_scenes.py into
tests/golden/isolation_forest/<scene>.npz: the points, the parameters, the bytes of IsolationForest::Serialize and the anomaly scores.

tools/isolation_forest_ref_driver.cpp (this project's text) is compiled against the reference header, reached through -I only, into a temporary directory;
nothing compiled from the reference is kept.  Scenes marked by_hash store the SHA-256 of the stream in place of its bytes.

    python tools/gen_golden_isolation_forest.py <reference tree>          # writes the fixtures
    python tools/gen_golden_isolation_forest.py <reference tree> --check  # recomputes and compares, writes nothing
"""
import hashlib
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden", "isolation_forest")
DRIVER = os.path.join(ROOT, "tools", "isolation_forest_ref_driver.cpp")


def build_driver(ref, tmp, opt="-O2"):
    exe = os.path.join(tmp, "isolation_forest_ref_driver")
    subprocess.check_call(["g++", opt, "-std=c++17", "-I", os.path.join(ref, "include"), DRIVER, "-o", exe])
    return exe


def scene_line(sc, prefix=""):
    p = np.ascontiguousarray(sc["points"], np.float32)
    return "%s%d %d %d %d %s\n" % (prefix, sc["tree_count"], sc["seed"], sc["sample_size"], len(p), " ".join("%08x" % v for v in p.reshape(-1).view(np.uint32)))


def run_reference(exe, sc):
    out = subprocess.run([exe], input=scene_line(sc), capture_output=True, text=True, check=True).stdout.strip().split("\n")
    if out[0] != "built 1":
        raise SystemExit("the reference did not build a forest: %r" % out[0])
    _, nbytes, hexs = out[1].split()
    stream = np.frombuffer(bytes.fromhex(hexs), np.uint8)
    assert len(stream) == int(nbytes)
    sc_tok = out[2].split()
    scores = np.array([int(h, 16) for h in sc_tok[2:]], np.uint64).view(np.float64)
    assert len(scores) == int(sc_tok[1]) == len(sc["points"])
    return stream, scores


def record(sc, stream, scores):
    rec = dict(points=np.ascontiguousarray(sc["points"], np.float32), tree_count=np.int64(sc["tree_count"]), seed=np.int64(sc["seed"]),
               sample_size=np.int64(sc["sample_size"]), class_id=np.int64(sc["class_id"]), scores=scores, stream_len=np.int64(len(stream)),
               stream_sha256=np.frombuffer(hashlib.sha256(stream.tobytes()).hexdigest().encode(), np.uint8))
    if not sc.get("by_hash"):
        rec["stream"] = stream
    return rec


def same(a, b):
    return set(a) == set(b) and all(np.asarray(a[k]).dtype == np.asarray(b[k]).dtype and np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)


def main():
    if len(sys.argv) < 2:
        raise SystemExit(__doc__)
    import isolation_forest_scenes as SC
    ref, check = sys.argv[1], "--check" in sys.argv
    bad = []
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(ref, tmp)
        for name, sc in sorted(SC.scenes().items()):
            rec = record(sc, *run_reference(exe, sc))
            path = os.path.join(OUT, name + ".npz")
            if check:
                z = np.load(path)
                if not same(rec, {k: z[k] for k in z.files}):
                    bad.append(name)
            else:
                os.makedirs(OUT, exist_ok=True)
                np.savez_compressed(path, **rec)
                print("wrote %s (%d bytes; stream %d bytes, %d points)" % (path, os.path.getsize(path), int(rec["stream_len"]), len(sc["points"])))
    if bad:
        raise SystemExit("fixture and reference differ: %s" % ", ".join(bad))
    if check:
        print("ok")


if __name__ == "__main__":
    main()
