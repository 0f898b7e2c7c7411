"""ORBVocabulary on the device: the time of eao_vocabulary_transform per frame (n = 1000 descriptors) and of eao_vocabulary_transform_batch over 64 such frames on
a tree of ORBvoc's shape (complete k = 10, L = 6: 1,111,110 nodes, 35.6 MB of node descriptors, random bytes, generated in memory), and of eao_bow_score_l1 of one
query against 64 stored vectors.  Host wall clock around the Python binding; every call ends in the stream's wait.  Reported separately:
  first     the first call on a new handle (code objects loaded by a warm-up on ANOTHER handle; the table was only ever written by the upload),
  evicted   a call after 1 GiB was streamed through the device (more than the 256 MiB Infinity Cache holds), --reps times,
  resident  back-to-back calls, the median of --reps behind --warmup.
Beside it a single-threaded -O3 host walk of the same flattened table over the same descriptors (tools/vocabulary_walk.cpp, built here: this project's own code,
the descent only, without the sorts and sums): its first pass and the fastest of its passes.  It must reach the device's words.  A record only: nothing is gated, the
parent commit has nothing to compare against, and the reference's DBoW2 needs OpenCV.

    python tools/bench_vocabulary.py [--reps 50] [--warmup 10] [--out profiles/vocabulary_timing.txt]
"""
import argparse
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402  (first: both runtimes resolve the same libamdhip64)

from eao_fusion_amd.vocabulary import Vocabulary, score_l1  # noqa: E402
import vocabulary_scenes as SC  # noqa: E402


def ms(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def spread(v):
    v = np.asarray(v)
    return "%8.3f (%.3f .. %.3f)" % (np.median(v), v.min(), v.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "no device: nothing is measured without one"
    sc = SC.orbvoc(n=64 * 1000, seed=21)
    desc, feats = sc["desc"], sc["features"]
    frames = [feats[f * 1000:(f + 1) * 1000] for f in range(64)]
    lines = ["# tools/bench_vocabulary.py --reps %d --warmup %d: milliseconds, median (min .. max); host wall clock of the Python binding, each call ends in the stream's wait" % (a.reps, a.warmup),
             "# tree: complete k = 10, L = 6, %d nodes, %.1f MB of node descriptors; levelsup 4; TF_IDF, L1" % (len(desc["parent"]), desc["descriptor"].nbytes / 1e6)]
    warm = Vocabulary(SC.k10_l3()["desc"])      # loads the code objects, creates this thread's stream and scratch
    warm.transform(frames[0], 2)
    warm.transform_batch(frames[:2], 2)
    t_create, voc = ms(lambda: Vocabulary(desc))
    lines.append("eao_vocabulary_create (flatten + upload)   %8.1f" % t_create)
    t_first, r0 = ms(lambda: voc.transform(frames[0], 4))
    lines.append("transform n=1000, first call on the handle %8.3f" % t_first)
    flush = torch.empty(1 << 28, dtype=torch.float32, device="cuda")      # 1 GiB

    def evict():
        flush.add_(1.0)
        torch.cuda.synchronize()

    ev = []
    for i in range(a.reps):
        evict()
        ev.append(ms(lambda: voc.transform(frames[i % 64], 4))[0])
    lines.append("transform n=1000, evicted                  " + spread(ev))
    for _ in range(a.warmup):
        voc.transform(frames[0], 4)
    lines.append("transform n=1000, resident, same frame     " + spread([ms(lambda: voc.transform(frames[0], 4))[0] for _ in range(a.reps)]))
    lines.append("transform n=1000, resident, frames in turn " + spread([ms(lambda: voc.transform(frames[i % 64], 4))[0] for i in range(a.reps)]))
    evb = []
    for i in range(max(a.reps // 5, 3)):
        evict()
        evb.append(ms(lambda: voc.transform_batch(frames, 4))[0])
    lines.append("batch of 64 x 1000, evicted                " + spread(evb))
    for _ in range(a.warmup):
        voc.transform_batch(frames, 4)
    tb = [ms(lambda: voc.transform_batch(frames, 4))[0] for _ in range(a.reps)]
    lines.append("batch of 64 x 1000, resident               " + spread(tb) + "   = %.3f per frame" % (np.median(tb) / 64))
    rb = voc.transform_batch(frames, 4)
    q = (rb[0]["word_id"], rb[0]["word_value"])
    stored = [(r["word_id"], r["word_value"]) for r in rb]
    for _ in range(a.warmup):
        score_l1(q, stored)
    lines.append("score_l1, 1 query x 64 stored vectors      " + spread([ms(lambda: score_l1(q, stored))[0] for _ in range(a.reps)]))
    # the host walk of the same table over frame 0 and over all 64 frames
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "vocabulary_walk")
        subprocess.check_call(["g++", "-O3", "-std=c++17", os.path.join(ROOT, "tools", "vocabulary_walk.cpp"), "-o", exe])
        for label, fs, reps in (("n=1000", frames[0], 20), ("64 x 1000", feats, 3)):
            blob = (np.array([len(desc["parent"]), len(fs), 4], np.int32).tobytes() + desc["parent"].tobytes() + desc["descriptor"].tobytes() + desc["weight"].tobytes()
                    + desc["is_leaf"].tobytes() + np.ascontiguousarray(fs).tobytes())
            with open(os.path.join(tmp, "in.bin"), "wb") as f:
                f.write(blob)
            out = subprocess.run([exe, os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin"), str(reps)], capture_output=True, text=True, check=True).stdout.split()
            words = np.frombuffer(open(os.path.join(tmp, "out.bin"), "rb").read()[:4 * len(fs)], np.uint32)
            dev = r0["feat_word"] if len(fs) == 1000 else np.concatenate([r["feat_word"] for r in rb])
            assert np.array_equal(words, dev), "the host walk and the device disagree"
            lines.append("host walk (1 thread, -O3, descent only) %-10s first pass %8.3f   fastest of %d %8.3f" % (label, float(out[1]), reps, float(out[3])))
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
