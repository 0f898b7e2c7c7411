"""KeyFrameDatabase on the device: the time of eao_keyframe_db_add, eao_keyframe_db_intersect and both kinds of eao_keyframe_db_query_scores over 1000, 5000 and
20 000 resident keyframes x about 1000 words over 10^6 word ids.  A quarter of every vector's draws fall on the first thousandth of the ids, so that the lists of
upstream's inverted file would be uneven.  Host wall clock around the C entry points (ctypes, arrays packed beforehand); every call ends in the stream's wait.
Median (min .. max) of --reps calls behind --warmup.  Beside them:
  today's route   eao_bow_score_l1 of the query against the same vectors UPLOADED with the call (all of them, and the 64 a host walk might leave);
  host walk       tools/keyframe_database_walk.cpp built -O3 here, `bench`: real inverted lists, upstream's walk and L1Scoring::score over std::map, one thread,
                  its own draw of the same distribution.
The kernel stages the query's ids in LDS; the form that probed global memory instead was measured once against it and dropped (the A/B section at the end of
profiles/keyframe_database_timing.txt is that measurement, kept from the run that made it).
A record only: nothing is gated; the parent commit has no such call and the reference's class needs OpenCV and DBoW2.

    python tools/bench_keyframe_database.py [--reps 50] [--warmup 10] [--out profiles/keyframe_database_timing.txt]
"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (first: both runtimes resolve the same libamdhip64)

from eao_fusion_amd import _lib  # noqa: E402
from eao_fusion_amd.keyframe_database import KeyFrameDatabase  # noqa: E402

N_WORDS = 1000000
SIZES = (1000, 5000, 20000)


def draw(rs, n=1000):
    hot = rs.randint(0, N_WORDS // 1000, n // 4)
    ids = np.unique(np.concatenate([hot, rs.randint(0, N_WORDS, n - len(np.unique(hot)))])).astype(np.uint32)
    v = rs.uniform(0.2, 1.0, len(ids))
    return ids, v / v.sum()


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return np.array(out)


def spread(v):
    return "%8.3f (%.3f .. %.3f)" % (np.median(v), v.min(), v.max())


def measure(n_kf, reps, warmup):
    L, p = _lib.load(), _lib.ptr
    rs = np.random.RandomState(n_kf)
    vecs = [draw(rs) for _ in range(n_kf)]
    db = KeyFrameDatabase(N_WORDS)
    t_add = []
    for k, (ids, vals) in enumerate(vecs):
        t0 = time.perf_counter()
        st = L.eao_keyframe_db_add(db.h, k + 1, len(ids), p(ids), p(vals))
        t_add.append((time.perf_counter() - t0) * 1e3)
        _lib.check(st)
    qi, qv = draw(rs)
    ids, common, first, score = np.zeros(n_kf, np.uint64), np.zeros(n_kf, np.int32), np.zeros(n_kf, np.uint32), np.zeros(n_kf, np.float64)
    n = C.c_int32(0)
    t_int = timed(lambda: L.eao_keyframe_db_intersect(db.h, len(qi), p(qi), p(qv), n_kf, p(ids), p(common), p(first), p(score), C.byref(n)), reps, warmup)
    assert n.value == n_kf and common.max() > 0
    lines = ["%6d keyframes, %d stored words (%.1f MB resident)" % (n_kf, db.info()["n_stored_words"], db.info()["n_stored_words"] * 12 / 1e6),
             "    add (one keyframe, about 1000 words)                   %s   the %d adds, arena growth included: %.1f ms" % (spread(np.array(t_add[-200:])), n_kf, sum(t_add)),
             "    intersect (kernel + 16 B per keyframe back)            %s" % spread(t_int)]
    keep = dict(a=np.zeros(n_kf, np.uint64), b=np.zeros(n_kf, np.int32), c=np.zeros(n_kf, np.uint64), d=np.zeros(n_kf, np.float32))
    R = _lib.KeyFrameDbScored()
    R.sharing_id, R.sharing_words, R.scored_id, R.scored_score = p(keep["a"]), p(keep["b"]), p(keep["c"]), p(keep["d"])
    conn = np.arange(1, 11, dtype=np.uint64)
    qid = [100]
    for kind, label in ((0, "query_scores, DetectLoopCandidates, 10 connected      "), (1, "query_scores, DetectRelocalizationCandidates          ")):
        def call():
            qid[0] += 1      # a new query id per call, as upstream's frames and keyframes have
            Q = _lib.KeyFrameDbQuery(kind, qid[0], len(qi), p(qi), p(qv), len(conn) if kind == 0 else 0, p(conn) if kind == 0 else None, 0.01)
            assert L.eao_keyframe_db_query_scores(db.h, C.byref(Q), n_kf, C.byref(R)) == 0
        t = timed(call, reps, warmup)
        lines.append("    %s %s   (%d listed, %d scored)" % (label, spread(t), R.n_sharing, R.n_scores))
    # today's route: the stored vectors travel with every call
    start = np.zeros(n_kf + 1, np.int32)
    start[1:] = np.cumsum([len(v[0]) for v in vecs])
    di, dv = np.concatenate([v[0] for v in vecs]), np.concatenate([v[1] for v in vecs])
    up = np.zeros(n_kf, np.float64)
    for m, r in ((n_kf, max(reps // 5, 5)), (64, reps)):
        t = timed(lambda: L.eao_bow_score_l1(len(qi), p(qi), p(qv), m, p(start), p(di), p(dv), p(up)), r, min(warmup, 3))
        lines.append("    eao_bow_score_l1, %6d vectors uploaded with the call %s" % (m, spread(t)))
        if m == n_kf:
            assert np.array_equal(up.view(np.uint64), score.view(np.uint64)), "resident and uploaded scores differ"
    return lines, score.copy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "no device: nothing is measured without one"
    lines = ["# tools/bench_keyframe_database.py --reps %d --warmup %d: milliseconds, median (min .. max); host wall clock around the C entry points, each call ends in the stream's wait" % (a.reps, a.warmup),
             "# vectors of about 1000 words over %d word ids, a quarter of the draws on the first %d ids; query: one more draw" % (N_WORDS, N_WORDS // 1000)]
    for n_kf in SIZES:
        lines += measure(n_kf, a.reps, a.warmup)[0]
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "keyframe_database_walk")
        subprocess.check_call(["g++", "-O3", "-std=c++17", os.path.join(ROOT, "tools", "keyframe_database_walk.cpp"), "-o", exe])
        lines.append("# host walk (1 thread, -O3): real inverted lists + L1Scoring::score over std::map, DetectRelocalizationCandidates up to lScoreAndMatch")
        for n_kf in SIZES:
            lines.append(subprocess.run([exe, "bench", str(n_kf), "1000", str(N_WORDS), str(min(a.reps, 20))], capture_output=True, text=True, check=True).stdout.strip())
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
