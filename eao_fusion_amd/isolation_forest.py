"""Object_Map::IsolationForestDeleteOutliers (reference src/Object.cc:1239-1348, include/isolation_forest.h) through eao_iforest_scores_batch and
eao_object_iforest_outliers_batch (csrc/iforest.hip): the ctypes mirror the tests and tools/bench_isolation_forest.py use.

An object is an (n, 3) float32 array of its map points' world positions in vector order."""
import ctypes as C

import numpy as np

from . import _lib


def _pack(objects):
    pts = [np.ascontiguousarray(o, np.float32).reshape(-1, 3) for o in objects]
    start = np.zeros(len(pts) + 1, np.int32)
    start[1:] = np.cumsum([len(p) for p in pts])
    xyz = np.ascontiguousarray(np.concatenate(pts) if pts else np.zeros((0, 3), np.float32), np.float32)
    if len(xyz) == 0:
        xyz = np.zeros((1, 3), np.float32)
    return start, xyz


def scores_batch(objects, tree_count, seed, sample_size, want_stream=False, stream_cap=None):
    """IsolationForest::Build + GetAnomalyScores per object.  tree_count / seed / sample_size: one value per object (or one for all).  Returns a list of
    dict(scores, total_path_len[, stream]) per object; stream is the bytes of IsolationForest::Serialize.  stream_cap: the stream buffer's size in bytes instead of
    the size asked from the library first (for the capacity test)."""
    n = len(objects)
    start, xyz = _pack(objects)
    tc = np.ascontiguousarray(np.broadcast_to(np.asarray(tree_count, np.int32), (n,)))
    sd = np.ascontiguousarray(np.broadcast_to(np.asarray(seed, np.uint32), (n,)))
    ss = np.ascontiguousarray(np.broadcast_to(np.asarray(sample_size, np.int32), (n,)))
    total = int(start[-1])
    scores, tot = np.zeros(max(total, 1), np.float64), np.zeros(max(total, 1), np.float64)
    L = _lib.load()
    sstart = np.zeros(n + 1, np.int64)
    stream = None
    if want_stream:
        if stream_cap is None:
            _lib.check(L.eao_iforest_scores_batch(n, _lib.ptr(start), _lib.ptr(xyz), _lib.ptr(tc), _lib.ptr(sd), _lib.ptr(ss), _lib.ptr(scores), None, None, 0,
                                                  _lib.ptr(sstart)))
            stream_cap = int(sstart[-1])
        stream = np.zeros(max(stream_cap, 1), np.uint8)
    _lib.check(L.eao_iforest_scores_batch(n, _lib.ptr(start), _lib.ptr(xyz), _lib.ptr(tc), _lib.ptr(sd), _lib.ptr(ss), _lib.ptr(scores), _lib.ptr(tot),
                                          _lib.ptr(stream), stream_cap or 0, _lib.ptr(sstart) if want_stream else None))
    out = []
    for j in range(n):
        r = dict(scores=scores[start[j]:start[j + 1]].copy(), total_path_len=tot[start[j]:start[j + 1]].copy())
        if want_stream:
            r["stream"] = stream[sstart[j]:sstart[j + 1]].tobytes()
        out.append(r)
    return out


def scores(points, tree_count, seed, sample_size, want_stream=False):
    return scores_batch([points], tree_count, seed, sample_size, want_stream)[0]


def outliers_batch(objects, class_ids, bi_forest=True, want_scores=False):
    """The whole of upstream's function per object: a list of dict(flags (n,) uint8, removed[, scores])."""
    n = len(objects)
    start, xyz = _pack(objects)
    cls = np.ascontiguousarray(class_ids, np.int32).reshape(n)
    total = int(start[-1])
    flags, removed = np.zeros(max(total, 1), np.uint8), np.zeros(max(n, 1), np.int32)
    sc = np.zeros(max(total, 1), np.float64) if want_scores else None
    _lib.check(_lib.load().eao_object_iforest_outliers_batch(n, _lib.ptr(start), _lib.ptr(xyz), _lib.ptr(cls), 1 if bi_forest else 0, _lib.ptr(flags),
                                                             _lib.ptr(removed), _lib.ptr(sc)))
    out = []
    for j in range(n):
        r = dict(flags=flags[start[j]:start[j + 1]].copy(), removed=int(removed[j]))
        if want_scores:
            r["scores"] = sc[start[j]:start[j + 1]].copy()
        out.append(r)
    return out


def delete_outliers(points, class_id, bi_forest=True):
    """Object_Map::IsolationForestDeleteOutliers over one object: the points that stay, in order, and the erased indices."""
    r = outliers_batch([points], [class_id], bi_forest)[0]
    keep = r["flags"] == 0
    return np.asarray(points)[keep], np.nonzero(~keep)[0]


def set_profiling(on):
    _lib.check(_lib.load().eao_iforest_set_profiling(1 if on else 0))


def last_kernel_ms():
    """Device time of k_iforest_build and k_iforest_score of this thread's last call (after set_profiling(True))."""
    ms = (C.c_float * 2)()
    _lib.check(_lib.load().eao_iforest_last_kernel_ms(ms))
    return float(ms[0]), float(ms[1])


def last_stage_us():
    """Inside k_iforest_build, mean over the trees of this thread's last call: (seeding, shuffle and sample, walk) in microseconds."""
    us = (C.c_double * 3)()
    _lib.check(_lib.load().eao_iforest_last_stage_us(us))
    return tuple(float(v) for v in us)
