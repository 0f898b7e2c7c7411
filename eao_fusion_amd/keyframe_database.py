"""KeyFrameDatabase (reference src/KeyFrameDatabase.cc): the recognition database resident on the device through eao_keyframe_db_* (csrc/keyframe_db.hip,
csrc/keyframe_db_internal.h).

A BowVector is (word_id u32 ascending, word_value f64).  intersect() is the kernel's raw result; query_scores() is stage 1 (DetectLoopCandidates /
DetectRelocalizationCandidates up to lScoreAndMatch), candidates() stage 2 over the callers' GetBestCovisibilityKeyFrames(10) lists; detect_loop_candidates() and
detect_relocalization_candidates() chain the two with a callable that names a keyframe's neighbours."""
import ctypes as C

import numpy as np

from . import _lib

LOOP, RELOCALIZATION = 0, 1
N_NEIGHBOURS = 10      # GetBestCovisibilityKeyFrames(10), src/KeyFrameDatabase.cc:150, :264


def _vec(v):
    return np.ascontiguousarray(v[0], np.uint32).reshape(-1), np.ascontiguousarray(v[1], np.float64).reshape(-1)


class KeyFrameDatabase:
    def __init__(self, n_words):
        self.h = C.c_void_p()
        self._lib = _lib.load()
        _lib.check(self._lib.eao_keyframe_db_create(int(n_words), C.byref(self.h)))

    def add(self, kf_id, bow):
        wi, wv = _vec(bow)
        assert len(wi) == len(wv)
        _lib.check(self._lib.eao_keyframe_db_add(self.h, int(kf_id), len(wi), _lib.ptr(wi), _lib.ptr(wv)))

    def erase(self, kf_id):
        _lib.check(self._lib.eao_keyframe_db_erase(self.h, int(kf_id)))

    def clear(self):
        _lib.check(self._lib.eao_keyframe_db_clear(self.h))

    def info(self):
        """dict(n_live, n_stored_words, arena_capacity) (eao_keyframe_db_info)"""
        n, w, c = C.c_int32(0), C.c_int64(0), C.c_int64(0)
        _lib.check(self._lib.eao_keyframe_db_info(self.h, C.byref(n), C.byref(w), C.byref(c)))
        return dict(n_live=int(n.value), n_stored_words=int(w.value), arena_capacity=int(c.value))

    def intersect(self, query):
        """dict(kf_id u64, common i32, first_word u32, score f64) over the live keyframes in storage order (eao_keyframe_db_intersect)"""
        qi, qv = _vec(query)
        cap = self.info()["n_live"]
        m = max(cap, 1)
        ids, common, first, score = np.zeros(m, np.uint64), np.zeros(m, np.int32), np.zeros(m, np.uint32), np.zeros(m, np.float64)
        n = C.c_int32(0)
        _lib.check(self._lib.eao_keyframe_db_intersect(self.h, len(qi), _lib.ptr(qi), _lib.ptr(qv), cap, _lib.ptr(ids), _lib.ptr(common), _lib.ptr(first),
                                                       _lib.ptr(score), C.byref(n)))
        n = int(n.value)
        return dict(kf_id=ids[:n].copy(), common=common[:n].copy(), first_word=first[:n].copy(), score=score[:n].copy())

    def query_scores(self, kind, query_id, query, connected=(), min_score=0.0):
        """Stage 1.  dict(sharing_id, sharing_words, max_common_words, min_common_words, n_scores, scored_id, scored_score f32)"""
        qi, qv = _vec(query)
        conn = np.ascontiguousarray(list(connected), np.uint64).reshape(-1)
        cap = self.info()["n_live"]
        m = max(cap, 1)
        keep = dict(sharing_id=np.zeros(m, np.uint64), sharing_words=np.zeros(m, np.int32), scored_id=np.zeros(m, np.uint64), scored_score=np.zeros(m, np.float32))
        Q = _lib.KeyFrameDbQuery(int(kind), int(query_id), len(qi), _lib.ptr(qi), _lib.ptr(qv), len(conn), _lib.ptr(conn), float(min_score))
        R = _lib.KeyFrameDbScored()
        for k, a in keep.items():
            setattr(R, k, _lib.ptr(a))
        _lib.check(self._lib.eao_keyframe_db_query_scores(self.h, C.byref(Q), cap, C.byref(R)))
        ns, nc = int(R.n_sharing), int(R.n_scored)
        return dict(sharing_id=keep["sharing_id"][:ns].copy(), sharing_words=keep["sharing_words"][:ns].copy(), max_common_words=int(R.max_common_words),
                    min_common_words=int(R.min_common_words), n_scores=int(R.n_scores), scored_id=keep["scored_id"][:nc].copy(),
                    scored_score=keep["scored_score"][:nc].copy())

    def candidates(self, kind, query_id, scored, neighbours, min_score=0.0):
        """Stage 2.  scored: the dict of query_scores; neighbours: per scored keyframe, the ids of GetBestCovisibilityKeyFrames(10).
        dict(cand_id u64, acc_score f32, best_id u64, used_unset)"""
        sid, ssc = np.ascontiguousarray(scored["scored_id"], np.uint64), np.ascontiguousarray(scored["scored_score"], np.float32)
        n = len(sid)
        assert len(neighbours) == n
        start = np.zeros(n + 1, np.int32)
        start[1:] = np.cumsum([len(nb) for nb in neighbours])
        nb = np.ascontiguousarray([i for l in neighbours for i in l], np.uint64).reshape(-1)
        m = max(n, 1)
        cand, acc, best = np.zeros(m, np.uint64), np.zeros(m, np.float32), np.zeros(m, np.uint64)
        nc, unset = C.c_int32(0), C.c_int32(0)
        _lib.check(self._lib.eao_keyframe_db_candidates(self.h, int(kind), int(query_id), int(scored["min_common_words"]), float(min_score), n, _lib.ptr(sid),
                                                        _lib.ptr(ssc), _lib.ptr(start), _lib.ptr(nb), _lib.ptr(cand), C.byref(nc), _lib.ptr(acc), _lib.ptr(best),
                                                        C.byref(unset)))
        return dict(cand_id=cand[:int(nc.value)].copy(), acc_score=acc[:n].copy(), best_id=best[:n].copy(), used_unset=int(unset.value))

    def detect_loop_candidates(self, query_id, query, connected, min_score, neighbours_of):
        """DetectLoopCandidates(pKF, minScore); neighbours_of(id) -> the ids of that keyframe's GetBestCovisibilityKeyFrames(10)"""
        s = self.query_scores(LOOP, query_id, query, connected, min_score)
        return self.candidates(LOOP, query_id, s, [list(neighbours_of(int(i)))[:N_NEIGHBOURS] for i in s["scored_id"]], min_score)["cand_id"]

    def detect_relocalization_candidates(self, query_id, query, neighbours_of):
        """DetectRelocalizationCandidates(F)"""
        s = self.query_scores(RELOCALIZATION, query_id, query)
        return self.candidates(RELOCALIZATION, query_id, s, [list(neighbours_of(int(i)))[:N_NEIGHBOURS] for i in s["scored_id"]])["cand_id"]

    def __del__(self):
        try:
            if self.h:
                self._lib.eao_keyframe_db_destroy(self.h)
                self.h = None
        except Exception:
            pass
