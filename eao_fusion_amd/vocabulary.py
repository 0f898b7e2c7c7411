"""ORBVocabulary (reference include/ORBVocabulary.h, Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h): the DBoW2 tree on the device through eao_vocabulary_* and
eao_bow_score_l1 (csrc/vocabulary.hip).

desc: dict(parent (n,) i32, descriptor (n,32) u8, weight (n,) f64, is_leaf (n,) u8, weighting 0..3 (TF_IDF, TF, IDF, BINARY), norm 0..2 (none, L1, L2)); entry i
is node id i + 1 in file order, parent 0 is the root.
A transform returns dict(word_id (u32), word_value (f64) -- the BowVector in std::map order --, fv = dict(node_id, node_start, index) -- the FeatureVector in the
layout the guided searches take --, feat_word, feat_node, feat_stopped per feature)."""
import ctypes as C

import numpy as np

from . import _lib

TF_IDF, TF, IDF, BINARY = 0, 1, 2, 3
NORM_NONE, NORM_L1, NORM_L2 = 0, 1, 2
MAX_FEATURES = 8192      # EAO_VOCABULARY_MAX_FEATURES


def _result(cap):
    m = max(cap, 1)
    keep = dict(word_id=np.zeros(m, np.uint32), word_value=np.zeros(m, np.float64), node_id=np.zeros(m, np.uint32), node_start=np.zeros(m + 1, np.int32),
                index=np.zeros(m, np.uint32), feat_word=np.zeros(m, np.uint32), feat_node=np.zeros(m, np.uint32), feat_stopped=np.zeros(m, np.uint8))
    R = _lib.BowResult()
    _fill(R, keep)
    return R, keep


def _fill(R, keep):
    for k, a in keep.items():
        setattr(R, k, _lib.ptr(a))


def _out(R, keep, n):
    nw, nn = int(R.n_words), int(R.n_fv_nodes)
    start = keep["node_start"][:nn + 1].copy()
    return dict(word_id=keep["word_id"][:nw].copy(), word_value=keep["word_value"][:nw].copy(),
                fv=dict(node_id=keep["node_id"][:nn].copy(), node_start=start, index=keep["index"][:int(start[nn])].copy()),
                feat_word=keep["feat_word"][:n].copy(), feat_node=keep["feat_node"][:n].copy(), feat_stopped=keep["feat_stopped"][:n].copy())


class Vocabulary:
    def __init__(self, desc):
        keep = dict(parent=np.ascontiguousarray(desc["parent"], np.int32).reshape(-1), descriptor=np.ascontiguousarray(desc["descriptor"], np.uint8).reshape(-1, 32),
                    weight=np.ascontiguousarray(desc["weight"], np.float64).reshape(-1), is_leaf=np.ascontiguousarray(desc["is_leaf"], np.uint8).reshape(-1))
        n = len(keep["parent"])
        assert len(keep["descriptor"]) == n and len(keep["weight"]) == n and len(keep["is_leaf"]) == n
        D = _lib.VocabularyDesc(n, _lib.ptr(keep["parent"]), _lib.ptr(keep["descriptor"]), _lib.ptr(keep["weight"]), _lib.ptr(keep["is_leaf"]),
                                int(desc["weighting"]), int(desc["norm"]))
        self.h = C.c_void_p()
        self._lib = _lib.load()
        _lib.check(self._lib.eao_vocabulary_create(C.byref(D), C.byref(self.h)))

    def info(self):
        """dict(n_nodes, n_words, depth, max_children) (eao_vocabulary_info)"""
        v = [C.c_int32(0) for _ in range(4)]
        _lib.check(self._lib.eao_vocabulary_info(self.h, *[C.byref(x) for x in v]))
        return dict(zip(("n_nodes", "n_words", "depth", "max_children"), [int(x.value) for x in v]))

    def transform(self, descriptors, levelsup):
        d = np.ascontiguousarray(descriptors, np.uint8).reshape(-1, 32)
        n = len(d)
        R, keep = _result(n)
        _lib.check(self._lib.eao_vocabulary_transform(self.h, _lib.ptr(d), n, int(levelsup), C.byref(R)))
        return _out(R, keep, n)

    def transform_batch(self, frames, levelsup):
        """frames: a list of (n_f, 32) descriptor arrays; one upload, one launch chain, one copy back (eao_vocabulary_transform_batch)."""
        ds = [np.ascontiguousarray(f, np.uint8).reshape(-1, 32) for f in frames]
        nf = len(ds)
        start = np.zeros(nf + 1, np.int32)
        start[1:] = np.cumsum([len(d) for d in ds])
        cat = np.ascontiguousarray(np.concatenate(ds)) if nf else np.zeros((0, 32), np.uint8)
        Rs = (_lib.BowResult * max(nf, 1))()
        keeps = []
        for f in range(nf):
            _, keep = _result(len(ds[f]))
            _fill(Rs[f], keep)
            keeps.append(keep)
        _lib.check(self._lib.eao_vocabulary_transform_batch(self.h, nf, _lib.ptr(cat), _lib.ptr(start), int(levelsup), Rs))
        return [_out(Rs[f], keeps[f], len(ds[f])) for f in range(nf)]

    def transform_device(self, d_desc_ptr, d_n_ptr, cap, levelsup, stream=None):
        """Over descriptors and a count resident in HBM (addresses, e.g. torch tensors' data_ptr()); eao_vocabulary_transform_device."""
        R, keep = _result(cap)
        _lib.check(self._lib.eao_vocabulary_transform_device(self.h, C.c_void_p(d_desc_ptr), C.c_void_p(d_n_ptr), int(cap), int(levelsup), C.byref(R),
                                                             C.c_void_p(stream) if stream else None))
        return _out(R, keep, cap)      # (feat_*: cap entries, those past the device-resident count stay zero)

    def __del__(self):
        try:
            if self.h:
                self._lib.eao_vocabulary_destroy(self.h)
                self.h = None
        except Exception:
            pass


def score_l1(query, stored):
    """L1Scoring::score of one BowVector (word_id, word_value) against a list of them (eao_bow_score_l1); float64 per stored vector."""
    qi, qv = np.ascontiguousarray(query[0], np.uint32), np.ascontiguousarray(query[1], np.float64)
    nd = len(stored)
    start = np.zeros(nd + 1, np.int32)
    start[1:] = np.cumsum([len(s[0]) for s in stored])
    di = np.ascontiguousarray(np.concatenate([np.asarray(s[0], np.uint32) for s in stored])) if nd else np.zeros(0, np.uint32)
    dv = np.ascontiguousarray(np.concatenate([np.asarray(s[1], np.float64) for s in stored])) if nd else np.zeros(0, np.float64)
    out = np.zeros(max(nd, 1), np.float64)
    _lib.check(_lib.load().eao_bow_score_l1(len(qi), _lib.ptr(qi), _lib.ptr(qv), nd, _lib.ptr(start), _lib.ptr(di), _lib.ptr(dv), _lib.ptr(out)))
    return out[:nd].copy()
