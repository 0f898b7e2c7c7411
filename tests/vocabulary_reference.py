"""The yardstick of the vocabulary tests: a literal restatement of DBoW2's tree in plain Python (Python floats are IEEE doubles), one feature at a time, dicts
for the two std::maps.  Written from the reference's lines and citing them (Thirdparty/DBoW2/DBoW2/):

  TemplatedVocabulary.h:1350-1480  the per-node content of both file formats; children in push_back (= ascending id) order; word ids count the leaf-flagged nodes
  TemplatedVocabulary.h:1229-1271  the descent of one feature, nid at level m_L - levelsup
  TemplatedVocabulary.h:1138-1206  transform(features, v, fv, levelsup)
  FORB.cpp:81-101                  distance: 8 x 32-bit popcount of the xor
  BowVector.cpp:34-84              addWeight, addIfNotExist, normalize
  FeatureVector.cpp:31-45          addFeature
  ScoringObject.cpp:23-68          L1Scoring::score

A desc is the dict eao_fusion_amd.vocabulary.Vocabulary takes.  m_L is derived as the largest leaf depth (include/eao_fusion.h says so).  Where upstream leaves nid
uninitialised (a leaf above nid_level, :1163 / :1263) nid is the leaf's id and feat_stopped gets bit 1."""
import math

import numpy as np

TF_IDF, TF, IDF, BINARY = 0, 1, 2, 3      # BowVector.h:36-42
NORM_NONE, NORM_L1, NORM_L2 = 0, 1, 2     # mustNormalize() false / LNorm L1 / L2 (BowVector.h:29-33, ScoringObject.h:74-89)
FORB_L = 32                               # FORB.cpp:26


class Tree:
    """m_nodes as the loaders build it: children lists in ascending id, word ids in id order"""

    def __init__(self, desc):
        self.parent = [0] + [int(p) for p in desc["parent"]]
        n = len(self.parent) - 1
        self.n_nodes = n
        self.descriptor = np.ascontiguousarray(desc["descriptor"], np.uint8).reshape(n, FORB_L)
        self.words32 = self.descriptor.view("<u4").reshape(n, 8) if n else np.zeros((0, 8), np.uint32)
        self.weight = [0.0] + [float(w) for w in desc["weight"]]
        self.children = [[] for _ in range(n + 1)]
        for nid in range(1, n + 1):
            assert 0 <= self.parent[nid] < nid
            self.children[self.parent[nid]].append(nid)      # :1404, :1464
        self.word_id = [None] * (n + 1)
        self.n_words = 0
        for nid in range(1, n + 1):
            if desc["is_leaf"][nid - 1]:                      # :1420-1427, :1468-1473
                assert not self.children[nid]
                self.word_id[nid] = self.n_words
                self.n_words += 1
            else:
                assert self.children[nid]
        level = [0] * (n + 1)
        for nid in range(1, n + 1):
            level[nid] = level[self.parent[nid]] + 1
        self.level = level
        self.depth = max([level[nid] for nid in range(1, n + 1) if not self.children[nid]], default=0)
        self.max_children = max([len(c) for c in self.children], default=0) if n else 0
        self.weighting, self.norm = int(desc["weighting"]), int(desc["norm"])


def distance(a32, b32):
    """FORB::distance (FORB.cpp:81-101) over the 8 words of each descriptor"""
    return sum(bin(int(x) ^ int(y)).count("1") for x, y in zip(a32, b32))


def descend(tree, feature, levelsup, ties=None):
    """:1229-1271.  Returns (word_id, weight, nid, leaf_above_level); ties: a list that receives 1 per level at which the minimum was shared"""
    f32 = np.frombuffer(np.ascontiguousarray(feature, np.uint8).tobytes(), "<u4")
    nid_level = tree.depth - levelsup
    nid = 0 if nid_level <= 0 else None      # :1239
    final_id, current_level = 0, 0
    while True:
        current_level += 1
        nodes = tree.children[final_id]
        final_id = nodes[0]
        best_d = distance(f32, tree.words32[final_id - 1])
        shared = False
        for cid in nodes[1:]:
            d = distance(f32, tree.words32[cid - 1])
            if d < best_d:      # :1256 strict: the first child in id order keeps a tie
                best_d, final_id, shared = d, cid, False
            elif d == best_d:
                shared = True
        if ties is not None and shared:
            ties.append(current_level)
        if current_level == nid_level:      # :1263
            nid = final_id
        if not tree.children[final_id]:      # :1266 isLeaf() = children.empty()
            break
    above = nid is None
    if above:
        nid = final_id
    return tree.word_id[final_id], tree.weight[final_id], nid, above


def descend_all(tree, features, levelsup):
    """the descents of a frame (they do not depend on weighting or norm): what transform(..., descents=) takes"""
    features = np.ascontiguousarray(features, np.uint8).reshape(-1, FORB_L)
    return [descend(tree, f, levelsup) for f in features] if tree.n_nodes > 0 else []


def transform(tree, features, levelsup, weighting=None, norm=None, descents=None):
    """:1138-1206.  Returns dict(word_id, word_value, fv = dict(node_id, node_start, index), feat_word, feat_node, feat_stopped).
    weighting / norm: instead of the tree's own; descents: descend_all(tree, features, levelsup) computed before"""
    features = np.ascontiguousarray(features, np.uint8).reshape(-1, FORB_L)
    n = len(features)
    weighting = tree.weighting if weighting is None else weighting
    norm_type = tree.norm if norm is None else norm
    fw, fn, fs = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint8)
    v, fv = {}, {}
    if tree.n_nodes > 0:      # :1146 empty()
        tf = weighting in (TF, TF_IDF)
        for i in range(n):
            wid, w, nid, above = descents[i] if descents is not None else descend(tree, features[i], levelsup)
            fw[i], fn[i] = wid, nid
            fs[i] = (0 if w > 0 else 1) | (2 if above else 0)
            if w > 0:      # :1169, :1197 not stopped
                if tf:
                    v[wid] = v[wid] + w if wid in v else w      # addWeight, BowVector.cpp:34-46
                elif wid not in v:
                    v[wid] = w                                  # addIfNotExist, :50-58
                fv.setdefault(nid, []).append(i)                # FeatureVector.cpp:31-45
        if tf and v and norm_type == NORM_NONE:      # :1176-1182
            nd = float(len(v))
            for k in v:
                v[k] = v[k] / nd
        if norm_type != NORM_NONE:      # BowVector.cpp:62-84
            norm = 0.0
            if norm_type == NORM_L1:
                for k in sorted(v):
                    norm += math.fabs(v[k])
            else:
                for k in sorted(v):
                    norm += v[k] * v[k]
                norm = math.sqrt(norm)
            if norm > 0.0:
                for k in v:
                    v[k] = v[k] / norm
    wk = sorted(v)
    nk = sorted(fv)
    start = np.zeros(len(nk) + 1, np.int32)
    for j, k in enumerate(nk):
        start[j + 1] = start[j] + len(fv[k])
    return dict(word_id=np.array(wk, np.uint32), word_value=np.array([v[k] for k in wk], np.float64),
                fv=dict(node_id=np.array(nk, np.uint32), node_start=start, index=np.array([i for k in nk for i in fv[k]], np.uint32)),
                feat_word=fw, feat_node=fn, feat_stopped=fs)


def score_l1(v1, v2):
    """L1Scoring::score (ScoringObject.cpp:23-68); v = (ascending word ids, values).  The lower_bound jumps of :47-58 visit the common ids in ascending order."""
    i1, x1 = [int(k) for k in v1[0]], [float(x) for x in v1[1]]
    i2, x2 = [int(k) for k in v2[0]], [float(x) for x in v2[1]]
    a, b, score = 0, 0, 0.0
    while a < len(i1) and b < len(i2):
        if i1[a] == i2[b]:
            vi, wi = x1[a], x2[b]
            score += math.fabs(vi - wi) - math.fabs(vi) - math.fabs(wi)      # :41
            a += 1
            b += 1
        elif i1[a] < i2[b]:
            a += 1
        else:
            b += 1
    return -score / 2.0      # :65
