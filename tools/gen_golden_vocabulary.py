"""Writes tests/golden/vocabulary/k4_l3_n70.npz and score_set.npz: one complete k = 4, L = 3 tree (84 nodes, file ids dealt at random), 70 descriptors (some
repeated, some words stopped) and what the plain-Python restatement tests/vocabulary_reference.py makes of them at every weighting x norm and levelsup 0, 1 and 4;
one query vector, 12 stored vectors and their L1 scores.  Written from the yardstick, never from the code under test.  Data only.

    python tools/gen_golden_vocabulary.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import vocabulary_reference as Y  # noqa: E402
import vocabulary_scenes as SC  # noqa: E402

LEVELSUPS = (0, 1, 4)


def tree_case():
    def weights(rng, n):
        w = rng.uniform(0.01, 10.0, n)
        w[rng.random(n) < 0.1] = 0.0
        w[rng.random(n) < 0.15] = SC.REPEATED_WEIGHT
        return w

    desc, rng = SC.random_tree(SC.complete(4, 3), 4370, weights=weights)
    feats = rng.integers(0, 256, (70, 32), dtype=np.uint8)
    feats[10:17] = feats[10]      # a word seen seven times
    feats[50:56] = feats[3]
    feats = feats[rng.permutation(70)]
    g = dict(parent=desc["parent"], descriptor=desc["descriptor"], weight=desc["weight"], is_leaf=desc["is_leaf"], features=feats, levelsups=np.array(LEVELSUPS, np.int32))
    tree = Y.Tree(desc)
    for levelsup in LEVELSUPS:
        descents = Y.descend_all(tree, feats, levelsup)
        for w in SC.WEIGHTINGS:
            for nm in SC.NORMS:
                r = Y.transform(tree, feats, levelsup, w, nm, descents)
                tag = "_l%d_w%d_n%d" % (levelsup, w, nm)
                g["word_id" + tag], g["word_value" + tag] = r["word_id"], r["word_value"]
        g["node_id_l%d" % levelsup], g["node_start_l%d" % levelsup], g["index_l%d" % levelsup] = r["fv"]["node_id"], r["fv"]["node_start"], r["fv"]["index"]
        g["feat_word_l%d" % levelsup], g["feat_node_l%d" % levelsup], g["feat_stopped_l%d" % levelsup] = r["feat_word"], r["feat_node"], r["feat_stopped"]
    return g


def score_case():
    rng = np.random.default_rng(4371)
    q = SC._vector(rng, 120, vocab=600)
    stored = [SC._vector(rng, int(rng.integers(0, 200)), vocab=600) for _ in range(11)] + [q]
    start = np.zeros(len(stored) + 1, np.int32)
    start[1:] = np.cumsum([len(s[0]) for s in stored])
    return dict(q_id=q[0], q_val=q[1], db_start=start, db_id=np.concatenate([s[0] for s in stored]).astype(np.uint32), db_val=np.concatenate([s[1] for s in stored]),
                scores=np.array([Y.score_l1(q, s) for s in stored], np.float64))


def main():
    out = os.path.join(ROOT, "tests", "golden", "vocabulary")
    os.makedirs(out, exist_ok=True)
    g = tree_case()
    np.savez_compressed(os.path.join(out, "k4_l3_n70.npz"), **g)
    print("k4_l3_n70: nodes", len(g["parent"]), "words", [len(g["word_id_l0_w0_n%d" % n]) for n in SC.NORMS], "fv nodes", [len(g["node_id_l%d" % l]) for l in LEVELSUPS],
          "stopped", int((g["feat_stopped_l0"] & 1).sum()))
    s = score_case()
    np.savez_compressed(os.path.join(out, "score_set.npz"), **s)
    print("score_set: stored", len(s["scores"]), "scores", s["scores"].min(), "..", s["scores"].max())


if __name__ == "__main__":
    main()
