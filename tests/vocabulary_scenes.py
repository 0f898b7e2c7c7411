"""Seeded scenes of the vocabulary tests (tests/test_vocabulary_reference_cpu.py holds each to the branch it claims, tests/test_gpu_vocabulary.py runs them on the
device).  A scene is dict(desc = the dict eao_fusion_amd.vocabulary.Vocabulary takes -- weighting TF_IDF and norm L1, ORB-SLAM2's, unless a test overrides them --,
features (n,32) u8, levelsups).  Trees have at most ~1.2 k nodes but for `orbvoc`; file ids are dealt so that the children of a node are NOT contiguous."""
import numpy as np

import vocabulary_reference as Y

WEIGHTINGS = (Y.TF_IDF, Y.TF, Y.IDF, Y.BINARY)
NORMS = (Y.NORM_NONE, Y.NORM_L1, Y.NORM_L2)
FEATURE_COUNTS = (0, 1, 3, 4, 5, 63, 64, 65, 1000)


def _desc(parent, descriptor, weight, is_leaf, weighting=Y.TF_IDF, norm=Y.NORM_L1):
    return dict(parent=np.asarray(parent, np.int32), descriptor=np.ascontiguousarray(descriptor, np.uint8).reshape(-1, 32), weight=np.asarray(weight, np.float64),
                is_leaf=np.asarray(is_leaf, np.uint8), weighting=weighting, norm=norm)


def from_shape(kids, rng, order="random"):
    """kids: dict structural node -> number of children, structural node 0 the root, children created on the fly.  Returns (parent, is_leaf, struct_of_id): file ids
    dealt in a random order that keeps parent < child (order='random'), or depth first (order='dfs')."""
    children = {}
    count = [1]

    def grow(s, depth):
        k = kids(s, depth)
        children[s] = list(range(count[0], count[0] + k))
        count[0] += k
        for c in children[s]:
            grow(c, depth + 1)

    grow(0, 0)
    n = count[0] - 1
    ids = {0: 0}
    if order == "dfs":
        stack = list(reversed(children[0]))
        while stack:
            s = stack.pop()
            ids[s] = len(ids)
            stack.extend(reversed(children[s]))
    else:
        ready = list(children[0])
        while ready:
            s = ready.pop(int(rng.integers(len(ready))))
            ids[s] = len(ids)
            ready.extend(children[s])
    parent, leaf = np.zeros(n, np.int32), np.zeros(n, np.uint8)
    for s, cs in children.items():
        for c in cs:
            parent[ids[c] - 1] = ids[s]
        if s:
            leaf[ids[s] - 1] = 0 if cs else 1
    return parent, leaf


def random_tree(kids, seed, order="random", weights=None):
    rng = np.random.default_rng(seed)
    parent, leaf = from_shape(kids, rng, order)
    n = len(parent)
    w = rng.uniform(0.01, 10.0, n) if weights is None else weights(rng, n)
    return _desc(parent, rng.integers(0, 256, (n, 32), dtype=np.uint8), w, leaf), rng


def complete(k, L):
    return lambda s, depth: k if depth < L else 0


def _features(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def k10_l3(n=1000, seed=11):
    """complete k = 10, L = 3, random descriptors: ties among siblings occur by themselves"""
    desc, rng = random_tree(complete(10, 3), seed, order="dfs")
    return dict(desc=desc, features=_features(rng, n), levelsups=(0, 2, 3, 4, 5))


def irregular(seed=12):
    """1 .. 20 children per node, leaves at depths 1 .. 5"""
    rng0 = np.random.default_rng(seed)

    def kids(s, depth):
        if depth == 0:
            return 7
        if depth >= 5 or (depth >= 1 and rng0.random() < 0.35 + 0.12 * depth):
            return 0
        return int(rng0.integers(1, 21)) if depth < 3 else int(rng0.integers(1, 6))

    desc, rng = random_tree(kids, seed + 100)
    return dict(desc=desc, features=_features(rng, 300), levelsups=(0, 1, 4, 5, 7))


def one_child(seed=13):
    """a chain: nodes with exactly one child, also directly under the root's first child"""
    shape = {0: 2, 1: 1, 2: 3, 3: 1, 7: 2}      # structural ids in creation (depth-first) order; everything else is a leaf

    desc, rng = random_tree(lambda s, depth: shape.get(s, 0), seed)
    return dict(desc=desc, features=_features(rng, 40), levelsups=(0, 1, 2, 4, 6))


def wide(k, seed):
    """complete k = 17 / 20, L = 2: more children than a 16-lane group"""
    desc, rng = random_tree(complete(k, 2), seed)
    # features near the LAST children of the root, so that the winner lies in the second chunk of lanes
    feats = _features(rng, 120)
    root_kids = np.flatnonzero(desc["parent"] == 0)
    for i in range(60):
        feats[i] = desc["descriptor"][root_kids[-1 - (i % 4)]]
        feats[i, i % 32] ^= 1 << (i % 8)
    return dict(desc=desc, features=feats, levelsups=(0, 1, 2, 4))


def duplicated_siblings(seed=16):
    """every sibling set holds each descriptor twice and the features are those descriptors: distance 0 twice, the first in id order must win"""
    desc, rng = random_tree(complete(6, 3), seed)
    par = desc["parent"]
    for p in range(len(par) + 1):
        sib = np.flatnonzero(par == p)
        for j in range(1, len(sib), 2):
            desc["descriptor"][sib[j]] = desc["descriptor"][sib[j - 1]]
    leaves = np.flatnonzero(desc["is_leaf"])
    feats = desc["descriptor"][rng.choice(leaves, 90)].copy()
    return dict(desc=desc, features=feats, levelsups=(0, 1, 3))


def _stop_weights(rng, n):
    w = rng.uniform(0.01, 10.0, n)
    kind = rng.integers(0, 6, n)
    w[kind == 0] = 0.0
    w[kind == 1] = -rng.uniform(0.01, 10.0, int((kind == 1).sum()))
    w[kind == 2] = -0.0
    return w


def stopped_words(seed=17):
    """zero, minus zero and negative weights: stopped words"""
    desc, rng = random_tree(complete(5, 3), seed, weights=_stop_weights)
    return dict(desc=desc, features=_features(rng, 200), levelsups=(0, 1, 4))


def all_stopped(seed=18):
    """every weight zero: both vectors come back empty"""
    desc, rng = random_tree(complete(4, 2), seed, weights=lambda rng, n: np.zeros(n))
    return dict(desc=desc, features=_features(rng, 33), levelsups=(0, 2))


REPEATED_WEIGHT = 0.1      # ((((0.1 + 0.1) + 0.1) + 0.1) + 0.1) + 0.1 = 0.6 but 6 * 0.1 = 0.6000000000000001


def repeated_word(seed=19):
    """one descriptor 6, 7 and 9 times: a word whose value is c - 1 sequential additions, which is not c * w"""
    desc, rng = random_tree(complete(4, 3), seed, weights=lambda rng, n: np.where(rng.random(n) < 0.5, REPEATED_WEIGHT, rng.uniform(0.01, 10.0, n)))
    feats = _features(rng, 60)
    for first, c in ((3, 6), (20, 7), (40, 9)):
        feats[first:first + c] = feats[first]
    feats = feats[rng.permutation(60)]      # (the copies are not adjacent in feature order)
    return dict(desc=desc, features=feats, levelsups=(0, 3))


def empty_vocabulary():
    return dict(desc=_desc(np.zeros(0, np.int32), np.zeros((0, 32), np.uint8), np.zeros(0), np.zeros(0, np.uint8)),
                features=_features(np.random.default_rng(20), 17), levelsups=(0, 4))


def orbvoc(n=300, seed=21, k=10, L=6):
    """the shape of ORBvoc: complete k = 10, L = 6, 1,111,110 nodes in breadth-first file order, random bytes (generated in memory, nothing committed)"""
    rng = np.random.default_rng(seed)
    N = (k ** (L + 1) - 1) // (k - 1) - 1
    ids = np.arange(1, N + 1, dtype=np.int64)
    parent = ((ids - 1) // k).astype(np.int32)
    leaf = (ids > N - k ** L).astype(np.uint8)
    desc = _desc(parent, rng.integers(0, 256, (N, 32), dtype=np.uint8), rng.uniform(0.01, 10.0, N), leaf)
    return dict(desc=desc, features=_features(rng, n), levelsups=(4,))


SCENES = {
    "k10_l3": k10_l3, "irregular": irregular, "one_child": one_child, "k17": lambda: wide(17, 14), "k20": lambda: wide(20, 15),
    "duplicated_siblings": duplicated_siblings, "stopped_words": stopped_words, "all_stopped": all_stopped, "repeated_word": repeated_word,
    "empty_vocabulary": empty_vocabulary,
}

_cache = {}


def scene(name):
    """the scene, its yardstick tree and a store of its descents, built once per process and left unchanged"""
    if name not in _cache:
        sc = orbvoc() if name == "orbvoc" else SCENES[name]()
        _cache[name] = dict(sc, tree=Y.Tree(sc["desc"]), descents={})
    return _cache[name]


def reference(name, levelsup, weighting, norm, n=None):
    """the yardstick's transform of the scene's first n features (None: all)"""
    sc = scene(name)
    feats = sc["features"] if n is None else sc["features"][:n]
    key = (levelsup, len(feats))
    if key not in sc["descents"]:
        sc["descents"][key] = Y.descend_all(sc["tree"], feats, levelsup)
    return Y.transform(sc["tree"], feats, levelsup, weighting, norm, sc["descents"][key])


def with_modes(desc, weighting, norm):
    return dict(desc, weighting=weighting, norm=norm)


# ---- score sets: (query, [stored vectors]); a vector is (ascending word ids u32, values f64)
def _vector(rng, n_words, vocab=5000, normalised=True):
    ids = np.sort(rng.choice(vocab, n_words, replace=False)).astype(np.uint32)
    v = rng.uniform(0.01, 10.0, n_words)
    if normalised and n_words:
        v = v / np.abs(v).sum()
    return ids, v


def score_sets(seed=30):
    rng = np.random.default_rng(seed)
    q = _vector(rng, 300)
    empty = (np.zeros(0, np.uint32), np.zeros(0, np.float64))
    disjoint = ((q[0][:50] + 100000).astype(np.uint32), _vector(rng, 50)[1])
    one_common = (np.sort(np.concatenate([[q[0][137]], 200000 + np.arange(20)])).astype(np.uint32), _vector(rng, 21)[1])
    many = [_vector(rng, int(rng.integers(1, 400)), vocab=900) for _ in range(61)]      # (the query's ids are below 5000: common words are plentiful)
    return {
        "n_db_0": (q, []),
        "n_db_1": (q, [_vector(rng, 250, vocab=900)]),
        "n_db_65": (q, many + [q, empty, disjoint, one_common]),
        "identical": (q, [q]),
        "disjoint": (q, [disjoint]),
        "empty_vector": (q, [empty]),
        "empty_query": (empty, [q, empty]),
        "one_common_word": (q, [one_common]),
    }
