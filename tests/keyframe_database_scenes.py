"""Seeded scenes of the KeyFrameDatabase tests.  A scene is dict(n_words, ops, neighbours, claim, check): ops is a sequence of
    ("add", id, bow) | ("erase", id) | ("clear",) | ("query", kind, query_id, bow, connected_ids, min_score)
with bow = (ascending uint32 word ids, float64 values); neighbours(id) names GetBestCovisibilityKeyFrames(10) of a keyframe; claim says which branch of
src/KeyFrameDatabase.cc the scene is there to reach and check(results) is True when the yardstick reached it (tests/test_keyframe_database_reference_cpu.py).
reference(name) runs the ops through tests/keyframe_database_reference.py once and returns, per query, dict(raw = the intersection before the query, res = the
yardstick's lists, counts, scores and candidates).

maxCommonWords * 0.8f against * 0.8: the issue asks for the counts at which the float product truncates differently from the double one.  There is none: an
exhaustive search over 1 .. 8192 (the cap of a vector, hence of a count) finds int(float32(m) * float32(0.8)) == int(m * 0.8) everywhere.  0.8f exceeds 0.8 by a
relative 1.5e-8, below half an ulp of float32 (3e-8 .. 6e-8), so at every multiple of 5 the float product rounds to the integer the double gives, and elsewhere
the fraction is .2 / .4 / .6 / .8.  float_truncation_differs() is that search; the scene `truncation_boundary` holds the boundary itself (a count equal to
minCommonWords is not scored, one above is) at multiples of 5 and next to them."""
import functools

import numpy as np

import keyframe_database_reference as Y

LOOP, RELOC = Y.LOOP, Y.RELOC


def float_truncation_differs(limit=8192):
    return [m for m in range(1, limit + 1) if int(np.float32(m) * np.float32(0.8)) != int(m * 0.8)]


def vec(rs, ids):
    """a BowVector over the given word ids: positive values, L1-normalised as ORBvoc's are"""
    ids = np.unique(np.asarray(ids, np.uint32))
    v = rs.uniform(0.2, 1.0, len(ids))
    return ids, (v / v.sum() if len(ids) else v).astype(np.float64)


def words(rs, n_words, n, avoid=()):
    pool = np.setdiff1d(np.arange(n_words, dtype=np.int64), np.asarray(list(avoid), np.int64))
    return rs.choice(pool, n, replace=False)


def similar(rs, n_words, base_ids, keep, extra):
    """keep of the base's words and extra others"""
    base_ids = np.asarray(base_ids, np.int64)
    return vec(rs, np.concatenate([rs.choice(base_ids, keep, replace=False), words(rs, n_words, extra, avoid=base_ids)]))


def chain(ids, reach=5):
    """neighbours(id): the up to ten keyframes next to it in the given order, nearest first"""
    pos = {k: i for i, k in enumerate(ids)}

    def nb(k):
        out = []
        for d in range(1, reach + 1):
            for j in (pos[k] - d, pos[k] + d):
                if 0 <= j < len(ids):
                    out.append(ids[j])
        return out
    return nb


def q(kind, qid, bow, connected=(), min_score=0.0):
    return ("query", kind, qid, bow, tuple(connected), float(min_score))


def both(qid, bow, connected=(), min_score=0.0):
    return [q(LOOP, qid, bow, connected, min_score), q(RELOC, qid, bow)]


SCENES = {}


def scene(fn):
    SCENES[fn.__name__] = fn
    return fn


@scene
def no_keyframe():
    rs = np.random.RandomState(1)
    return dict(n_words=100, ops=both(3, vec(rs, words(rs, 100, 20))), neighbours=lambda k: [], claim=":106 / :223 on an empty database",
                check=lambda R: all(len(r["raw"]) == 0 and not r["res"]["sharing_id"] for r in R))


@scene
def one_keyframe():
    rs = np.random.RandomState(2)
    base = words(rs, 200, 30)
    return dict(n_words=200, ops=[("add", 1, similar(rs, 200, base, 20, 5))] + both(3, vec(rs, base)), neighbours=lambda k: [],
                claim="one keyframe is listed, scored and returned", check=lambda R: all(r["res"]["cand_id"] == [1] for r in R))


@scene
def empty_query():
    rs = np.random.RandomState(3)
    ops = [("add", i, vec(rs, words(rs, 100, 10))) for i in (1, 2, 3)] + both(9, (np.zeros(0, np.uint32), np.zeros(0)))
    return dict(n_words=100, ops=ops, neighbours=chain([1, 2, 3]), claim="an empty mBowVec walks no list; every raw score is -0.0",
                check=lambda R: all(not r["res"]["sharing_id"] and all(c == 0 and s == 0.0 and np.signbit(s) for _, c, _, s in r["raw"]) for r in R))


@scene
def no_sharing():
    rs = np.random.RandomState(4)
    ops = [("add", i, vec(rs, rs.choice(np.arange(0, 150), 20, replace=False))) for i in (1, 2, 3, 4)] + both(9, vec(rs, rs.choice(np.arange(150, 300), 20, replace=False)))
    return dict(n_words=300, ops=ops, neighbours=chain([1, 2, 3, 4]), claim=":106 / :223 with keyframes that hold none of the query's words",
                check=lambda R: all(len(r["raw"]) == 4 and not r["res"]["sharing_id"] for r in R))


@scene
def every_sharer_connected():
    rs = np.random.RandomState(5)
    base = words(rs, 300, 40)
    ids = [1, 2, 3, 4, 5]
    ops = [("add", i, similar(rs, 300, base, 25, 10)) for i in ids]
    ops += [q(LOOP, 7, vec(rs, base), connected=ids + [77], min_score=0.01), q(LOOP, 8, vec(rs, base), connected=[2, 4], min_score=0.01), q(RELOC, 8, vec(rs, base))]
    return dict(n_words=300, ops=ops, neighbours=chain(ids), claim=":95 keeps every connected keyframe off the list (their count ends at 1); the next query lists the others",
                check=lambda R: not R[0]["res"]["sharing_id"] and all(c > 0 for _, c, _, _ in R[0]["raw"]) and sorted(R[1]["res"]["sharing_id"]) == [1, 3, 5])


@scene
def all_scores_below_min_score():
    rs = np.random.RandomState(6)
    base = words(rs, 300, 40)
    ids = [1, 2, 3, 4]
    ops = [("add", i, similar(rs, 300, base, 30, 10)) for i in ids] + [q(LOOP, 7, vec(rs, base), min_score=2.0)]
    return dict(n_words=300, ops=ops, neighbours=chain(ids), claim=":135 rejects every score, :140 returns", check=lambda R: R[0]["res"]["n_scores"] > 0 and not R[0]["res"]["scored_id"])


@scene
def first_word_ties():
    rs = np.random.RandomState(7)
    ids = [9, 3, 7, 1, 8, 2]
    qv = vec(rs, [10, 20, 30, 40, 50, 60, 70, 80])
    held = {9: [20, 30, 90], 3: [10, 20, 91], 7: [20, 40, 50, 92], 1: [10, 93], 8: [5, 20, 30, 40], 2: [30, 94]}
    ops = [("add", i, vec(rs, held[i])) for i in ids] + both(11, qv)
    return dict(n_words=100, ops=ops, neighbours=chain(ids), claim="several keyframes enter at the same word: list order is push_back order inside the word's list, not id order",
                check=lambda R: all(r["res"]["sharing_id"] == [3, 1, 9, 7, 8, 2] for r in R))


@scene
def erase_then_readd():
    rs = np.random.RandomState(8)
    base = words(rs, 300, 30)
    v = {i: vec(rs, np.concatenate([base[:1], words(rs, 300, 12, avoid=base)])) for i in (1, 2, 3)}      # all three enter at the same word
    qv = vec(rs, base)
    ops = [("add", i, v[i]) for i in (1, 2, 3)] + both(5, qv) + [("erase", 1), ("erase", 44), ("add", 1, v[1])] + both(6, qv)
    return dict(n_words=300, ops=ops, neighbours=chain([1, 2, 3]), claim="a re-added keyframe goes to the back of every list; erasing an unknown id changes nothing",
                check=lambda R: R[0]["res"]["sharing_id"] == [1, 2, 3] and R[2]["res"]["sharing_id"] == [2, 3, 1])


@scene
def added_empty_vector():
    rs = np.random.RandomState(9)
    base = words(rs, 200, 30)
    ops = [("add", 1, similar(rs, 200, base, 20, 5)), ("add", 2, (np.zeros(0, np.uint32), np.zeros(0))), ("add", 3, similar(rs, 200, base, 20, 5))] + both(5, vec(rs, base))
    return dict(n_words=200, ops=ops, neighbours=chain([1, 2, 3]), claim="a keyframe without words is in no list",
                check=lambda R: all(len(r["raw"]) == 3 and sorted(r["res"]["sharing_id"]) == [1, 3] for r in R))


def _stored(n):
    def make():
        rs = np.random.RandomState(20 + n)
        base = words(rs, 400, 40)
        ids = list(range(1, n + 1))
        ops = [("add", i, similar(rs, 400, base, int(rs.randint(20, 36)), 8)) for i in ids] + both(50, vec(rs, base), connected=[2], min_score=0.05)
        return dict(n_words=400, ops=ops, neighbours=chain(ids), claim="%d stored vectors: the last workgroup of four wavefronts is partly / exactly / just over full" % n,
                    check=lambda R: len(R[0]["raw"]) == n and len(R[1]["res"]["sharing_id"]) == n)
    make.__name__ = "stored_%d" % n
    return scene(make)


for _n in (3, 4, 5):
    _stored(_n)


@scene
def stored_lengths_63_64_65_200():
    rs = np.random.RandomState(30)
    base = words(rs, 3000, 220)
    ids = [1, 2, 3, 4]
    ops = [("add", i, similar(rs, 3000, base, n - 7, 7)) for i, n in zip(ids, (63, 64, 65, 200))] + both(50, vec(rs, base), min_score=0.01)
    return dict(n_words=3000, ops=ops, neighbours=chain(ids), claim="stored vectors of one chunk less one, one chunk, one chunk and one, several chunks",
                check=lambda R: [c for _, c, _, _ in R[0]["raw"]] == [56, 57, 58, 193])


@scene
def common_63_64_65():
    rs = np.random.RandomState(31)
    base = words(rs, 3000, 150)
    ids = [1, 2, 3]
    ops = [("add", i, similar(rs, 3000, base, n, 90)) for i, n in zip(ids, (63, 64, 65))] + both(50, vec(rs, base), min_score=0.01)
    return dict(n_words=3000, ops=ops, neighbours=chain(ids), claim="63, 64 and 65 common words spread over more than one chunk of the stored vector",
                check=lambda R: [c for _, c, _, _ in R[0]["raw"]] == [63, 64, 65])


@scene
def truncation_boundary():
    # maxCommonWords m and a second keyframe with exactly int(m * 0.8f) resp. one more common words: the first is not scored (:128 is a strict >), the second is
    rs = np.random.RandomState(32)
    ops, want = [], []
    qid, kid = 100, 1
    for m in (5, 10, 11, 14, 15, 64, 65, 125):
        base = words(rs, 5000, m + 5)
        t = int(np.float32(m) * np.float32(0.8))
        ops.append(("clear",))
        for keep in (m, t, t + 1):
            ops.append(("add", kid, similar(rs, 5000, base, keep, 3)))
            kid += 1
        ops += both(qid, vec(rs, base))
        want += [(m, t)] * 2
        qid += 1
    return dict(n_words=5000, ops=ops, neighbours=lambda k: [], claim=":119 / :234 minCommonWords = int(maxCommonWords * 0.8f) and the strict > of :128 / :245",
                check=lambda R: all((r["res"]["max_common_words"], r["res"]["min_common_words"]) == w and r["res"]["n_scores"] == 2
                                    and len(r["res"]["sharing_id"]) == 3 for r, w in zip(R, want)))


def _reloc_pair(second_query):
    rs = np.random.RandomState(33)
    base = words(rs, 2000, 60)
    other = words(rs, 2000, 60, avoid=base)
    # X shares 50 words with the first query and 2 with the second; A shares 40 with the second and has X as a neighbour
    x = vec(rs, np.concatenate([base[:50], other[:2], words(rs, 2000, 5, avoid=np.concatenate([base, other]))]))
    a = vec(rs, np.concatenate([other[5:45], words(rs, 2000, 5, avoid=np.concatenate([base, other]))]))
    ops = [("add", 1, x), ("add", 2, a)]
    if second_query:
        ops += [q(RELOC, 7, vec(rs, base))]
    ops += [q(RELOC, 8, vec(rs, other))]
    return ops


@scene
def reloc_stale_score():
    def check(R):
        first, second = R[0]["res"], R[1]["res"]
        stale = first["scored_score"][first["scored_id"].index(1)]
        return (1 in second["sharing_id"] and second["scored_id"] == [2] and second["used_unset"] == 0
                and second["acc_score"][0] == np.float32(second["scored_score"][0] + stale))
    return dict(n_words=2000, ops=_reloc_pair(True), neighbours=lambda k: [1] if k == 2 else [2], claim=":272 tests mnRelocQuery alone: a neighbour at or below minCommonWords adds the score an EARLIER query left",
                check=check)


@scene
def reloc_unset_score():
    return dict(n_words=2000, ops=_reloc_pair(False), neighbours=lambda k: [1] if k == 2 else [2], claim=":275 reads mRelocScore of a keyframe that was never scored (uninitialised upstream)",
                check=lambda R: R[0]["res"]["scored_id"] == [2] and R[0]["res"]["used_unset"] == 1 and R[0]["res"]["acc_score"][0] == R[0]["res"]["scored_score"][0])


@scene
def query_id_0():
    rs = np.random.RandomState(34)
    base = words(rs, 300, 40)
    ids = [1, 2, 3]
    ops = [("add", i, similar(rs, 300, base, 30, 5)) for i in ids] + both(0, vec(rs, base)) + both(0, vec(rs, base)) + both(4, vec(rs, base))
    return dict(n_words=300, ops=ops, neighbours=chain(ids), claim="mnLoopQuery / mnRelocQuery start at 0: query id 0 lists nothing (:92 / :213 are false) and only counts",
                check=lambda R: all(not r["res"]["sharing_id"] for r in R[:4]) and all(len(r["res"]["sharing_id"]) == 3 for r in R[4:]))


@scene
def repeated_query_id():
    rs = np.random.RandomState(35)
    base = words(rs, 300, 40)
    ids = [1, 2, 3, 4]
    ops = [("add", i, similar(rs, 300, base, 30, 5)) for i in ids[:3]] + both(5, vec(rs, base)) + [("add", 4, similar(rs, 300, base, 30, 5))] + both(5, vec(rs, base), min_score=0.01)
    ops += both(6, vec(rs, base))
    # after the repeat, keyframes 1 .. 3 carry the counts of both queries: as neighbours of 4 they pass :158 with the FIRST query's score
    return dict(n_words=300, ops=ops, neighbours=chain(ids), claim="a query id equal to the stored one lists nothing new and adds its count on top (:101, :219)",
                check=lambda R: R[2]["res"]["sharing_id"] == [4] and R[3]["res"]["sharing_id"] == [4] and len(R[4]["res"]["sharing_id"]) == 4 and len(R[2]["res"]["acc_score"]) == 1
                and R[2]["res"]["acc_score"][0] > R[2]["res"]["scored_score"][0])


@scene
def best_keyframe_named_twice():
    rs = np.random.RandomState(36)
    base = words(rs, 1000, 60)
    qv = vec(rs, base)
    strong = (qv[0].copy(), qv[1].copy())      # the query itself: score 1
    ops = [("add", 1, similar(rs, 1000, base, 50, 10)), ("add", 2, strong), ("add", 3, similar(rs, 1000, base, 50, 10)), ("add", 4, similar(rs, 1000, base, 49, 30))]
    ops += both(9, qv, min_score=0.01)
    nb = {1: [2], 2: [], 3: [2, 1], 4: []}
    return dict(n_words=1000, ops=ops, neighbours=lambda k: nb[k], claim=":186 / :299 spAlreadyAddedKF: two scored entries name the same best keyframe, returned once in first-seen order",
                check=lambda R: all(r["res"]["best_id"].count(2) == 3 and r["res"]["cand_id"].count(2) == 1 and len(r["res"]["cand_id"]) < len(r["res"]["best_id"]) for r in R))


def _places(seed, n_kf, n_words, per_kf, n_places, place_words, n_queries, erase_every=0):
    """keyframes around `places` (word pools), so that a query shares many words with a few keyframes and a few with many; ids are added out of order"""
    rs = np.random.RandomState(seed)
    skew = rs.zipf(1.3, n_words * 2)
    skew = np.unique(skew[skew < n_words])      # a skewed set of frequent words every vector draws from
    pools = [np.unique(rs.randint(0, n_words, place_words)) for _ in range(n_places)]
    ids = [int(i) for i in rs.permutation(n_kf) + 1]

    def draw(place):
        k = int(per_kf * rs.uniform(0.55, 0.75))
        return vec(rs, np.concatenate([rs.choice(pools[place], k, replace=False), rs.randint(0, n_words, per_kf - k), skew[rs.randint(0, len(skew), 6)]]))
    place_of = {k: (i * n_places) // n_kf for i, k in enumerate(ids)}
    ops = [("add", k, draw(place_of[k])) for k in ids]
    for j in range(n_queries):
        place = int(rs.randint(n_places))
        near = [k for k in ids if place_of[k] == place]
        if erase_every and j % erase_every == 1:
            gone = near[:max(1, len(near) // 2)] + [ids[j]]
            ops += [("erase", k) for k in gone]
            back = gone[0]
            ops.append(("add", back, draw(place_of[back])))
        ops += both(1000 + j // 2, draw(place), connected=near[:3], min_score=0.02)      # (every query id is used by two queries in a row)
    return dict(n_words=n_words, ops=ops, neighbours=chain(ids))


@scene
def k300_w100():
    s = _places(40, 300, 2000, 100, 12, 150, 6, erase_every=2)
    s.update(claim="300 keyframes x about 100 words over 2000: long lists, erasures, repeated query ids",
             check=lambda R: max(len(r["res"]["sharing_id"]) for r in R) > 250 and any(len(r["res"]["cand_id"]) > 1 for r in R))
    return s


@scene
def k2000_w800():
    s = _places(41, 2000, 1000000, 800, 40, 1200, 1)
    s.update(claim="2000 keyframes x about 800 words over 10^6 word ids", check=lambda R: len(R[0]["raw"]) == 2000 and len(R[0]["res"]["sharing_id"]) > 500 and R[0]["res"]["cand_id"])
    return s


SMALL = [n for n in SCENES if n != "k2000_w800"]


@functools.lru_cache(maxsize=None)
def get(name):
    return SCENES[name]()


def run(sc, db):
    """the ops through a yardstick Database; per query dict(op, raw, res)"""
    out = []
    last = None      # (the bow whose intersection is at hand: nothing was added or erased since)
    for op in sc["ops"]:
        if op[0] != "query":
            last = None
        if op[0] == "add":
            db.add(Y.KeyFrame(op[1], op[2]))
        elif op[0] == "erase":
            db.erase(op[1])
        elif op[0] == "clear":
            db.clear()
        else:
            _, kind, qid, bow, connected, min_score = op
            raw = last[1] if last is not None and last[0] is bow else db.intersect(bow)
            last = (bow, raw)
            res = db.detect_loop_candidates(qid, bow, connected, min_score, sc["neighbours"]) if kind == LOOP else db.detect_relocalization_candidates(qid, bow, sc["neighbours"])
            out.append(dict(op=op, raw=raw, res=res))
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    sc = get(name)
    return run(sc, Y.Database(sc["n_words"]))
