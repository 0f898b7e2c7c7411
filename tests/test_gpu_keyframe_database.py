"""KeyFrameDatabase on the device (eao_keyframe_db_*; csrc/keyframe_db.hip, csrc/keyframe_db_internal.h) against the plain-Python yardstick
tests/keyframe_database_reference.py on the scenes of tests/keyframe_database_scenes.py.  Every comparison is exact: ids, counts and orders with array_equal, the
double scores as their 64-bit and the float scores as their 32-bit patterns.  There is no tolerance anywhere in this file."""
import ctypes as C
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch  # noqa: F401  (before the library loads, so that both resolve the same HIP runtime)

import keyframe_database_reference as Y
import keyframe_database_scenes as SC
import vocabulary_reference as VY

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "keyframe_database")
sys.path.insert(0, os.path.join(ROOT, "tools"))


def replay(sc, db=None):
    """the scene's ops through a device database; per query dict(raw, s1, s2)"""
    from eao_fusion_amd.keyframe_database import KeyFrameDatabase
    db = db or KeyFrameDatabase(sc["n_words"])
    out = []
    for op in sc["ops"]:
        if op[0] == "add":
            db.add(op[1], op[2])
        elif op[0] == "erase":
            db.erase(op[1])
        elif op[0] == "clear":
            db.clear()
        else:
            _, kind, qid, bow, connected, min_score = op
            raw = db.intersect(bow)
            s1 = db.query_scores(kind, qid, bow, connected, min_score)
            s2 = db.candidates(kind, qid, s1, [list(sc["neighbours"](int(i)))[:Y.N_NEIGHBOURS] for i in s1["scored_id"]], min_score)
            out.append(dict(raw=raw, s1=s1, s2=s2))
    return out


def assert_raw(got, want, what):
    ids, common, first, score = [np.array([t[k] for t in want], d) for k, d in enumerate((np.uint64, np.int32, np.uint32, np.float64))]
    assert np.array_equal(got["kf_id"], ids), what + " storage order"
    assert np.array_equal(got["common"], common), what + " common"
    assert np.array_equal(got["first_word"][common > 0], first[common > 0]), what + " first_word"      # (unspecified where common == 0)
    assert np.array_equal(got["score"].view(np.uint64), score.view(np.uint64)), what + " score"


def assert_query(got, want, what):
    s1, s2 = got["s1"], got["s2"]
    assert s1["sharing_id"].tolist() == list(want["sharing_id"]) and s1["sharing_words"].tolist() == list(want["sharing_words"]), what + " lKFsSharingWords"
    assert (s1["max_common_words"], s1["min_common_words"], s1["n_scores"]) == (want["max_common_words"], want["min_common_words"], want["n_scores"]), what + " counts"
    assert s1["scored_id"].tolist() == list(want["scored_id"]), what + " lScoreAndMatch ids"
    assert np.array_equal(s1["scored_score"].view(np.uint32), np.array(want["scored_score"], np.float32).view(np.uint32)), what + " lScoreAndMatch scores"
    assert np.array_equal(s2["acc_score"].view(np.uint32), np.array(want["acc_score"], np.float32).view(np.uint32)), what + " accScore"
    assert s2["best_id"].tolist() == list(want["best_id"]), what + " pBestKF"
    assert s2["cand_id"].tolist() == list(want["cand_id"]), what + " candidates"
    assert s2["used_unset"] == want["used_unset"], what + " used_unset"


def assert_scene(got, want, name):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert_raw(g["raw"], w["raw"], "%s query %d" % (name, k))
        assert_query(g, w["res"], "%s query %d" % (name, k))


def blob(results):
    return b"".join(np.ascontiguousarray(a).tobytes() for r in results for part in ("raw", "s1", "s2") for k, a in sorted(r[part].items()) if isinstance(a, np.ndarray))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SC.SCENES))
def test_every_scene_raw_intersection_and_both_stages(name):
    assert_scene(replay(SC.get(name)), SC.reference(name), name)


@pytest.mark.gpu
def test_arena_growth_and_compaction():
    from eao_fusion_amd.keyframe_database import KeyFrameDatabase
    sc = SC.get("k300_w100")
    adds = [op for op in sc["ops"] if op[0] == "add"][:300]
    bow = next(op for op in sc["ops"] if op[0] == "query")[3]
    db = KeyFrameDatabase(sc["n_words"])
    db.add(*adds[0][1:])
    first_capacity = db.info()["arena_capacity"]
    one = db.intersect(bow)
    words = len(adds[0][2][0])
    for op in adds[1:]:
        db.add(op[1], op[2])
        words += len(op[2][0])
    info = db.info()
    assert info == dict(n_live=300, n_stored_words=words, arena_capacity=info["arena_capacity"]) and info["arena_capacity"] > first_capacity >= len(adds[0][2][0])
    before = db.intersect(bow)
    assert all(np.array_equal(before[k][:1], one[k]) for k in one)      # the first vector survived every reallocation
    y = Y.Database(sc["n_words"])
    for op in adds:
        y.add(Y.KeyFrame(op[1], op[2]))
    assert_raw(before, y.intersect(bow), "grown")
    # erase two of every three: the dead words pass half of the words in use on the way, the live ones are moved together
    gone = [op[1] for i, op in enumerate(adds) if i % 3 != 1]
    for k in gone:
        db.erase(k)
        y.erase(k)
    after = db.intersect(bow)
    keep = ~np.isin(before["kf_id"], np.array(gone, np.uint64))
    live_words = sum(len(op[2][0]) for i, op in enumerate(adds) if i % 3 == 1)
    # n_stored_words counts the dead words too until they are compacted away: without compaction it would still be `words`
    assert db.info()["n_live"] == 100 and live_words <= db.info()["n_stored_words"] <= 2 * live_words < words
    assert all(np.array_equal(after[k].view(np.uint8), before[k][keep].view(np.uint8)) for k in before)
    assert_raw(after, y.intersect(bow), "compacted")
    db.add(*adds[0][1:])      # and the arena goes on behind the compacted words
    y.add(Y.KeyFrame(*adds[0][1:]))
    assert_raw(db.intersect(bow), y.intersect(bow), "after compaction")


@pytest.mark.gpu
def test_resident_scores_equal_uploaded_scores():
    from eao_fusion_amd.keyframe_database import KeyFrameDatabase
    from eao_fusion_amd.vocabulary import score_l1
    sc = SC.get("k300_w100")
    adds = [op for op in sc["ops"] if op[0] == "add"][:300]
    db = KeyFrameDatabase(sc["n_words"])
    for op in adds:
        db.add(op[1], op[2])
    for q in [op[3] for op in sc["ops"] if op[0] == "query"][:4] + [(np.zeros(0, np.uint32), np.zeros(0))]:
        assert np.array_equal(db.intersect(q)["score"].view(np.uint64), score_l1(q, [op[2] for op in adds]).view(np.uint64))


@pytest.mark.gpu
def test_same_calls_same_bytes_and_host_threads():
    from eao_fusion_amd.keyframe_database import KeyFrameDatabase
    names = ["k300_w100", "repeated_query_id", "first_word_ties", "stored_lengths_63_64_65_200"]
    sequential = [blob(replay(SC.get(n))) for n in names]
    assert [blob(replay(SC.get(n))) for n in names] == sequential
    got, errors = [None] * 4, []

    def work(i):
        try:
            got[i] = blob(replay(SC.get(names[i])))
        except Exception as e:      # noqa: BLE001
            errors.append(e)
    threads = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors and got == sequential      # four handles, four threads
    # four threads on ONE handle: intersect is pure
    sc = SC.get("k300_w100")
    db = KeyFrameDatabase(sc["n_words"])
    for op in [op for op in sc["ops"] if op[0] == "add"][:300]:
        db.add(op[1], op[2])
    bow = next(op for op in sc["ops"] if op[0] == "query")[3]
    want = b"".join(a.tobytes() for _, a in sorted(db.intersect(bow).items()))
    shared = [None] * 4

    def ask(i):
        try:
            for _ in range(5):
                shared[i] = b"".join(a.tobytes() for _, a in sorted(db.intersect(bow).items()))
        except Exception as e:      # noqa: BLE001
            errors.append(e)
    threads = [threading.Thread(target=ask, args=(i,)) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors and shared == [want] * 4


@pytest.mark.gpu
def test_invalid_arguments_leave_outputs_and_state_untouched():
    from eao_fusion_amd import _lib
    from eao_fusion_amd.keyframe_database import KeyFrameDatabase
    L = _lib.load()
    sc = SC.get("repeated_query_id")
    ops, want = sc["ops"], SC.reference("repeated_query_id")
    n_before = sum(op[0] == "query" for op in ops[:6])
    db = KeyFrameDatabase(sc["n_words"])
    head = replay(dict(sc, ops=ops[:6]), db)      # three adds, a loop and a relocalisation query, a fourth add
    INV = _lib.EAO_ERR_INVALID
    u32, f64, u64 = (lambda *a: np.array(a, np.uint32)), (lambda *a: np.array(a, np.float64)), (lambda *a: np.array(a, np.uint64))
    p = _lib.ptr

    def add(k, ids, vals=None):
        ids = np.ascontiguousarray(ids, np.uint32)
        vals = np.full(len(ids), 0.5) if vals is None else vals
        return L.eao_keyframe_db_add(db.h, k, len(ids), p(ids), p(vals))
    info = db.info()
    assert add(1, u32(1, 2)) == INV                                  # an id that is live
    assert add(50, u32(5, 5)) == INV and add(50, u32(6, 5)) == INV   # ids that do not ascend strictly
    assert add(50, u32(1, sc["n_words"])) == INV                     # a word id at n_words
    assert add(50, np.arange(8193, dtype=np.uint32)) == INV          # more words than EAO_VOCABULARY_MAX_FEATURES
    two = u32(1, 2)
    assert L.eao_keyframe_db_add(db.h, 50, 2, p(two), None) == INV and L.eao_keyframe_db_add(db.h, 50, -1, None, None) == INV
    assert db.info() == info
    # intersect: a bad query or a short cap writes nothing
    out = dict(ids=np.full(8, 77, np.uint64), common=np.full(8, 77, np.int32), first=np.full(8, 77, np.uint32), score=np.full(8, 77.0))
    n = C.c_int32(-5)

    def intersect(ids, vals, cap):
        return L.eao_keyframe_db_intersect(db.h, len(ids), p(ids), p(vals), cap, p(out["ids"]), p(out["common"]), p(out["first"]), p(out["score"]), C.byref(n))
    long, long_vals = np.arange(8193, dtype=np.uint32), np.zeros(8193)
    assert intersect(u32(3, 3), f64(0.5, 0.5), 8) == INV and intersect(u32(4, 3), f64(0.5, 0.5), 8) == INV and intersect(u32(sc["n_words"]), f64(1.0), 8) == INV
    assert intersect(u32(1, 2), f64(0.5, 0.5), 3) == INV             # cap below the four live keyframes
    assert L.eao_keyframe_db_intersect(db.h, 8193, p(long), p(long_vals), 8, p(out["ids"]), p(out["common"]), p(out["first"]), p(out["score"]), C.byref(n)) == INV
    assert n.value == -5 and all((a == 77).all() for a in out.values())
    # query_scores: the same, and the per-keyframe state stays (the valid queries below show it)
    keep = dict(sharing_id=np.full(8, 77, np.uint64), sharing_words=np.full(8, 77, np.int32), scored_id=np.full(8, 77, np.uint64), scored_score=np.full(8, 77, np.float32))
    R = _lib.KeyFrameDbScored()
    for k, a in keep.items():
        setattr(R, k, p(a))
    R.n_sharing = R.n_scored = R.n_scores = R.max_common_words = R.min_common_words = -5
    qi, qv = ops[6][3]

    def scores(kind, ids, vals, cap, qid=5):
        Q = _lib.KeyFrameDbQuery(kind, qid, len(ids), p(ids), p(vals), 0, None, 0.0)
        return L.eao_keyframe_db_query_scores(db.h, C.byref(Q), cap, C.byref(R))
    assert scores(2, qi, qv, 8) == INV and scores(-1, qi, qv, 8) == INV      # a kind that is neither
    assert scores(1, qi, qv, 3, qid=6) == INV                               # a short cap, with a query id that would list everything
    assert scores(0, u32(9, 9), f64(0.5, 0.5), 8, qid=6) == INV
    Q = _lib.KeyFrameDbQuery(0, 6, len(qi), p(qi), p(qv), 2, None, 0.0)      # connected ids announced, none given
    assert L.eao_keyframe_db_query_scores(db.h, C.byref(Q), 8, C.byref(R)) == INV
    assert (R.n_sharing, R.n_scored, R.n_scores, R.max_common_words, R.min_common_words) == (-5,) * 5 and all((a == 77).all() for a in keep.values())
    # candidates: a kind out of range, a CSR that does not start at 0 or descends
    cand, nc, unset = np.full(4, 77, np.uint64), C.c_int32(-5), C.c_int32(-5)

    sid, ssc, nbs = u64(1, 2), np.array([0.5, 0.5], np.float32), u64(2, 1, 3)

    def candidates(kind, start):
        start = np.array(start, np.int32)
        return L.eao_keyframe_db_candidates(db.h, kind, 5, 1, 0.0, 2, p(sid), p(ssc), p(start), p(nbs), p(cand), C.byref(nc), None, None, C.byref(unset))
    assert candidates(3, [0, 1, 2]) == INV and candidates(0, [1, 1, 2]) == INV and candidates(1, [0, 2, 1]) == INV
    assert (nc.value, unset.value) == (-5, -5) and (cand == 77).all()
    # the rest of the scene: a repeated query id and a new one, as if none of the above had been called
    tail = replay(dict(sc, ops=ops[6:]), db)
    assert_scene(head + tail, want, "repeated_query_id around invalid calls")
    assert len(head) == n_before


@pytest.mark.gpu
def test_golden_files():
    import gen_golden_keyframe_database as G
    for name in G.NAMES:
        sc, want = G.unpack(np.load(os.path.join(GOLDEN, name + ".npz")))
        assert_scene(replay(sc), want, "golden " + name)


@pytest.mark.gpu
def test_chain_from_vocabulary_file_to_relocalisation_candidates(tmp_path):
    """include/eaofusion/ORBVocabulary.h and KeyFrameDatabase.h linked with the library: a binary vocabulary file is loaded, the descriptors of ten stand-in
    keyframes and one frame go through ORBVocabulary::transform into KeyFrameDatabase::add and DetectRelocalizationCandidates / DetectLoopCandidates, and the
    keyframes returned are the yardstick's over the yardstick's BowVectors."""
    import vocabulary_scenes as VSC
    from test_vocabulary_class_cpu import _binary
    exe = str(tmp_path / "keyframe_database_chain")
    src = os.path.join(ROOT, "tests", "cpp", "keyframe_database", "keyframe_database_driver.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-DKFDB_CHAIN", "-DEAOFUSION_FORCE_CV_COMPAT", "-I", os.path.join(ROOT, "include"), src, "-o", exe,
                           "-L", os.path.join(ROOT, "eao_fusion_amd"), "-leaofusion_hip", "-Wl,-rpath," + os.path.join(ROOT, "eao_fusion_amd"), "-Wl,-rpath,/opt/rocm/lib",
                           "-pthread"])
    d = VSC.scene("k10_l3")["desc"]
    d32 = dict(d, weight=d["weight"].astype(np.float32).astype(np.float64))      # what the binary file holds
    (tmp_path / "voc.bin").write_bytes(_binary(d32))
    tree = VY.Tree(d32)
    feats = VSC.scene("k10_l3")["features"]
    rs = np.random.RandomState(5)
    n = 10
    # keyframe i sees a window of the scene's features; the frame sees what keyframes 3 .. 5 see
    sets = [feats[np.sort(rs.choice(np.arange(60 * i, 60 * i + 300), 150, replace=False))] for i in range(n)] + [feats[np.sort(rs.choice(np.arange(200, 520), 150, replace=False))]]
    files = []
    for i, s in enumerate(sets):
        files.append(str(tmp_path / ("f%d.desc" % i)))
        open(files[-1], "wb").write(np.ascontiguousarray(s).tobytes())
    out = subprocess.run([exe, "chain", str(tmp_path / "voc.bin"), "2"] + files, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().split("\n")
    bows = [VY.transform(tree, s, 2) for s in sets]
    bows = [(b["word_id"], b["word_value"]) for b in bows]
    assert lines[0] == "words " + " ".join(str(len(b[0])) for b in bows)
    y = Y.Database(tree.n_words)
    for i in range(n):
        y.add(Y.KeyFrame(i, bows[i]))
    nb = lambda k: [j for j in (k - 1, k + 1) if 0 <= j < n]      # noqa: E731
    reloc = y.detect_relocalization_candidates(77, bows[n], nb)
    assert lines[1] == "reloc" + "".join(" %d" % c for c in reloc["cand_id"]) and reloc["cand_id"]
    loop = y.detect_loop_candidates(n - 1, bows[n - 1], [n - 2], 0.01, nb)
    assert lines[2] == "loop" + "".join(" %d" % c for c in loop["cand_id"])
