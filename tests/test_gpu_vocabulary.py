"""ORBVocabulary on the device (eao_vocabulary_*, eao_bow_score_l1; csrc/vocabulary.hip) against the plain-Python yardstick tests/vocabulary_reference.py on the
scenes of tests/vocabulary_scenes.py.  Every comparison is exact: ids and indices with array_equal, the doubles as their 64-bit patterns.  There is no tolerance
anywhere in this file."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest
import torch  # (before the library loads, so that both resolve the same HIP runtime)

import vocabulary_reference as Y
import vocabulary_scenes as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "vocabulary")
KEYS = ("word_id", "word_value", "feat_word", "feat_node", "feat_stopped")
FV_KEYS = ("node_id", "node_start", "index")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def assert_same(dev, ref, what=""):
    for k in KEYS:
        assert dev[k].dtype == ref[k].dtype and np.array_equal(_bits(dev[k]), _bits(ref[k])), "%s %s" % (what, k)
    for k in FV_KEYS:
        assert dev["fv"][k].dtype == ref["fv"][k].dtype and np.array_equal(dev["fv"][k], ref["fv"][k]), "%s fv.%s" % (what, k)


def result_bytes(r):
    return b"".join(np.ascontiguousarray(r[k]).tobytes() for k in KEYS) + b"".join(np.ascontiguousarray(r["fv"][k]).tobytes() for k in FV_KEYS)


_handles = {}


def _voc(name, weighting=Y.TF_IDF, norm=Y.NORM_L1):
    from eao_fusion_amd.vocabulary import Vocabulary
    key = (name, weighting, norm)
    if key not in _handles:
        _handles[key] = Vocabulary(SC.with_modes(SC.scene(name)["desc"], weighting, norm))
    return _handles[key]


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SC.SCENES) + ["orbvoc"])
def test_every_scene_weighting_and_norm(name):
    from eao_fusion_amd.vocabulary import Vocabulary
    sc = SC.scene(name)
    t = sc["tree"]
    for weighting in SC.WEIGHTINGS:
        for norm in SC.NORMS:
            voc = Vocabulary(SC.with_modes(sc["desc"], weighting, norm))
            assert voc.info() == dict(n_nodes=t.n_nodes, n_words=t.n_words, depth=t.depth, max_children=t.max_children)
            for levelsup in sc["levelsups"]:
                assert_same(voc.transform(sc["features"], levelsup), SC.reference(name, levelsup, weighting, norm), "%s w%d n%d l%d" % (name, weighting, norm, levelsup))


@pytest.mark.gpu
@pytest.mark.parametrize("n", SC.FEATURE_COUNTS)
def test_feature_counts(n):
    feats = SC.scene("k10_l3")["features"][:n]
    for weighting, norm in ((Y.TF_IDF, Y.NORM_L1), (Y.TF, Y.NORM_NONE), (Y.BINARY, Y.NORM_L2)):
        assert_same(_voc("k10_l3", weighting, norm).transform(feats, 2), SC.reference("k10_l3", 2, weighting, norm, n=n), "n=%d" % n)


@pytest.mark.gpu
def test_batch_equals_single_calls():
    feats = SC.scene("k10_l3")["features"]
    frames = [feats[:0], feats[:1], feats[100:165], feats, feats[7:10], feats[500:564], feats[:0]]
    for weighting, norm in ((Y.TF_IDF, Y.NORM_L1), (Y.IDF, Y.NORM_NONE)):
        voc = _voc("k10_l3", weighting, norm)
        got = voc.transform_batch(frames, 2)
        assert len(got) == len(frames)
        for f, fr in enumerate(frames):
            assert result_bytes(got[f]) == result_bytes(voc.transform(fr, 2)), "frame %d" % f
    assert _voc("k10_l3").transform_batch([], 2) == []
    # the irregular tree and the empty vocabulary through the batch path
    irr = SC.scene("irregular")["features"]
    got = _voc("irregular").transform_batch([irr[:50], irr[50:]], 1)
    assert_same(got[0], Y.transform(SC.scene("irregular")["tree"], irr[:50], 1), "irregular frame 0")
    assert_same(got[1], Y.transform(SC.scene("irregular")["tree"], irr[50:], 1), "irregular frame 1")
    emp = _voc("empty_vocabulary").transform_batch([feats[:5], feats[:0]], 4)
    assert all(len(e["word_id"]) == 0 and e["fv"]["node_start"].tolist() == [0] for e in emp)


@pytest.mark.gpu
def test_device_resident_descriptors_equal_the_host_call():
    feats = SC.scene("k10_l3")["features"]
    voc = _voc("k10_l3")
    cap = 1200
    block = np.zeros((cap, 32), np.uint8)
    block[:1000] = feats
    block[1000:] = 0xA5      # (rows past the count are never read as features)
    d_desc = torch.from_numpy(block).cuda()
    for n in (1000, 65, 0):
        d_n = torch.tensor([n], dtype=torch.int32).cuda()
        torch.cuda.synchronize()
        for stream in (None, torch.cuda.Stream()):
            got = voc.transform_device(d_desc.data_ptr(), d_n.data_ptr(), cap, 2, None if stream is None else stream.cuda_stream)
            want = voc.transform(feats[:n], 2)
            for k in ("feat_word", "feat_node", "feat_stopped"):
                assert not got[k][n:].any()
                got[k] = got[k][:n]
            assert result_bytes(got) == result_bytes(want)
    # a count outside 0 .. cap fails after the chain and leaves the outputs untouched
    from eao_fusion_amd import _lib, vocabulary as V
    for bad in (cap + 1, -1):
        d_n = torch.tensor([bad], dtype=torch.int32).cuda()
        torch.cuda.synchronize()
        R, keep = V._result(cap)
        for a in keep.values():
            a[...] = 77
        R.n_words, R.n_fv_nodes = -5, -6
        st = _lib.load().eao_vocabulary_transform_device(voc.h, C.c_void_p(d_desc.data_ptr()), C.c_void_p(d_n.data_ptr()), cap, 2, C.byref(R), None)
        assert st == _lib.EAO_ERR_INVALID and (R.n_words, R.n_fv_nodes) == (-5, -6) and all((a == 77).all() for a in keep.values())


@pytest.mark.gpu
def test_two_calls_give_identical_bytes():
    sc = SC.scene("irregular")
    voc = _voc("irregular")
    a = voc.transform(sc["features"], 1)
    _voc("k10_l3").transform(SC.scene("k10_l3")["features"], 0)      # (another size through this thread's scratch in between)
    b = voc.transform(sc["features"], 1)
    assert result_bytes(a) == result_bytes(b)
    sets = SC.score_sets()["n_db_65"]
    from eao_fusion_amd.vocabulary import score_l1
    assert score_l1(*sets).tobytes() == score_l1(*sets).tobytes()


@pytest.mark.gpu
def test_four_host_threads_share_one_handle():
    voc = _voc("k10_l3")
    feats = SC.scene("k10_l3")["features"]
    slices = [feats[:1000], feats[:65], feats[200:700], feats[3:4]]
    want = [result_bytes(voc.transform(s, 2)) for s in slices]
    errors = []

    def work(t):
        try:
            for _ in range(10):
                if result_bytes(voc.transform(slices[t], 2)) != want[t]:
                    errors.append("thread %d differs" % t)
        except Exception as e:      # noqa: BLE001
            errors.append(repr(e))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors


@pytest.mark.gpu
def test_invalid_descs_and_arguments_fail_before_a_launch():
    from eao_fusion_amd import EaoError, _lib, vocabulary as V
    good = SC.scene("one_child")["desc"]

    def broken(**kw):
        d = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in good.items()}
        for k, (i, v) in kw.items():
            if i is None:
                d[k] = v
            else:
                d[k][i] = v
        return d

    internal = int(np.flatnonzero(good["is_leaf"] == 0)[0])
    leaf = int(np.flatnonzero(good["is_leaf"] == 1)[0])
    for d in (broken(parent=(3, 4)), broken(parent=(3, 9)), broken(parent=(0, -1)), broken(is_leaf=(internal, 1)), broken(is_leaf=(leaf, 0)), broken(weighting=(None, 4)),
              broken(weighting=(None, -1)), broken(norm=(None, 3)), broken(norm=(None, -1))):
        with pytest.raises(EaoError) as e:
            V.Vocabulary(d)
        assert e.value.status == _lib.EAO_ERR_INVALID
    L = _lib.load()
    h = C.c_void_p(1234)
    D = _lib.VocabularyDesc(-1, None, None, None, None, 0, 1)
    assert L.eao_vocabulary_create(C.byref(D), C.byref(h)) == _lib.EAO_ERR_INVALID and h.value == 1234
    D = _lib.VocabularyDesc(3, None, None, None, None, 0, 1)
    assert L.eao_vocabulary_create(C.byref(D), C.byref(h)) == _lib.EAO_ERR_INVALID and h.value == 1234
    # transform: outputs untouched
    voc = _voc("k10_l3")
    feats = np.ascontiguousarray(SC.scene("k10_l3")["features"][:20])
    R, keep = V._result(20)

    def untouched(status):
        return status == _lib.EAO_ERR_INVALID and (R.n_words, R.n_fv_nodes) == (-5, -6) and all((a == 77).all() for a in keep.values())

    for a in keep.values():
        a[...] = 77
    R.n_words, R.n_fv_nodes = -5, -6
    assert untouched(L.eao_vocabulary_transform(voc.h, _lib.ptr(feats), 20, -1, C.byref(R)))
    assert untouched(L.eao_vocabulary_transform(voc.h, _lib.ptr(feats), -1, 2, C.byref(R)))
    assert untouched(L.eao_vocabulary_transform(voc.h, None, 20, 2, C.byref(R)))
    assert untouched(L.eao_vocabulary_transform(None, _lib.ptr(feats), 20, 2, C.byref(R)))
    assert untouched(L.eao_vocabulary_transform(voc.h, _lib.ptr(feats), V.MAX_FEATURES + 1, 2, C.byref(R)))
    start = np.array([0, 12, 8, 20], np.int32)
    Rs = (_lib.BowResult * 3)(R, R, R)
    assert L.eao_vocabulary_transform_batch(voc.h, 3, _lib.ptr(feats), _lib.ptr(start), 2, Rs) == _lib.EAO_ERR_INVALID and untouched(_lib.EAO_ERR_INVALID)
    wid = R.word_id
    R.word_id = None
    assert L.eao_vocabulary_transform(voc.h, _lib.ptr(feats), 20, 2, C.byref(R)) == _lib.EAO_ERR_INVALID
    R.word_id = wid
    assert untouched(_lib.EAO_ERR_INVALID)
    # score: ids that do not ascend strictly, db_start that descends
    q = (np.array([1, 5, 9], np.uint32), np.array([0.2, 0.3, 0.5]))
    with pytest.raises(EaoError):
        V.score_l1((np.array([1, 9, 5], np.uint32), q[1]), [q])
    with pytest.raises(EaoError):
        V.score_l1(q, [q, (np.array([4, 4], np.uint32), np.array([0.5, 0.5]))])
    out = np.full(2, 77.0)
    bad_start = np.array([0, 3, 2], np.int32)
    assert L.eao_bow_score_l1(3, _lib.ptr(q[0]), _lib.ptr(q[1]), 2, _lib.ptr(bad_start), _lib.ptr(q[0]), _lib.ptr(q[1]), _lib.ptr(out)) == _lib.EAO_ERR_INVALID
    assert (out == 77.0).all()


@pytest.mark.gpu
def test_supported_maximum_and_one_past_it():
    from eao_fusion_amd import EaoError, _lib, vocabulary as V
    sc = SC.scene("k10_l3")
    n = V.MAX_FEATURES
    feats = np.ascontiguousarray(np.tile(sc["features"], (9, 1))[:n])      # every word is seen 8 or 9 times: c - 1 sequential additions each
    for weighting, norm in ((Y.TF_IDF, Y.NORM_L1), (Y.TF, Y.NORM_L2)):
        key = (2, 1000)
        SC.reference("k10_l3", 2, weighting, norm)      # (fills the store of descents)
        descents = [sc["descents"][key][i % 1000] for i in range(n)]
        assert_same(_voc("k10_l3", weighting, norm).transform(feats, 2), Y.transform(sc["tree"], feats, 2, weighting, norm, descents), "n = 8192")
    with pytest.raises(EaoError) as e:
        _voc("k10_l3").transform(np.zeros((n + 1, 32), np.uint8), 2)
    assert e.value.status == _lib.EAO_ERR_INVALID and str(n) in str(e.value)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SC.score_sets()))
def test_score_l1_bitwise(name):
    from eao_fusion_amd.vocabulary import score_l1
    q, stored = SC.score_sets()[name]
    got = score_l1(q, stored)
    want = np.array([Y.score_l1(q, s) for s in stored], np.float64)
    assert got.shape == want.shape and np.array_equal(got.view(np.uint64), want.view(np.uint64))      # (-0.0 where no word is common)


@pytest.mark.gpu
def test_golden_files():
    from eao_fusion_amd.vocabulary import Vocabulary, score_l1
    z = np.load(os.path.join(GOLDEN, "k4_l3_n70.npz"))
    for weighting in SC.WEIGHTINGS:
        for norm in SC.NORMS:
            voc = Vocabulary(dict(parent=z["parent"], descriptor=z["descriptor"], weight=z["weight"], is_leaf=z["is_leaf"], weighting=weighting, norm=norm))
            for levelsup in z["levelsups"]:
                r = voc.transform(z["features"], int(levelsup))
                tag = "_l%d_w%d_n%d" % (levelsup, weighting, norm)
                want = dict(word_id=z["word_id" + tag], word_value=z["word_value" + tag], feat_word=z["feat_word_l%d" % levelsup], feat_node=z["feat_node_l%d" % levelsup],
                            feat_stopped=z["feat_stopped_l%d" % levelsup],
                            fv=dict(node_id=z["node_id_l%d" % levelsup], node_start=z["node_start_l%d" % levelsup], index=z["index_l%d" % levelsup]))
                assert_same(r, want, tag)
    s = np.load(os.path.join(GOLDEN, "score_set.npz"))
    stored = [(s["db_id"][s["db_start"][j]:s["db_start"][j + 1]], s["db_val"][s["db_start"][j]:s["db_start"][j + 1]]) for j in range(len(s["scores"]))]
    assert np.array_equal(score_l1((s["q_id"], s["q_val"]), stored).view(np.uint64), s["scores"].view(np.uint64))


@pytest.mark.gpu
def test_adapter_from_file_to_search_by_bow(tmp_path):
    """include/eaofusion/ORBVocabulary.h linked with the library: a binary vocabulary file is loaded, both keyframes of a search scene are transformed, and
    eao_kf_search_by_bow over handles created with the adapter's FeatureVectors returns what it returns over the yardstick's."""
    from eao_fusion_amd import search, synth
    from test_vocabulary_class_cpu import _binary
    exe = str(tmp_path / "vocabulary_adapter")
    src = os.path.join(ROOT, "tests", "cpp", "vocabulary", "vocabulary_driver.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-DEAOFUSION_FORCE_CV_COMPAT", "-I", os.path.join(ROOT, "include"), src, "-o", exe,
                           "-L", os.path.join(ROOT, "eao_fusion_amd"), "-leaofusion_hip", "-Wl,-rpath," + os.path.join(ROOT, "eao_fusion_amd"), "-Wl,-rpath,/opt/rocm/lib",
                           "-pthread"])
    d = SC.scene("k10_l3")["desc"]
    d32 = dict(d, weight=d["weight"].astype(np.float32).astype(np.float64))      # what the binary file holds
    (tmp_path / "voc.bin").write_bytes(_binary(d32))
    tree = Y.Tree(d32)
    sc = synth.synth_search_scene(n=300, seed=8300)
    fvs, bows = {}, {}
    for side in ("K1", "K2"):
        feats = sc[side]["descriptors"]
        (tmp_path / (side + ".desc")).write_bytes(np.ascontiguousarray(feats).tobytes())
        out = subprocess.run([exe, "binary", str(tmp_path / "voc.bin"), str(tmp_path / (side + ".desc")), "2"], capture_output=True, text=True)
        assert out.returncode == 0, out.stdout + out.stderr
        lines = out.stdout.strip().split("\n")
        assert lines[0] == "loaded 1 size 1000 empty 0"
        bow = [w.split(":") for w in lines[1].split()[1:]]
        nodes = [w.split(":") for w in lines[2].split()[1:]]
        ref = Y.transform(tree, feats, 2)
        assert [int(k) for k, _ in bow] == ref["word_id"].tolist() and [float(x) for _, x in bow] == ref["word_value"].tolist()
        start = np.cumsum([0] + [len(ix.split(",")) for _, ix in nodes]).astype(np.int32)
        fvs[side] = dict(node_id=np.array([int(k) for k, _ in nodes], np.uint32), node_start=start, index=np.array([int(i) for _, ix in nodes for i in ix.split(",")], np.uint32))
        bows[side] = ref
        # the batch score of the adapter against the yardstick: v against itself, a vector with other words, an empty one
        assert lines[3].split()[0] == "scores" and float(lines[3].split()[1]) == Y.score_l1((ref["word_id"], ref["word_value"]), (ref["word_id"], ref["word_value"]))
    hb = search.product_handles()
    valid1, valid2 = (sc["mp1"] >= 0).astype(np.uint8), (sc["mp2"] >= 0).astype(np.uint8)
    got = hb.search_by_bow_h(1, hb.handle(sc["K1"], fvs["K1"]), valid1, hb.handle(sc["K2"], fvs["K2"]), valid2, 0.75, True)
    ref_fv = {side: bows[side]["fv"] for side in ("K1", "K2")}
    want = hb.search_by_bow_h(1, hb.handle(sc["K1"], ref_fv["K1"]), valid1, hb.handle(sc["K2"], ref_fv["K2"]), valid2, 0.75, True)
    assert got[0] == want[0] and np.array_equal(got[1], want[1]) and got[0] > 0
