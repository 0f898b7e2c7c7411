"""Object_Map::IsolationForestDeleteOutliers on the device (eao_iforest_scores_batch, eao_object_iforest_outliers_batch; csrc/iforest.hip) against what the
REFERENCE's own include/isolation_forest.h recorded (tests/golden/isolation_forest/*.npz): the Serialize stream byte for byte, the total path lengths replayed
from that stream by the yardstick bit for bit, the scores, the flags."""
import hashlib
import os
import subprocess
import threading

import numpy as np
import pytest

import isolation_forest_reference as Y
import isolation_forest_scenes as SC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "isolation_forest")
SCENES = SC.scenes()


@pytest.fixture(scope="module")
def IF():
    from eao_fusion_amd import isolation_forest
    return isolation_forest


_fix = {}


def fixture(name):
    if name not in _fix:
        z = np.load(os.path.join(GOLD, name + ".npz"))
        _fix[name] = {k: z[k] for k in z.files}
    return _fix[name]


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def host_scores(total, tree_count, sample_size):
    """the host's own libm over the device's totals"""
    return Y.scores_from_totals(total, tree_count, sample_size)


def check_scores(got, want):
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert (np.abs(got[~nan].view(np.int64) - want[~nan].view(np.int64)) <= 1).all()


@pytest.mark.parametrize("name", sorted(SCENES))
def test_scene_against_the_reference(IF, name):
    sc, z = SCENES[name], fixture(name)
    r = IF.scores(sc["points"], sc["tree_count"], sc["seed"], sc["sample_size"], want_stream=True)
    assert len(r["stream"]) == int(z["stream_len"])
    assert hashlib.sha256(r["stream"]).hexdigest().encode() == z["stream_sha256"].tobytes()
    if "stream" in z:
        assert r["stream"] == z["stream"].tobytes()
    want_total = Y.total_path_lengths(sc["points"], Y.parse(r["stream"])[1])
    assert np.array_equal(bits(r["total_path_len"]), bits(want_total))
    check_scores(r["scores"], z["scores"])
    hs = host_scores(r["total_path_len"], sc["tree_count"], sc["sample_size"])
    assert np.array_equal(np.isnan(hs), np.isnan(r["scores"])) and np.array_equal(bits(hs)[~np.isnan(hs)], bits(r["scores"])[~np.isnan(hs)])
    if sc["entry"] == "object":
        o = IF.outliers_batch([sc["points"]], [sc["class_id"]], want_scores=True)[0]
        want = Y.outlier_flags(z["scores"], sc["class_id"])
        assert np.array_equal(o["flags"], want) and o["removed"] == int(want.sum())
        assert np.array_equal(bits(o["scores"]), bits(r["scores"]))


def test_batch_equals_single_calls(IF):
    names = ["gauss_30", "adjacent", "gauss_129", "sample_2", "flat_y", "sample_eq_n", "gauss_300", "all_same"]
    objs = [SCENES[n]["points"] for n in names]
    batch = IF.scores_batch(objs, [SCENES[n]["tree_count"] for n in names], [SCENES[n]["seed"] for n in names], [SCENES[n]["sample_size"] for n in names],
                            want_stream=True)
    for n, b in zip(names, batch):
        z = fixture(n)
        assert b["stream"] == z["stream"].tobytes(), n
        s = IF.scores(SCENES[n]["points"], SCENES[n]["tree_count"], SCENES[n]["seed"], SCENES[n]["sample_size"], want_stream=True)
        assert b["stream"] == s["stream"] and np.array_equal(bits(b["scores"]), bits(s["scores"])) and np.array_equal(bits(b["total_path_len"]), bits(s["total_path_len"]))


def test_batch_across_the_lds_budget(IF):
    """an object in LDS and one through the global workspace in one launch"""
    names = ["gauss_65", "global_path", "lds_edge"]
    batch = IF.scores_batch([SCENES[n]["points"] for n in names], [SCENES[n]["tree_count"] for n in names], [SCENES[n]["seed"] for n in names],
                            [SCENES[n]["sample_size"] for n in names], want_stream=True)
    for n, b in zip(names, batch):
        z = fixture(n)
        assert hashlib.sha256(b["stream"]).hexdigest().encode() == z["stream_sha256"].tobytes(), n
        check_scores(b["scores"], z["scores"])


def test_mixed_batch(IF):
    mixed = SC.mixed_batch()
    with pytest.raises(Exception) as e:      # the object with a NaN: the whole call is refused
        IF.outliers_batch([m[0] for m in mixed], [m[1] for m in mixed])
    assert e.value.status == -1
    mixed = [m for m in mixed if m[2] != "refused"]
    out = IF.outliers_batch([m[0] for m in mixed], [m[1] for m in mixed], want_scores=True)
    for (pts, cls, name), o in zip(mixed, out):
        if name is None:
            assert o["removed"] == 0 and not o["flags"].any() and (o["scores"] == -1.0).all()
        else:
            want = Y.outlier_flags(fixture(name)["scores"], cls)
            assert np.array_equal(o["flags"], want) and o["removed"] == int(want.sum())
            check_scores(o["scores"], fixture(name)["scores"])
    c62 = [o for (p, c, n), o in zip(mixed, out) if n == "class62_60"][0]
    assert c62["removed"] < int(Y.outlier_flags(fixture("class62_60")["scores"], 0).sum())      # th = 0.65f, not 0.6f
    # biForest off: nothing runs, the NaN object included
    mixed = SC.mixed_batch()
    off = IF.outliers_batch([m[0] for m in mixed], [m[1] for m in mixed], bi_forest=False)
    assert all(o["removed"] == 0 and not o["flags"].any() for o in off)
    # a NaN in an object the rules skip is not read
    bad = SC._cloud(40, 7)
    bad[0, 0] = np.nan
    assert IF.outliers_batch([bad], [64])[0]["removed"] == 0


def test_deterministic_across_calls_and_threads(IF):
    names = ["gauss_128", "four_ulps", "dup_pairs"]

    def run():
        return [IF.scores(SCENES[n]["points"], SCENES[n]["tree_count"], SCENES[n]["seed"], SCENES[n]["sample_size"], want_stream=True) for n in names]

    first = run()
    results, errors = [None] * 4, []

    def worker(k):
        try:
            results[k] = run()
        except Exception as ex:      # noqa: BLE001
            errors.append(ex)

    threads = [threading.Thread(target=worker, args=(k,)) for k in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for res in [run()] + results:
        for a, b, n in zip(first, res, names):
            assert a["stream"] == b["stream"] == fixture(n)["stream"].tobytes()
            assert np.array_equal(bits(a["scores"]), bits(b["scores"])) and np.array_equal(bits(a["total_path_len"]), bits(b["total_path_len"]))


def test_n2000_by_hash(IF):
    sc, z = SCENES["n2000"], fixture("n2000")
    assert "stream" not in z
    o = IF.outliers_batch([sc["points"]], [0], want_scores=True)[0]
    check_scores(o["scores"], z["scores"])
    assert np.array_equal(o["flags"], Y.outlier_flags(z["scores"], 0))


def test_short_stream_buffer_is_a_capacity_error(IF):
    from eao_fusion_amd import _lib
    sc, z = SCENES["gauss_31"], fixture("gauss_31")
    with pytest.raises(_lib.EaoError) as e:
        IF.scores_batch([sc["points"]], sc["tree_count"], sc["seed"], sc["sample_size"], want_stream=True, stream_cap=int(z["stream_len"]) - 1)
    assert e.value.status == _lib.EAO_ERR_CAPACITY
    r = IF.scores_batch([sc["points"]], sc["tree_count"], sc["seed"], sc["sample_size"], want_stream=True, stream_cap=int(z["stream_len"]))[0]
    assert r["stream"] == z["stream"].tobytes()


def test_refusals(IF):
    from eao_fusion_amd import _lib
    p = SC._cloud(40, 11)

    def refused(points, tree_count, sample_size):
        with pytest.raises(_lib.EaoError) as e:
            IF.scores(points, tree_count, 1, sample_size)
        return e.value.status == _lib.EAO_ERR_INVALID

    assert refused(p, 50, 0) and refused(p, 50, 41) and refused(p, 0, 20)
    for bad_value in (np.nan, np.inf, -np.inf):
        bad = p.copy()
        bad[39, 2] = bad_value
        assert refused(bad, 50, 20)
    assert refused(np.zeros((65536, 3), np.float32), 1, 2)
    with pytest.raises(_lib.EaoError):
        IF.outliers_batch([np.zeros((65536, 3), np.float32)], [0])
    # the largest accepted size goes through (one tree, a sample of two: the shuffle is all of the work)
    big = np.random.RandomState(5).normal(0, 1, (65535, 3)).astype(np.float32)
    r = IF.scores(big, 1, 3, 2, want_stream=True)
    want_stream, want_scores, _ = Y.forest(big, 1, 3, 2)
    assert r["stream"] == want_stream and np.array_equal(bits(r["scores"]), bits(want_scores))


def test_adapter_over_stand_in_objects(tmp_path):
    """include/eaofusion/ObjectMap.h over the stand-in Object_Map of tests/cpp/object_map, linked against the library itself"""
    exe = str(tmp_path / "object_map_gpu")
    lib_dir = os.path.join(ROOT, "eao_fusion_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "object_map", "object_map_driver.cpp"),
                           "-L", lib_dir, "-leaofusion_hip", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-pthread", "-o", exe])
    import test_object_map_class_cpu as T
    for name in ("gauss_64", "class62_60", "gauss_300"):
        sc = SCENES[name]
        flags = Y.outlier_flags(fixture(name)["scores"], sc["class_id"])
        got = T.run_driver(exe, T.script([(sc["points"], sc["class_id"])], bi_forest=1, batch=False))
        T.check_object(got, sc["points"], flags)
    objs = [(SCENES[n]["points"], SCENES[n]["class_id"]) for n in ("gauss_30", "class62_60", "gauss_129")]
    got = T.run_driver(exe, T.script(objs, bi_forest=1, batch=True))
    per = T.split_objects(got, len(objs))
    for (pts, cls), g, n in zip(objs, per, ("gauss_30", "class62_60", "gauss_129")):
        T.check_object(g, pts, Y.outlier_flags(fixture(n)["scores"], cls))
