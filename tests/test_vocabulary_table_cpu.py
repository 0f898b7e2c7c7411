"""The host half of eao_vocabulary_create without a device: csrc/vocabulary_internal.h (validation and the remap into the table whose siblings are contiguous)
through tools/vocabulary_walk.cpp, a single-threaded walk of that table, built as a stand-alone program with -fsanitize=address,undefined.  On every scene the
walk must reach the yardstick's word, node and flags per feature, and the table's counts must be the yardstick's; descs the library must reject are rejected."""
import os
import subprocess

import numpy as np
import pytest

import vocabulary_scenes as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("vocabulary_walk") / "vocabulary_walk")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tools", "vocabulary_walk.cpp"), "-o", exe])
    return exe


def _blob(d, feats, levelsup):
    return (np.array([len(d["parent"]), len(feats), levelsup], np.int32).tobytes() + np.ascontiguousarray(d["parent"], np.int32).tobytes()
            + np.ascontiguousarray(d["descriptor"], np.uint8).tobytes() + np.ascontiguousarray(d["weight"], np.float64).tobytes()
            + np.ascontiguousarray(d["is_leaf"], np.uint8).tobytes() + np.ascontiguousarray(feats, np.uint8).tobytes())


def _run(walk, tmp_path, d, feats, levelsup):
    (tmp_path / "in.bin").write_bytes(_blob(d, feats, levelsup))
    return subprocess.run([walk, str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), "1"], capture_output=True, text=True, env=ENV)


@pytest.mark.parametrize("name", sorted(set(SC.SCENES) - {"empty_vocabulary"}))
def test_walk_of_the_flattened_table_equals_the_yardstick(walk, tmp_path, name):
    sc = SC.scene(name)
    nf = len(sc["features"])
    for levelsup in sc["levelsups"]:
        out = _run(walk, tmp_path, sc["desc"], sc["features"], levelsup)
        assert out.returncode == 0, out.stderr
        raw = (tmp_path / "out.bin").read_bytes()
        ref = SC.reference(name, levelsup, 0, 1)
        assert np.array_equal(np.frombuffer(raw[:4 * nf], np.uint32), ref["feat_word"]) and np.array_equal(np.frombuffer(raw[4 * nf:8 * nf], np.uint32), ref["feat_node"])
        assert np.array_equal(np.frombuffer(raw[8 * nf:], np.uint8), ref["feat_stopped"])
    t = sc["tree"]
    w = out.stdout.split()
    assert [int(w[w.index(k) + 1]) for k in ("nodes", "words", "depth", "max_children")] == [t.n_nodes, t.n_words, t.depth, t.max_children]


def test_rejected_descs(walk, tmp_path):
    good = SC.scene("one_child")["desc"]
    feats = SC.scene("one_child")["features"][:2]
    internal, leaf = int(np.flatnonzero(good["is_leaf"] == 0)[0]), int(np.flatnonzero(good["is_leaf"] == 1)[0])
    for key, i, v in (("parent", 3, 4), ("parent", 3, 9), ("parent", 0, -1), ("is_leaf", internal, 1), ("is_leaf", leaf, 0)):
        d = dict(good, **{key: good[key].copy()})
        d[key][i] = v
        out = _run(walk, tmp_path, d, feats, 0)
        assert out.returncode == 4 and out.stderr.strip(), (key, i, v)
