"""The class surface include/eaofusion/ORBVocabulary.h without a device: compiled with g++ against the stand-ins of tests/cpp/vocabulary/vocabulary_driver.cpp and
linked with tests/cpp/vocabulary/vocabulary_stub.cpp, which prints every library call and answers by a made-up rule.  Checked: both loaders on files this test
writes (a trailing newline and a blank line, a leaf as the last node, rejected headers, a truncated record, a node the library rejects) hand eao_vocabulary_create
the flattened arrays of the file and stop at the end of the data; the two maps are rebuilt from the library's answer; scoreBatch packs query and stored vectors;
the host score is the yardstick's."""
import os
import struct
import subprocess

import numpy as np
import pytest

import vocabulary_reference as Y
import vocabulary_scenes as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("vocabulary") / "vocabulary_surface")
    src = os.path.join(ROOT, "tests", "cpp", "vocabulary")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-DEAOFUSION_FORCE_CV_COMPAT", "-I", os.path.join(ROOT, "include"),
                           os.path.join(src, "vocabulary_driver.cpp"), os.path.join(src, "vocabulary_stub.cpp"), "-o", exe])
    return exe


def _tree():
    d = SC.one_child()["desc"]
    assert d["is_leaf"][-1] == 1      # the last node of the file is a leaf: upstream's binary loader would count it twice
    return d


def _text(d, header="10 6 0 0", tail="\n"):
    rows = [header]
    for i in range(len(d["parent"])):
        rows.append("%d %d %s %r" % (d["parent"][i], d["is_leaf"][i], " ".join(str(int(b)) for b in d["descriptor"][i]), float(d["weight"][i])))
    return "\n".join(rows) + tail


def _binary(d, size_node=41, scoring=0, weighting=0, drop=0):
    n = len(d["parent"])
    blob = struct.pack("<IIiiii", n + 1, size_node, 10, 6, scoring, weighting)
    for i in range(n):
        blob += struct.pack("<I", int(d["parent"][i])) + d["descriptor"][i].tobytes() + struct.pack("<f", float(d["weight"][i])) + struct.pack("<B", int(d["is_leaf"][i]))
    return blob[:len(blob) - drop]


def _run(driver, kind, path):
    out = subprocess.run([driver, kind, path], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout.strip().split("\n")


def _created(line):
    w = line.split()
    assert w[0] == "create"
    n = int(w[2])
    at = {k: w.index(k) for k in ("parent", "leaf", "weight", "desc")}
    return dict(n=n, weighting=int(w[4]), norm=int(w[6]), parent=np.array(w[at["parent"] + 1:at["leaf"]], np.int32), leaf=np.array(w[at["leaf"] + 1:at["weight"]], np.uint8),
                weight=np.array(w[at["weight"] + 1:at["desc"]], np.float64), desc=np.array(w[at["desc"] + 1:], np.uint8).reshape(n, 32))


def _same_arrays(c, d, weight):
    assert c["n"] == len(d["parent"]) and np.array_equal(c["parent"], d["parent"]) and np.array_equal(c["leaf"], d["is_leaf"])
    assert np.array_equal(c["desc"], d["descriptor"]) and np.array_equal(c["weight"].view(np.uint64), np.asarray(weight, np.float64).view(np.uint64))


@pytest.mark.parametrize("tail", ["", "\n", "\n\n  \n"])
def test_text_loader_stops_at_the_end_of_the_data(driver, tmp_path, tail):
    d = _tree()
    p = tmp_path / "voc.txt"
    p.write_text(_text(d, header="10 6 1 2", tail=tail))
    lines = _run(driver, "text", str(p))
    c = _created(lines[0])
    _same_arrays(c, d, d["weight"])      # (no junk child of the root behind the last line)
    assert (c["weighting"], c["norm"]) == (2, 2)      # IDF; L2_NORM normalises with L2
    assert lines[1] == "loaded 1 size %d empty 0" % int(d["is_leaf"].sum())


@pytest.mark.parametrize("scoring, norm", [(0, 1), (1, 2), (2, 1), (3, 1), (4, 1), (5, 0)])
def test_binary_loader_and_the_norm_of_every_scoring_type(driver, tmp_path, scoring, norm):
    d = _tree()
    p = tmp_path / "voc.bin"
    p.write_bytes(_binary(d, scoring=scoring, weighting=1))
    lines = _run(driver, "binary", str(p))
    c = _created(lines[0])
    _same_arrays(c, d, d["weight"].astype(np.float32).astype(np.float64))      # the file stores float, promoted
    assert (c["weighting"], c["norm"]) == (1, norm)
    # size(): the leaf-flagged nodes of the file, not one more for a duplicate of the last node
    assert lines[1] == "loaded 1 size %d empty 0" % int(d["is_leaf"].sum())
    assert any(ln.startswith("scores refused") for ln in lines) == (scoring != 0)      # score / scoreBatch: L1_NORM only


def test_rejected_files(driver, tmp_path):
    d = _tree()
    cases = {"k.txt": _text(d, header="25 6 0 0"), "L.txt": _text(d, header="10 0 0 0"), "scoring.txt": _text(d, header="10 6 6 0"), "weighting.txt": _text(d, header="10 6 0 4"),
             "short_line.txt": _text(d)[:-40] + "\n", "empty.txt": ""}
    for name, txt in cases.items():
        p = tmp_path / name
        p.write_text(txt)
        lines = _run(driver, "text", str(p))
        assert lines[-1] == "loaded 0 size 0 empty 1" and not any(ln.startswith("create") for ln in lines), name
    for name, blob in {"size_node.bin": _binary(d, size_node=40), "truncated.bin": _binary(d, drop=5), "scoring.bin": _binary(d, scoring=6), "head.bin": b"\x01\x02"}.items():
        p = tmp_path / name
        p.write_bytes(blob)
        lines = _run(driver, "binary", str(p))
        assert lines[-1] == "loaded 0 size 0 empty 1" and not any(ln.startswith("create") for ln in lines), name
    assert _run(driver, "text", str(tmp_path / "missing"))[-1] == "loaded 0 size 0 empty 1"
    # a node the library rejects (its parent comes after it): create is called, the loader returns false
    bad = dict(d, parent=d["parent"].copy())
    bad["parent"][2] = 5
    p = tmp_path / "order.txt"
    p.write_text(_text(bad))
    lines = _run(driver, "text", str(p))
    assert lines[0].startswith("create") and lines[1] == "loaded 0 size 0 empty 1"


def test_maps_are_rebuilt_and_score_batch_is_packed(driver, tmp_path):
    d = _tree()
    p = tmp_path / "voc.txt"
    p.write_text(_text(d))
    lines = _run(driver, "text", str(p))
    feats = np.array([[7 * i + 3, i * i] + [i] * 30 for i in range(6)], np.uint8)
    call = lines[2].split()
    assert call[:5] == ["transform", "n", "6", "levelsup", "4"] and np.array_equal(np.array(call[6:], np.uint8).reshape(6, 32), feats)
    # the stub's rule restated: word d[0] % 5 with 0.5 per feature, node 10 + d[1] % 3
    words, nodes = {}, {}
    for i in range(6):
        words[int(feats[i, 0]) % 5] = words.get(int(feats[i, 0]) % 5, 0) + 1
        nodes.setdefault(10 + int(feats[i, 1]) % 3, []).append(i)
    assert lines[3] == "bow " + " ".join("%d:%s" % (k, "%.17g" % (0.5 * words[k])) for k in sorted(words))
    assert lines[4] == "fv " + " ".join("%d:%s" % (k, ",".join(str(i) for i in nodes[k])) for k in sorted(nodes))
    v = (np.array(sorted(words), np.uint32), np.array([0.5 * words[k] for k in sorted(words)]))
    second = (np.array([0, 3, 4, 77], np.uint32), np.array([0.125, 0.3, 0.7, 0.1]))
    none = (np.zeros(0, np.uint32), np.zeros(0))
    call = lines[5].split()
    nq = len(v[0])
    assert call[:3] == ["score", "nq", str(nq)]
    pairs = lambda vec: ["%d:%.17g" % (k, x) for k, x in zip(*vec)]      # noqa: E731
    assert call[4:4 + nq] == pairs(v)
    assert call[4 + nq:4 + nq + 6] == ["ndb", "3", "start", "0", str(nq), str(nq + 4)] and call[4 + nq + 6] == str(nq + 4)
    assert call[4 + nq + 7] == "db" and call[4 + nq + 8:] == pairs(v) + pairs(second)
    assert lines[6] == "scores " + " ".join("%.17g" % (1000.0 * nq + 10.0 * m + 0.25 * j) for j, m in enumerate((nq, 4, 0)))
    # the host score: ScoringObject.cpp:23-68 op for op
    assert lines[7] == "host " + " ".join("%.17g" % Y.score_l1(v, w) for w in (v, second, none))
    assert lines[7].split()[3] == "-0"
    assert lines[-1] == "destroy"
