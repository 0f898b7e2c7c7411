"""The host half of the device isolation forest (eao_fusion_amd/csrc/iforest_internal.h) without a device: tools/isolation_forest_walk.cpp -- the forest built on
the host in the kernel's sort-free form, upstream's rules and removal over a stand-in object -- is built with g++ -fsanitize=address,undefined and run as a
program of its own.  It must print the recorded bytes of the reference's own Serialize and its scores on every fixture, the yardstick's total path lengths, and
erase exactly the flagged points, the object whose last point is the last outlier included."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import isolation_forest_reference as Y
import isolation_forest_scenes as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "isolation_forest")
SCENES = SC.scenes()


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("iforest") / "isolation_forest_walk")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tools", "isolation_forest_walk.cpp"), "-o", exe])
    return exe


def hx(a):
    return " ".join("%08x" % v for v in np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32))


def run_walk(walk, script):
    out = subprocess.run([walk], input=script, capture_output=True, text=True)
    assert out.returncode == 0, "exit %d\n%s" % (out.returncode, out.stderr[-3000:])
    return out.stdout.strip().split("\n") if out.stdout.strip() else []


def doubles(line, tag):
    tok = line.split()
    assert tok[0] == tag and int(tok[1]) == len(tok) - 2
    return np.array([int(h, 16) for h in tok[2:]], np.uint64).view(np.float64)


@pytest.mark.parametrize("name", sorted(SCENES))
def test_every_fixture(walk, name):
    sc = SCENES[name]
    z = np.load(os.path.join(GOLD, name + ".npz"))
    got = run_walk(walk, "%d %d %d %d %s\n" % (sc["tree_count"], sc["seed"], sc["sample_size"], len(sc["points"]), hx(sc["points"])))
    assert got[0] == "built 1"
    _, nbytes, hexs = got[1].split()
    stream = bytes.fromhex(hexs)
    assert len(stream) == int(nbytes) == int(z["stream_len"]) and hashlib.sha256(stream).hexdigest().encode() == z["stream_sha256"].tobytes()
    if "stream" in z.files:
        assert stream == z["stream"].tobytes()
    scores, want = doubles(got[2], "scores"), z["scores"]
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(scores), nan) and (np.abs(scores[~nan].view(np.int64) - want[~nan].view(np.int64)) <= 1).all()
    totals = doubles(got[3], "totals")
    assert np.array_equal(totals.view(np.uint64), Y.total_path_lengths(sc["points"], Y.parse(stream)[1]).view(np.uint64))


def object_line(points, class_id, bi_forest=1):
    return "object %d %d %d %s\n" % (class_id, bi_forest, len(points), hx(points))


def check_removal(got, points, flags):
    assert got[0] == "flags %d %s" % (len(points), " ".join(str(int(f)) for f in flags))
    kept = [int(i) for i in np.nonzero(flags == 0)[0]]
    assert got[1] == ("kept %d %s" % (len(kept), " ".join(str(i) for i in kept))).rstrip()
    total = [0.0, 0.0, 0.0]
    for p in points:      # mSumPointsPos as the stand-in keeps it: every point added in order, the erased ones subtracted in order
        total = [t + float(c) for t, c in zip(total, p)]
    for i in np.nonzero(flags)[0]:
        total = [t - float(c) for t, c in zip(total, points[i])]
    assert np.array_equal(doubles(got[2], "sum").view(np.uint64), np.array(total, np.float64).view(np.uint64))


@pytest.mark.parametrize("name", sorted(n for n, s in SCENES.items() if s["entry"] == "object" and not s.get("by_hash")))
def test_objects_flags_and_removal(walk, name):
    sc = SCENES[name]
    flags = Y.outlier_flags(np.load(os.path.join(GOLD, name + ".npz"))["scores"], sc["class_id"])
    check_removal(run_walk(walk, object_line(sc["points"], sc["class_id"])), sc["points"], flags)


def test_last_point_is_the_last_outlier(walk):
    """upstream's loop reads outliernum one past its end there (src/Object.cc:1336); the walk's list is bounded, and the sanitizers watch"""
    sc = SCENES["gauss_64"]
    flags = Y.outlier_flags(np.load(os.path.join(GOLD, "gauss_64.npz"))["scores"], 0)
    last = int(np.nonzero(flags)[0][-1])
    pts = sc["points"].copy()
    order = np.r_[np.delete(np.arange(len(pts)), last), last]      # the last outlier moved to the end: the forest sees another order, so ask the yardstick
    pts = pts[order]
    _, scores, _ = Y.forest(pts, Y.TREE_COUNT, Y.SEED, len(pts) // 2)
    want = Y.outlier_flags(scores, 0)
    assert want[-1] == 1 and np.abs(scores - np.float64(np.float32(0.6))).min() > 1e-9
    check_removal(run_walk(walk, object_line(pts, 0)), pts, want)


def test_rules_and_refusals(walk):
    p40, p29 = SC._cloud(40, 9), SC._cloud(29, 10)
    bad = p40.copy()
    bad[3, 1] = np.inf
    script = (object_line(p40, 0, bi_forest=0) + object_line(p40, 75) + object_line(p40, 64) + object_line(p40, 65) + object_line(p29, 0) + object_line(bad, 0)
              + "50 1 0 40 %s\n" % hx(p40) + "50 1 41 40 %s\n" % hx(p40) + "0 1 20 40 %s\n" % hx(p40) + "50 1 20 40 %s\n" % hx(bad))
    got = run_walk(walk, script)
    assert got[:5] == ["skipped"] * 5
    assert len(got) == 10 and all(g.startswith("refused") for g in got[5:])
