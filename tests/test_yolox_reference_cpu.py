"""The yolox yardstick (tests/yolox_reference.py) against itself, without a device: the literal transcription against the vectorised form on every scene, every
scene reaching the branch it names, the geometry of StaticResize, and the variant condition -- outside the declared tie scenes the double-precision
exponential and the recorded expf of the machine that wrote the golden files give the same proposal order, picks and labels, and no quotient the greedy loop
compares lies within 1e-4 of 0.65f, so neither exponential nor a last-bit difference of a box can move a verdict."""
import os
import sys

import numpy as np
import pytest

import yolox_reference as Y
import yolox_scenes as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden_yolox as G  # noqa: E402

SCENES = SC.scenes()
SMALL = sorted(n for n, s in SCENES.items() if s["S"] == 64)
MARGIN = 1e-4


@pytest.fixture(scope="module")
def decoded():
    """every scene once: literal (the reference's order), literal under the stable rule, vectorised"""
    out = {}
    for name, s in SCENES.items():
        a = (s["feat"], s["S"], *s["img"])
        out[name] = dict(literal=Y.decode_literal(*a), stable=Y.decode_literal(*a, stable=True), vec=Y.decode_vectorised(*a))
    return out


@pytest.mark.parametrize("name", sorted(SCENES))
def test_literal_equals_vectorised(decoded, name):
    d = decoded[name]
    for k in ("objects", "proposals"):
        assert Y.same_records(d["stable"][k], d["vec"][k]), k
    assert d["stable"]["picked"] == d["vec"]["picked"] and d["stable"]["n_tied"] == d["vec"]["n_tied"] == d["literal"]["n_tied"]
    if not SCENES[name]["tie"]:
        assert d["literal"]["n_tied"] == 0 and Y.same_records(d["literal"]["objects"], d["stable"]["objects"])
        assert Y.same_records(d["literal"]["proposals"], d["stable"]["proposals"])


@pytest.mark.parametrize("name", sorted(SCENES))
def test_scene_reaches_its_branch(decoded, name):
    assert SCENES[name]["reaches"](decoded[name]["stable"]), SCENES[name]["branch"]
    assert SCENES[name]["reaches"](decoded[name]["literal"]), SCENES[name]["branch"]


def test_the_tie_scene_orders_differ(decoded):
    d = decoded["tie"]
    assert d["literal"]["n_tied"] == 7 and not Y.same_records(d["literal"]["objects"], d["stable"]["objects"])
    # (two classes of anchor 50 share one box and one prob: whichever the sort puts first suppresses the other, so even the surviving label depends on the rule)
    assert len(d["literal"]["objects"]) == len(d["stable"]["objects"]) == 7


@pytest.mark.parametrize("name", sorted(SCENES))
def test_variant_condition(decoded, name):
    """both exponentials: one proposal order, one set of picks, one list of labels; every compared quotient at least 1e-4 from the threshold in both"""
    z = G.load(name)
    ex = Y.exp_table(z["expf_in"], z["expf_out"])
    s = SCENES[name]
    a = Y.decode_literal(s["feat"], s["S"], *s["img"], stable=True)
    b = Y.decode_literal(s["feat"], s["S"], *s["img"], ex=ex, stable=True)
    for r in (a, b):
        q = r["ious"][np.isfinite(r["ious"])]
        assert (np.abs(q.astype(np.float64) - np.float64(Y.NMS)) >= MARGIN).all(), "a quotient within %g of the threshold" % MARGIN
    assert a["picked"] == b["picked"]
    assert np.array_equal(a["proposals"]["label"], b["proposals"]["label"]) and np.array_equal(a["proposals"]["prob"], b["proposals"]["prob"])
    assert np.array_equal(a["objects"]["label"], b["objects"]["label"])


def test_both_sides_of_the_threshold_are_tested(decoded):
    q = np.concatenate([decoded[n]["stable"]["ious"] for n in SCENES])
    q = q[np.isfinite(q)]
    assert (q > Y.NMS).sum() >= 10 and ((q < Y.NMS) & (q > 0)).sum() >= 10


def test_geometry():
    assert Y.geometry(1064, 20, 640)[1:] == (639, 12)            # the float product 0.6015038 * 1064 is below 640
    assert Y.geometry(848, 480, 640)[1:] == (640, 362)
    assert Y.geometry(100, 700, 640)[1:] == (91, 640)
    assert Y.geometry(640, 480, 640) == (np.float32(1), 640, 480)
    assert Y.geometry(5000, 1, 640) is None and Y.geometry(1, 700, 640) is None
    short = [w for w in range(641, 4097) if Y.geometry(w, 8, 640)[1] == 639]
    assert len(short) == 45 and {1064, 1101, 1122, 1129, 1131} <= set(short)


def test_letterbox_identity_and_halving(oracle):
    rs = np.random.RandomState(11)
    img = rs.randint(0, 256, (48, 64, 3)).astype(np.uint8)
    c = Y.letterbox(img, 64, oracle.resize_linear)                 # r == 1
    assert np.array_equal(c[:48], img) and (c[48:] == Y.PAD).all()
    big = rs.randint(0, 256, (40, 128, 3)).astype(np.uint8)        # r == 0.5
    c = Y.letterbox(big, 64, oracle.resize_linear)
    q = big.astype(np.int32)
    assert np.array_equal(c[:20], ((q[0::2, 0::2] + q[0::2, 1::2] + q[1::2, 0::2] + q[1::2, 1::2] + 2) >> 2).astype(np.uint8))
    assert (c[20:] == Y.PAD).all()


def test_blob_forms_agree(oracle):
    img = np.random.RandomState(12).randint(0, 256, (23, 37, 3)).astype(np.uint8)
    c = Y.letterbox(img, 64, oracle.resize_linear)
    a, b = Y.blob_literal(c), Y.blob_vectorised(c)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.array_equal(b[:, 63, 63].view(np.uint32), Y.blob_table()[:, Y.PAD].view(np.uint32))
    assert b[0, 0, 0] == Y.blob_table()[0, c[0, 0, 2]]            # channel 0 of the blob is byte 2 of the pixel


def test_exp_double_at_the_ends():
    assert Y.exp_double(np.float32(800)) == np.inf and Y.exp_double(np.float32(100)) == np.inf and Y.exp_double(np.float32(-120)) == 0
    assert Y.exp_double(np.float32(0)) == 1


def test_tracking_filter():
    o = Y.records([(0, 0, 1, 1, 0.5, 0), (0, 0, 1, 1, 0.49999, 0), (0, 0, 1, 1, 0.9, 1), (0, 0, 1, 1, 0.7, 73), (0, 0, 1, 1, 0.8, 62)])
    t = Y.tracking_boxes(o)
    assert t["label"].tolist() == [62, 73, 0] and t["prob"].tolist() == [np.float32(0.8), np.float32(0.7), np.float32(0.5)]


def test_golden_files_equal_a_fresh_run(oracle):
    have = sorted(f[:-4] for f in os.listdir(G.OUT) if f.endswith(".npz"))
    assert have == sorted(list(SCENES) + [G.FRAME])
    fresh = {name: G.scene_record(s) for name, s in SCENES.items()}
    fresh[G.FRAME] = G.frame()
    for name, rec in fresh.items():
        z = G.load(name)
        for k, v in rec.items():
            assert np.asarray(v).dtype == z[k].dtype and np.asarray(v).tobytes() == z[k].tobytes(), (name, k)
