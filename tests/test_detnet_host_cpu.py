"""The host header of the detector network (eao_fusion_amd/csrc/detnet_internal.h) as a stand-alone program under AddressSanitizer and UBSan
(tools/detnet_walk.cpp): it equals the numpy yardstick on every scene, bit for bit, and it refuses every broken file with a message and a clean exit."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detnet_models as M  # noqa: E402
import detnet_reference as R  # noqa: E402

SAN = ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
SCENES = M.scenes()
BROKEN = M.broken_files()


@pytest.fixture(scope="module")
def walk():
    return M.walk_binary(SAN)


@pytest.mark.parametrize("name", sorted(SCENES))
def test_walk_equals_the_yardstick(walk, name):
    sc = SCENES[name]
    want_t, want_head = R.forward(sc["model"], sc["S"], sc.get("blob"), sc["inputs"])
    got_t, got_head = M.walk_run(walk, sc["model"], sc["S"], sc.get("blob"), sc["inputs"])
    assert sorted(got_t) == sorted(want_t)
    for t in want_t:
        assert M.same_bits(got_t[t], want_t[t]), "tensor %d differs" % t
    assert (want_head is None) == (got_head is None) and (want_head is None or M.same_bits(got_head, want_head))


def test_the_planted_minus_zero_survives():
    sc = SCENES["conv_minus_zero_bias"]
    t, _ = R.forward(sc["model"], sc["S"], None, sc["inputs"])
    assert (t[sc["dst"]].view(np.uint32) == 0x80000000).all()


def test_the_optimised_walks_agree(walk):
    sc = SCENES["yolox_nano_width_32"]
    a = M.walk_run(walk, sc["model"], 32, sc["blob"])[1]
    for flags in (("-O2",), ("-O3",)):
        assert M.same_bits(M.walk_run(M.walk_binary(flags), sc["model"], 32, sc["blob"])[1], a)


@pytest.mark.parametrize("name", sorted(BROKEN))
def test_walk_refuses(walk, name):
    data, S, word = BROKEN[name]
    ok, out, code, err = M.walk_check(walk, data, S)
    assert not ok and out.startswith("refused: ") and word in out, out
    assert code == 0 and err == "", err[-2000:]


def test_the_good_file_is_accepted_at_every_size(walk):
    data = SCENES["yolox_nano_width_32"]["model"].tobytes()
    for S in (32, 64, 640):
        assert M.walk_check(walk, data, S)[0]
    assert not M.walk_check(walk, data, 48)[0]
