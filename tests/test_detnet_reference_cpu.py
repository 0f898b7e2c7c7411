"""The numpy yardstick of the detector network (tests/detnet_reference.py) on its own: its fmaf emulation against std::fmaf of tools/detnet_walk.cpp, and each
op against torch in float64 on the same input, within bounds that are derived and not measured."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detnet_models as M  # noqa: E402
import detnet_reference as R  # noqa: E402
from eao_fusion_amd import detnet as D  # noqa: E402

F = np.float32


def walk_fma(triples):
    exe = M.walk_binary(("-O2",))
    with tempfile.TemporaryDirectory() as d:
        pi, po = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        np.ascontiguousarray(triples, "<f4").tofile(pi)
        subprocess.check_call([exe, "fma", pi, po])
        return np.fromfile(po, "<f4")


def planted_midpoints():
    """x * w + a whose float64 sum is a float32 midpoint while the exact sum is not: a has an odd last bit, x * w is half an ulp of a times (1 - 2^-46).  The exact
    sum lies below (above, for the subtracted form) the midpoint, the float64 sum lands on it, and a second round-to-nearest-even then leaves a."""
    e = F(2.0) ** F(-23)
    rows = []
    for scale in (F(1.0), F(2.0) ** F(40), F(2.0) ** F(-60)):
        for sign in (F(1.0), F(-1.0)):
            a = sign * (F(1.0) + e) * scale
            x = (F(1.0) + e) * F(2.0) ** F(-24) * scale
            w = F(1.0) - e
            rows.append((x, sign * w, a))           # towards the upper neighbour: fmaf stays at a
            rows.append((x, -sign * w, a))          # towards the lower neighbour: fmaf stays at a
    return np.array(rows, F)


def test_fma_emulation_equals_std_fmaf_on_a_million_triples():
    rng = np.random.default_rng(20261020)
    n = 1_000_000
    t = np.empty((n, 3), F)
    # a third each: ordinary values, products that nearly cancel the addend, raw bit patterns (subnormals, infinities, NaN)
    t[: n // 3] = rng.standard_normal((n // 3, 3)) * np.exp(rng.uniform(-30, 30, (n // 3, 3)))
    m = n // 3
    x, w = rng.standard_normal(m).astype(F), rng.standard_normal(m).astype(F)
    t[m:2 * m, 0], t[m:2 * m, 1] = x, w
    t[m:2 * m, 2] = -(x.astype(np.float64) * w.astype(np.float64) * (1 + rng.integers(-3, 4, m) * 2.0 ** -24)).astype(F)
    t[2 * m:] = rng.integers(0, 1 << 32, (n - 2 * m, 3), dtype=np.uint64).astype(np.uint32).view(F)
    want = walk_fma(t)
    got = R.fma(t[:, 0], t[:, 1], t[:, 2])
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))


def test_fma_emulation_on_planted_midpoints_where_double_rounding_fails():
    t = planted_midpoints()
    want = walk_fma(t)
    assert np.array_equal(want.view(np.uint32), t[:, 2].view(np.uint32)), "the planted cases are meant to leave the addend"
    assert np.array_equal(R.fma(t[:, 0], t[:, 1], t[:, 2]).view(np.uint32), want.view(np.uint32))
    twice = R.fma_double_rounding(t[:, 0], t[:, 1], t[:, 2])
    assert (twice.view(np.uint32) != want.view(np.uint32)).all(), "plain double rounding is meant to fail on every planted case"


def test_exp_is_the_host_header_s():
    # through the walk: a 1 x 1 sigmoid convolution with weight 1 and bias 0 is sigmoid(x); the yardstick's exp must give the same bits
    x = np.concatenate([np.linspace(-30, 30, 4001), [-104.5, -103.9, 88.9, 89.5, 0.0, -0.0]]).astype(F).reshape(-1, 1, 1)
    sc = M.single_conv(x, np.ones((1, 1, 1, 1), F), np.zeros(1, F), act=D.SIGMOID)
    t, _ = M.walk_run(M.walk_binary(("-O2",)), sc["model"], 32, inputs=sc["inputs"])
    assert M.same_bits(t[sc["dst"]], R.sigmoid(R.fma(x, F(1.0), F(0.0))))


CONV_CASES = [(9, 8, 3, 5, 3, 1), (6, 7, 12, 4, 3, 2), (5, 5, 33, 6, 1, 1), (8, 6, 64, 3, 3, 1), (7, 9, 5, 2, 1, 2)]


@pytest.mark.parametrize("H,W,ci,co,k,stride", CONV_CASES)
def test_convolution_against_torch_float64(H, W, ci, co, k, stride):
    import torch
    rng = np.random.default_rng(H * 1000 + ci)
    x, w, b = rng.standard_normal((H, W, ci)).astype(F), rng.standard_normal((co, k, k, ci)).astype(F), rng.standard_normal(co).astype(F)
    pre = R.conv_pre(x, w, b, stride)
    tx = torch.from_numpy(x.astype(np.float64)).permute(2, 0, 1)[None]
    tw = torch.from_numpy(w.astype(np.float64)).permute(0, 3, 1, 2)
    ref = torch.nn.functional.conv2d(tx, tw, torch.from_numpy(b.astype(np.float64)), stride=stride, padding=(k - 1) // 2)[0].permute(1, 2, 0).numpy()
    mag = torch.nn.functional.conv2d(tx.abs(), tw.abs(), torch.from_numpy(np.abs(b).astype(np.float64)), stride=stride, padding=(k - 1) // 2)[0].permute(1, 2, 0).numpy()
    K = k * k * ci
    # a chain of K fused multiply-adds: K roundings of at most half an ulp of a partial sum, each partial sum at most sum |x w| + |b| (1 + u)^K
    bound = (K + 1) * 2.0 ** -24 * mag
    assert pre.shape == ref.shape and (np.abs(pre.astype(np.float64) - ref) <= bound).all()
    # sigmoid and SiLU: exp, the sum, the quotient (and the product) each round once, half an ulp each: within 4 ulp of the float64 formula
    p64 = pre.astype(np.float64)
    for act, f64 in ((D.SIGMOID, 1.0 / (1.0 + np.exp(-p64))), (D.SILU, p64 / (1.0 + np.exp(-p64)))):
        got = R.activate(pre, act)
        ulp = np.spacing(np.abs(f64).astype(F)).astype(np.float64)
        assert (np.abs(got.astype(np.float64) - f64) <= 4 * ulp).all()


def test_maxpool_and_upsample_against_torch():
    import torch
    rng = np.random.default_rng(5)
    x = rng.standard_normal((7, 6, 4)).astype(F)
    tx = torch.from_numpy(x).permute(2, 0, 1)[None]
    for k in (5, 9, 13):
        ref = torch.nn.functional.max_pool2d(tx, k, 1, k // 2)[0].permute(1, 2, 0).numpy()
        assert M.same_bits(R.maxpool(x, k), ref)
    # repeated 5 x 5 is 9 x 9 and 13 x 13, also over +-0 and NaN
    p = M.planted_maps(9, 8, 3, 6)
    p[~np.isfinite(p)] = F(-0.0)
    p[0, 0, 0] = np.nan
    assert M.same_bits(R.maxpool(R.maxpool(p, 5), 5), R.maxpool(p, 9)) and M.same_bits(R.maxpool(R.maxpool(R.maxpool(p, 5), 5), 5), R.maxpool(p, 13))
    z = R.maxpool(np.array([[[0.0], [-0.0]], [[-0.0], [-0.0]]], F), 3)
    assert (z.view(np.uint32) == 0).all(), "+0 is above -0"
    assert (R.maxpool(np.full((2, 2, 1), -0.0, F), 3).view(np.uint32) == 0x80000000).all()
    nanmap = R.maxpool(p, 5)
    assert (nanmap[:3, :3, 0].view(np.uint32) == 0x7fc00000).all() and not np.isnan(nanmap[4:, 4:, 0]).any()
    ref = torch.nn.functional.interpolate(tx, scale_factor=2, mode="nearest")[0].permute(1, 2, 0).numpy()
    assert M.same_bits(R.upsample2(x), ref)


def test_focus_order():
    b = M.blob(8, 3)
    f = R.focus(b)
    assert f.shape == (4, 4, 12)
    assert f[1, 2, 0] == b[0, 2, 4] and f[1, 2, 3 + 1] == b[1, 3, 4] and f[1, 2, 6 + 2] == b[2, 2, 5] and f[1, 2, 9] == b[0, 3, 5]
