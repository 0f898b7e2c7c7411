"""CPU: the triangulation yardstick (tests/triangulation_reference.py) and its scenes (tests/triangulation_scenes.py) hold what they claim; the bands file, the
tolerances and the probe agree; the loop's literals in the kernel's constant block, the yardstick and the adapter are those of the reference text; the header, the
ctypes mirror and the golden files carry the feature."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from reference_literals import literals  # noqa: E402
import triangulation_reference as Y  # noqa: E402
import triangulation_scenes as S  # noqa: E402
import triangulation_tolerances as T  # noqa: E402


@pytest.fixture(scope="module")
def runs():
    return {name: Y.triangulate_batch(sc["K1"], sc["cam1"], sc["K2s"], sc["cams2"], sc["match12"], sc["ratio_factor"]) for name, sc in S.all_scenes().items()}


def test_scenes_have_the_stated_sizes():
    sc = S.all_scenes()
    per_nb = {int((row >= 0).sum()) for s in sc.values() for row in s["match12"]}
    assert {0, 1, 63, 64, 65, 257} <= per_nb
    assert {len(s["K2s"]) for s in sc.values()} >= {1, 3, 20}
    assert all(len(s["K1"]["kp_x"]) % 64 for s in sc.values())
    w = sc["wide_mono"]["match12"]
    assert (w[0] >= 0).any() and not (w[1] >= 0).any() and (w[2] >= 0).any()      # an empty row between two populated ones
    assert len(sc["twenty"]["K1"]["kp_x"]) > 1024                                  # more than one workgroup per neighbour
    assert np.abs(sc["twenty"]["cam1"]["Ow"]).max() >= 100
    assert not np.array_equal(sc["stereo_mix"]["K1"]["raw_x"], sc["stereo_mix"]["K1"]["kp_x"])
    cams = [sc["wide_mono"]["cam1"]] + sc["wide_mono"]["cams2"]
    assert len({float(c["fx"]) for c in cams}) == len(cams)                        # different intrinsics per keyframe
    assert float(sc["stereo_mix"]["cams2"][3]["mbf"]) != float(sc["stereo_mix"]["cam1"]["mbf"])


@pytest.mark.parametrize("name", list(S.all_scenes()))
def test_scene_reaches_what_it_claims(runs, name):
    sc = S.all_scenes()[name]
    _v, _x, per = runs[name]
    got = {}
    for k, p in enumerate(per):
        for i1, v in zip(p["idx1"], p["pair_verdict"]):
            kind = sc["kinds"][k][int(i1)]
            if kind in S.EXPECT:
                assert int(v) in S.EXPECT[kind], "%s: neighbour %d slot %d of kind %s ends at %s" % (name, k, i1, kind, Y.VERDICT_NAMES[v])
                got[kind] = got.get(kind, 0) + 1
    assert sc["claims"] and set(sc["claims"]) <= set(S.EXPECT)
    for kind, least in sc["claims"].items():
        assert got.get(kind, 0) >= least, (name, kind, got.get(kind, 0), least)
    assert set(got) <= set(sc["claims"]), (name, set(got) - set(sc["claims"]))      # no kind goes unclaimed


def test_every_verdict_is_reached(runs):
    total = np.zeros(13, np.int64)
    for v, _x, _per in runs.values():
        total += np.bincount(v.ravel(), minlength=13)
    for code, least in S.MIN_PER_VERDICT.items():
        assert total[code] >= least, (Y.VERDICT_NAMES[code], int(total[code]), least)


def test_stereo_quirks_decide_verdicts(runs):
    sc = S.all_scenes()["stereo_mix"]
    _v, _x, per = runs["stereo_mix"]
    # the `else if` of :317: with stereo on both sides (neighbour 2) only keyframe 1 unprojects
    assert (sc["K2s"][2]["u_right"][per[2]["idx2"]] >= 0).all() and set(per[2]["pair_verdict"]) <= {Y.UNPROJECTED_1, Y.NO_DEPTH, Y.REPROJ_1}
    assert (per[2]["pair_verdict"] == Y.UNPROJECTED_1).sum() >= 50
    # :410: with the neighbour's own mbf in its place the `mbf2` pairs would pass
    cam1b = dict(sc["cam1"], mbf=sc["cams2"][3]["mbf"])
    own = Y.triangulate_neighbour(sc["K1"], cam1b, sc["K2s"][3], sc["cams2"][3], sc["match12"][3], sc["ratio_factor"])
    kinds = sc["kinds"][3]
    mbf2 = np.array([kinds[int(i)] == "mbf2" for i in per[3]["idx1"]])
    assert mbf2.sum() >= 10 and (per[3]["pair_verdict"][mbf2] == Y.REPROJ_2).all() and (own["pair_verdict"][mbf2] != Y.REPROJ_2).all()
    # right1: the left error alone passes 5.991 (with the keypoint made monocular the pair is accepted)
    K1m = dict(sc["K1"], u_right=np.full_like(sc["K1"]["u_right"], -1))
    mono = Y.triangulate_neighbour(K1m, sc["cam1"], sc["K2s"][3], sc["cams2"][3], sc["match12"][3], sc["ratio_factor"])
    r1 = np.array([kinds[int(i)] == "right1" for i in per[3]["idx1"]])
    assert r1.sum() >= 10 and (per[3]["pair_verdict"][r1] == Y.REPROJ_1).all() and (mono["pair_verdict"][r1] != Y.REPROJ_1).all()


def test_nan_row_falls_through_as_upstream_writes_it(runs):
    sc = S.all_scenes()["nan_row"]
    v, x, _per = runs["nan_row"]
    a, b = sc["nan_slots"]
    assert v[0, a] == Y.LOW_PARALLAX and not x[0, a].any()
    assert v[0, b] == Y.UNPROJECTED_1 and np.isnan(x[0, b]).any()


@pytest.mark.parametrize("name", [n for n, s in S.all_scenes().items() if s["friendly"]])
def test_friendly_scenes_stay_clear_of_the_gates(runs, name):
    _v, _x, per = runs[name]
    near = np.concatenate([p["near"] for p in per])
    assert len(near) and (near < T.MARGIN_REL).mean() <= T.IN_MARGIN_MAX_SHARE


def test_svd_variants_agree_within_the_band(runs):
    for name, sc in S.all_scenes().items():
        if not sc["friendly"]:
            continue
        v2, x2, _ = Y.triangulate_batch(sc["K1"], sc["cam1"], sc["K2s"], sc["cams2"], sc["match12"], sc["ratio_factor"], "jacobi32")
        v, x, _ = runs[name]
        assert np.array_equal(v, v2)
        acc = np.isin(v, Y.ACCEPTING)
        d = np.linalg.norm(x.astype(np.float64) - np.asarray(sc["cam1"]["Ow"], np.float64), axis=2)
        assert (np.linalg.norm(x.astype(np.float64) - x2, axis=2)[acc] <= T.x3d_rel(name) * d[acc]).all()


def test_bands_file_tolerances_and_probe_agree():
    import triangulation_bands as B
    txt = open(os.path.join(ROOT, "profiles", "triangulation_bands.txt")).read()
    const = {m.group(1): m.group(2) for m in re.finditer(r"^constant (\w+) (\S+)", txt, flags=re.M)}
    want = {"X3D_REL": "%.3e" % T.X3D_REL, "MARGIN_REL": "%.3e" % T.MARGIN_REL}
    want.update({"X3D_REL_" + name: "%.3e" % v for name, v in T.X3D_REL_BY_SCENE.items()})
    assert const == want and set(T.X3D_REL_BY_SCENE) == {n for n, s in S.all_scenes().items() if s["friendly"]}
    assert max(T.X3D_REL_BY_SCENE.values()) == T.X3D_REL
    assert B.render(B.measure()) == txt


def test_the_loops_literals_are_the_reference_text():
    lit = literals("triangulation")      # (held to the reference text by tests/test_reference_literals.py)
    assert set(lit) == {"RATIO_FACTOR_BASE", "LOW_PARALLAX_COS", "CHI2_MONO", "CHI2_STEREO"}
    # the yardstick
    for name, literal in lit.items():
        assert getattr(Y, name) == float(literal), name
    # the kernel's block: one named constant per literal, and no other line of the file spells one
    src = open(os.path.join(ROOT, "eao_fusion_amd", "csrc", "triangulate.hip")).read()
    code = [re.sub(r"//.*", "", ln) for ln in re.sub(r"/\*.*?\*/", "", src, flags=re.S).split("\n")]
    names = {"LOW_PARALLAX_COS": "kLowParallaxCos", "CHI2_MONO": "kChi2Mono", "CHI2_STEREO": "kChi2Stereo", "RATIO_FACTOR_BASE": "kRatioFactorBase"}
    for name, literal in lit.items():
        decl = [ln for ln in code if re.search(r"constexpr (double|float) %s = %sf?;" % (names[name], re.escape(literal)), ln)]
        assert len(decl) == 1, name
        others = [ln for ln in code if re.search(r"(?<![\w.])%s(?![\w.])f?" % re.escape(literal), ln) and ln not in decl]
        assert not others, (name, others)
    # the adapter forms ratioFactor from the same literal
    hdr = open(os.path.join(ROOT, "include", "eaofusion", "LocalMapping.h")).read()
    assert re.search(r"static constexpr float RATIO_FACTOR_BASE = %sf;" % re.escape(lit["RATIO_FACTOR_BASE"]), hdr)
    # the file is none of the consumers that test_ref_constants forbids these literals in, and the generated headers are untouched by it
    import test_ref_constants as RC
    assert not any("triangulate" in rel for rels in RC.CONSUMERS.values() for rel in rels)


def test_header_and_mirror_carry_the_feature():
    hdr = open(os.path.join(ROOT, "include", "eao_fusion.h")).read()
    for sym in ("eao_triangulate_matches_batch", "eao_keyframe_set_depth", "eao_kf_create_new_map_points", "eao_tri_camera", "eao_tri_verdict"):
        assert sym in hdr, sym
    codes = dict(re.findall(r"EAO_TRI_(\w+) = (\d+)", hdr))
    assert {k: int(v) for k, v in codes.items()} == {n: i for i, n in enumerate(Y.VERDICT_NAMES)}
    assert "src/LocalMapping.cc:288-454" in hdr and "src/KeyFrame.cc:654-670" in hdr
    from eao_fusion_amd import _lib, search
    for sym in ("eao_triangulate_matches_batch", "eao_keyframe_set_depth", "eao_kf_create_new_map_points"):
        assert sym in _lib.SYMBOLS
    assert [getattr(search, "TRI_" + n) for n in Y.VERDICT_NAMES] == list(range(13))
    assert all(callable(getattr(search, f)) for f in ("triangulate_matches_batch", "keyframe_set_depth", "kf_create_new_map_points"))
    import ctypes
    assert ctypes.sizeof(search.TriCamera) == 4 * 23


def test_golden_files_freeze_the_yardstick(runs):
    import gen_golden_triangulation as G
    got = G.build()
    # the recorded scene stays clear of every comparison: the device tests hold ALL its verdicts to the file
    assert min(p["near"].min() for p in runs["stereo_mix"][2] if len(p["near"])) > 10 * T.MARGIN_REL
    for fn, arrays in got.items():
        z = np.load(os.path.join(ROOT, "tests", "golden", "triangulation", fn))
        assert set(z.files) == set(arrays)
        for k, a in arrays.items():
            assert np.array_equal(z[k], a, equal_nan=True), (fn, k)


def test_arguments_are_checked_before_the_device_is_asked_for():
    """The host-array entry point refuses malformed input with EAO_ERR_INVALID and writes nothing -- with or without a device in the machine; every scene of the
    GPU tests passes that check (without a device the call then ends with EAO_ERR_NO_DEVICE: there is no CPU path)."""
    from eao_fusion_amd import _lib, search
    g = search.product()
    sc = S.all_scenes()["stereo_mix"]
    n_nb, n1 = sc["match12"].shape
    v, x = np.full((n_nb, n1), -7, np.int32), np.full((n_nb, n1, 3), np.float32(-7), np.float32)
    bad = sc["match12"].copy()
    bad[1, 5] = len(sc["K2s"][1]["kp_x"])
    k1 = dict(sc["K1"], kp_octave=np.where(np.arange(n1) == 3, 8, sc["K1"]["kp_octave"]).astype(np.int32))
    for K1, m, kw in ((sc["K1"], sc["match12"], dict(out=(None, x))), (sc["K1"], sc["match12"], dict(out=(v, None))), (sc["K1"], sc["match12"], dict(out=(v, x), n_nb=-1)),
                      (sc["K1"], bad, dict(out=(v, x))), (k1, sc["match12"], dict(out=(v, x)))):
        with pytest.raises(_lib.EaoError) as ei:
            g.triangulate_matches_batch(K1, sc["cam1"], sc["K2s"], sc["cams2"], m, sc["ratio_factor"], **kw)
        assert ei.value.status == _lib.EAO_ERR_INVALID
    assert (v == -7).all() and (x == -7).all()
    if _lib.load().eao_device_check() == _lib.EAO_ERR_NO_DEVICE:
        for s in S.all_scenes().values():
            with pytest.raises(_lib.EaoError) as ei:
                g.triangulate_matches_batch(s["K1"], s["cam1"], s["K2s"], s["cams2"], s["match12"], s["ratio_factor"])
            assert ei.value.status == _lib.EAO_ERR_NO_DEVICE
