"""The irregular bundle-adjustment shapes of tests/ba_shapes.py, on the CPU (no GPU needed).  Three things are held here so that tests/test_gpu_ba_shapes.py can hold the
library to the oracle at the unchanged bar (lm_tolerances.UPDATE_REL) on them:
  * every shape still IS what it is named after (its `facts`: degree histograms, empty cameras / landmarks, no right coordinate at zero) -- a later edit of synth_ba cannot
    quietly turn a shape back into an ordinary window -- and the two outlier shapes empty their camera / landmarks already in the first pass (so the row is inactive in the
    second optimize());
  * the conditioning gate: six one-ulp perturbed oracle runs per shape and entry point leave the LM schedule and the outlier table unchanged and move poses / points by at
    most GATE * UPDATE_REL of the largest update (the measured bands: profiles/ba_shapes_oracle_bands.txt, tools/ba_shape_bands.py).  A shape that fails is re-drawn,
    never loosened;
  * the oracle itself handles empty and rank-deficient blocks as a plain solve does: one LM step against a numpy dense solve over poses + points."""
import os

import numpy as np
import pytest

import ba_shapes as S
from lm_tolerances import UPDATE_REL
from test_oracle_lm import check_schur_step_against_dense_step

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the largest band measured when the shapes were drawn is 6.2e-5 of the update (thin_map, BundleAdjustment non-robust, points); the margin keeps a shape from sitting
# right under the bar the GPU is then held to
GATE = 0.7


@pytest.mark.parametrize("name", list(S.SHAPES))
def test_shape_is_what_it_is_named_after(name):
    p, facts = S.shape(name)
    bad = S.check_facts(p, facts)
    assert not bad, "%s: %s" % (name, "; ".join(bad))
    for k in ("poses", "points", "obs", "inv_sigma2"):
        assert p[k].dtype == np.float32 and np.all(np.isfinite(p[k]))
    assert p["edge_cam"].dtype == np.int32 and p["edge_point"].dtype == np.int32
    assert p["edge_cam"].min() >= 0 and p["edge_cam"].max() < len(p["poses"]) and p["edge_point"].min() >= 0 and p["edge_point"].max() < len(p["points"])


def test_every_recipe_of_the_issue_is_there():
    assert set(S.WINDOW_SHAPES) >= {"single_observer", "single_observer_mono", "fixed_only", "long_tracks", "skewed", "camera_all_outliers", "landmarks_all_outliers",
                                    "one_free", "all_mono"}
    assert set(S.MAP_SHAPES) >= {"hub", "long_tracks_map", "thin_map"}
    for name in S.WINDOW_SHAPES:
        assert int((S.shape(name)[0]["fixed"] == 0).sum()) <= 30, "%s is not a window of the tile solver" % name
    for name in S.MAP_SHAPES:
        assert int((S.shape(name)[0]["fixed"] == 0).sum()) > 64, "%s is not beyond every single-workgroup solver" % name


def test_rebuild_never_draws_a_right_coordinate_a_one_ulp_probe_could_flip():
    """obs[:, 2] == 0.0 is a stereo edge and one ulp below it a monocular one: an added observation near zero is made monocular, and the probe never moves a value across zero."""
    for name in S.SHAPES:
        p, _ = S.shape(name)
        assert not np.any(p["obs"][:, 2] == 0.0), name
        for s in range(3):
            q = S.one_ulp(p, s)
            assert np.array_equal(q["obs"][:, 2] < 0, p["obs"][:, 2] < 0), name
            for k in ("points", "obs", "poses"):
                assert np.array_equal(np.sign(q[k]), np.sign(p[k])), (name, k)
                assert np.abs(q[k].view(np.int32).astype(np.int64) - p[k].view(np.int32).astype(np.int64)).max() <= 1, (name, k)
            assert np.array_equal(q["poses"][:, 3, :], p["poses"][:, 3, :])
            assert np.any(q["points"] != p["points"]) and np.any(q["obs"] != p["obs"]) and np.any(q["poses"] != p["poses"])


@pytest.mark.parametrize("name", ["camera_all_outliers", "landmarks_all_outliers"])
def test_the_outlier_pass_empties_what_the_shape_says(oracle, name):
    """Every edge of camera 9 / of the chosen landmarks is an outlier in the oracle's result, and already after the first pass (its = (5, 0) runs the first optimize() and
    the classification behind it): the camera / the landmarks have no active edge in the second optimize()."""
    p, facts = S.shape(name)
    sel = facts["rejected_edges"]
    if "rejected_camera" in facts:
        assert np.array_equal(sel, p["edge_cam"] == facts["rejected_camera"]) and sel.sum() > 100
    else:
        assert np.array_equal(sel, np.isin(p["edge_point"], facts["rejected_landmarks"])) and len(facts["rejected_landmarks"]) == 100
    o, o1 = oracle.local_ba(p), oracle.local_ba(p, its=(5, 0))
    assert o1["edge_outlier"][sel].all(), "%d of %d edges survive the first pass" % (int((o1["edge_outlier"][sel] == 0).sum()), int(sel.sum()))
    assert o["edge_outlier"][sel].all()
    assert o["iters"][1] > 0 and not o["edge_outlier"][~sel].all()          # (there IS a second pass, over the rest of the window)


@pytest.mark.parametrize("name", list(S.SHAPES))
def test_conditioning_gate(oracle, name, capsys):
    """What justifies holding the GPU to UPDATE_REL on this shape: the oracle's own answer moves by less than GATE * UPDATE_REL when its float32 inputs move by one ulp."""
    p, _ = S.shape(name)
    bands = {entry: S.oracle_band(oracle, entry, p) for entry in S.ENTRY_POINTS}
    with capsys.disabled():
        print()
        for entry, b in bands.items():
            print("[ba shapes] %-24s %-10s schedule %s, band: poses %.2e, points %.2e of the largest update" %
                  (name, entry, "same" if b["schedule_stable"] else "DIFFERENT", b["poses"], b["points"]))
    for entry, b in bands.items():
        assert b["schedule_stable"], "%s / %s: one ulp on the inputs changes the oracle's own LM schedule or outlier table: re-draw the shape" % (name, entry)
        assert max(b["poses"], b["points"]) <= GATE * UPDATE_REL, "%s / %s: the oracle's own one-ulp band is %.2e (gate %.1e): re-draw the shape" % (
            name, entry, max(b["poses"], b["points"]), GATE * UPDATE_REL)


def test_measured_bands_are_on_file():
    path = os.path.join(ROOT, "profiles", "ba_shapes_oracle_bands.txt")
    assert os.path.exists(path), "run tools/ba_shape_bands.py"
    text = open(path).read()
    for name in S.SHAPES:
        for entry in S.ENTRY_POINTS:
            assert any(ln.split()[:2] == [name, entry] for ln in text.splitlines()), "%s / %s is missing from %s" % (name, entry, path)


@pytest.mark.parametrize("name", ["single_observer_mono", "fixed_only", "skewed"])
def test_oracle_schur_step_equals_dense_step_on_irregular_graphs(oracle, name):
    """The thing the GPU is compared with, independent of its own Schur code: one LM step (its = (1, 0)) of the oracle against a numpy dense solve over poses + points
    (tests/test_oracle_lm.py, 1e-9 / 1e-10 as there) on the shapes with rank-2 landmark blocks, landmarks that touch no free camera, and a free camera without edges --
    cut to 120 landmarks with the same strides, a size the dense solve takes."""
    p, facts = S.SHAPES[name](n_points=120)
    assert not S.check_facts(p, facts), S.check_facts(p, facts)
    check_schur_step_against_dense_step(oracle, p)
