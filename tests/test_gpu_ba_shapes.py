"""GPU parity on IRREGULAR map graphs: the shapes of tests/ba_shapes.py (landmarks of degree 0 and 1, landmarks nobody free observes, tracks over every camera, a
camera that sees everything beside one that sees nothing, cameras / landmarks emptied by the outlier pass, a hub keyframe in a band map) through every solver path of the
bundle adjustment, each held to the fp64 oracle at the unchanged bar.  Every bound comes from tests/lm_tolerances.py (tests/test_lm_tolerances.py scans this file too);
tests/test_ba_shapes_cpu.py shows on the CPU that the oracle's own one-ulp band on every shape is below 0.7 of that bar.

For every case: iters equal to the oracle's, edge_outlier equal (LocalBundleAdjustment), the LM trace on its well-conditioned prefix, poses and points within UPDATE_REL of
the update (a failure names the camera / landmark and its degree), fixed cameras and cameras / landmarks without any edge bit-equal to what the oracle returns, all finite.
A case that forces a path shows that the path ran (tests/test_gpu_lm.py, _force_map_scale_path: a forced run that silently is the default run is worse than no case)."""
import numpy as np
import pytest

import ba_shapes as S
from eao_fusion_amd import synth
from lm_tolerances import CHI2_REL, CHI2_REL_PLANES
from test_gpu_lm import _bits_differ, _check_trace, _check_updates, _close_result, _force_map_scale_path, _same_result, _shuffle_edges

pytestmark = pytest.mark.gpu

WINDOWS, MAPS = list(S.WINDOW_SHAPES), list(S.MAP_SHAPES)


@pytest.fixture(scope="module")
def gpu():
    import eao_fusion_amd as E
    assert E.load().eao_device_check() == 0, E.load().eao_last_error()
    return E


@pytest.fixture(scope="module")
def cache():
    """oracle results (and the library's default-path results) of this module, keyed by (what, shape, entry point, arguments): each is computed once"""
    return {}


def _oracle(cache, oracle, name, entry, p=None, tag=""):
    key = ("oracle", name, entry, tag)
    if key not in cache:
        cache[key] = S.run_oracle(oracle, entry, S.shape(name)[0] if p is None else p)
    return cache[key]


def _default(cache, gpu, name, entry):
    """the library's own choice of path for this shape (no switch set)"""
    key = ("library", name, entry)
    if key not in cache:
        cache[key] = S.run_library(gpu, entry, S.shape(name)[0])
    return cache[key]


def _trace_rel(p):
    return CHI2_REL_PLANES if int((p["fixed"] == 0).sum()) > 30 else CHI2_REL      # (band maps: as test_bundle_adjustment_on_sparse_maps; windows: as test_local_ba_parity)


def _hold_updates(r, o, p, what):
    """_check_updates of tests/test_gpu_lm.py (the same bound), with the offending row and its degree in the message"""
    c = S.census(p)
    for key, width, deg in (("poses", 16, c["cam_deg"]), ("points", 3, c["lm_deg"])):
        try:
            _check_updates(r[key], o[key], p[key], key)
        except AssertionError as e:
            _, at = S.displacement(r[key], o[key], p[key])
            row = at // width
            extra = ", %d of them to free cameras" % c["lm_free"][row] if key == "points" else (" (fixed)" if p["fixed"][row] else " (free)")
            raise AssertionError("%s: %s -- worst entry in %s %d, which has %d edges%s" % (what, e, "camera" if key == "poses" else "landmark", row, deg[row], extra)) from None


def _hold(r, o, p, entry, what, rel=None, trace=True):
    """one library result against the oracle's, everything the module promises"""
    if entry == "local_ba":
        assert list(r["iters"]) == list(o["iters"]), "%s: LM schedule %s, the oracle's %s" % (what, list(r["iters"]), list(o["iters"]))
        assert np.array_equal(r["edge_outlier"], o["edge_outlier"]), "%s: %d entries of the outlier table differ" % (what, int((r["edge_outlier"] != o["edge_outlier"]).sum()))
    else:
        assert list(r["iters"]) == [int(o["iters"][0]), 0], "%s: LM schedule %s, the oracle's %s" % (what, list(r["iters"]), list(o["iters"]))
        assert not r["edge_outlier"].any()
    if trace:
        _check_trace(r, o, rel=_trace_rel(p) if rel is None else rel)
    for k in ("poses", "points"):
        assert np.all(np.isfinite(r[k])), "%s: %s not finite" % (what, k)
    _hold_updates(r, o, p, what)
    c = S.census(p)
    still = p["fixed"].astype(bool) | (c["cam_deg"] == 0)
    assert np.array_equal(r["poses"][still].view(np.uint32), o["poses"][still].view(np.uint32)), "%s: a fixed camera or a camera without edges differs from the oracle's" % what
    lone = c["lm_deg"] == 0
    assert np.array_equal(r["points"][lone].view(np.uint32), o["points"][lone].view(np.uint32)), "%s: a landmark without edges differs from the oracle's" % what
    assert np.array_equal(r["points"][lone], p["points"][lone])


# ------------------------------------------------------------------------------------------------ the tile solver (the library's choice up to 30 free keyframes)
@pytest.mark.parametrize("entry", S.ENTRY_POINTS)
@pytest.mark.parametrize("name", WINDOWS)
def test_window_shapes_on_the_tile_solver(gpu, oracle, cache, name, entry):
    p, _ = S.shape(name)
    _hold(_default(cache, gpu, name, entry), _oracle(cache, oracle, name, entry), p, entry, "%s / %s" % (name, entry))


# ------------------------------------------------------------------------------------------------ the map-scale kernels on the same windows
@pytest.mark.parametrize("entry", S.ENTRY_POINTS)
@pytest.mark.parametrize("name", WINDOWS)
def test_window_shapes_on_the_map_scale_kernels(gpu, oracle, cache, name, entry, monkeypatch):
    """EAO_BA_SOLVER=big: identity padding up to the 32-column panels, a single panel (one_free: 6 unknowns), camera blocks that are lambda * I inside the panels, observer
    lists of one entry and of none in k_bal_pair_fill.  The forced run is shown not to be the default run -- on the probe window and on the shape itself."""
    p, _ = S.shape(name)
    default = _default(cache, gpu, name, entry)
    _force_map_scale_path(gpu, monkeypatch)
    r = S.run_library(gpu, entry, p)
    assert _bits_differ(r, default), "%s / %s: the forced run is the default run, bit for bit" % (name, entry)
    _hold(r, _oracle(cache, oracle, name, entry), p, entry, "%s / %s on the map-scale kernels" % (name, entry))


# ------------------------------------------------------------------------------------------------ the batched entry point
def _neighbours():
    return [synth.synth_ba(n_free=5, n_fixed=2, n_points=300, seed=6300 + w) for w in range(9)]


@pytest.mark.parametrize("name", WINDOWS)
def test_window_shape_as_one_window_of_a_batch(gpu, oracle, cache, name):
    """The shape as window 3 of nine: its result is its own single call's (within the batch-vs-single bound) AND the oracle's; the ordinary windows beside it come out as
    their own single calls do -- a per-window bound taken from the odd window (or from its neighbour) would show in either."""
    p, _ = S.shape(name)
    probs = _neighbours()
    probs[3] = p
    if "batch neighbours" not in cache:
        cache["batch neighbours"] = [gpu.Optimizer.LocalBundleAdjustment(q) for q in _neighbours()]
    res = gpu.Optimizer.LocalBundleAdjustmentBatch(probs)
    assert len(res) == 9
    for w, q in enumerate(probs):
        if w != 3:
            _close_result(res[w], cache["batch neighbours"][w], q)
    _close_result(res[3], _default(cache, gpu, name, "local_ba"), p)
    _hold(res[3], _oracle(cache, oracle, name, "local_ba"), p, "local_ba", "%s as window 3 of a batch" % name, trace=False)


def test_all_window_shapes_as_one_batch(gpu, oracle, cache):
    probs = [S.shape(name)[0] for name in WINDOWS]
    res = gpu.Optimizer.LocalBundleAdjustmentBatch(probs)
    rev = gpu.Optimizer.LocalBundleAdjustmentBatch(probs[::-1])[::-1]
    for name, p, r, r2 in zip(WINDOWS, probs, res, rev):
        _close_result(r, _default(cache, gpu, name, "local_ba"), p)
        _hold(r, _oracle(cache, oracle, name, "local_ba"), p, "local_ba", "%s in the batch of all shapes" % name, trace=False)
        assert _same_result(r, r2), "%s: the batch depends on its order" % name


# ------------------------------------------------------------------------------------------------ map scale, the library's own choice beyond 30 free keyframes
@pytest.mark.parametrize("entry", S.ENTRY_POINTS)
@pytest.mark.parametrize("name", MAPS)
def test_map_shapes(gpu, oracle, cache, name, entry):
    """BundleAdjustment (8 iterations, robust and not) and LocalBundleAdjustment (an oversized window: both passes, the outlier pass deactivating edges in the pair lists)"""
    p, _ = S.shape(name)
    r = _default(cache, gpu, name, entry)
    assert r["iters"][0] >= 3
    _hold(r, _oracle(cache, oracle, name, entry), p, entry, "%s / %s" % (name, entry))


@pytest.mark.parametrize("segments", [1, 3, 5])
@pytest.mark.parametrize("name", MAPS)
def test_map_shapes_in_nested_dissection_order(gpu, oracle, cache, name, segments, monkeypatch):
    """EAO_BA_ND = 1 (natural order), 3 and 5 segments forced onto the map: a hub keyframe is covisible with every segment and belongs in every separator; a keyframe without
    edges belongs nowhere.  The forced order is shown to be another order: its result differs from the natural order's in some bit."""
    p, _ = S.shape(name)
    monkeypatch.setenv("EAO_BA_ND", str(segments))
    r = S.run_library(gpu, "ba_plain", p)
    _hold(r, _oracle(cache, oracle, name, "ba_plain"), p, "ba_plain", "%s, EAO_BA_ND=%d" % (name, segments))
    r2 = S.run_library(gpu, "ba_plain", p)          # (the cached plan: bit for bit the same call)
    assert not _bits_differ(r, r2)
    if segments > 1:
        monkeypatch.setenv("EAO_BA_ND", "1")
        assert _bits_differ(r, S.run_library(gpu, "ba_plain", p)), "%s: %d segments give the natural order's result bit for bit -- the order was not forced" % (name, segments)


@pytest.mark.parametrize("name", MAPS)
def test_map_shapes_set_up_on_the_host_crew(gpu, oracle, cache, name, monkeypatch):
    """EAO_BA_SETUP_THREADS = 1 (the serial walks) against 5 and 12 (the chunked validation pass and the camera-range walks on the crew): bit-identical.  thin_map has the
    landmarks without edges in the middle of the list that the chunk boundaries must step over, and cameras whose lists are empty."""
    p, _ = S.shape(name)
    monkeypatch.setenv("EAO_BA_SETUP_THREADS", "1")
    one = S.run_library(gpu, "ba_plain", p)
    _hold(one, _oracle(cache, oracle, name, "ba_plain"), p, "ba_plain", "%s, serial set-up" % name)
    for nt in ("5", "12"):
        monkeypatch.setenv("EAO_BA_SETUP_THREADS", nt)
        r = S.run_library(gpu, "ba_plain", p)
        assert list(r["iters"]) == list(one["iters"]) and not _bits_differ(r, one), "%s: the set-up on %s threads gives another result than the serial one" % (name, nt)


@pytest.mark.parametrize("name", ["hub", "long_tracks_map", "hub_last"])
def test_map_shapes_with_four_wave_pairs(gpu, oracle, cache, name, monkeypatch):
    """EAO_BA_PAIR_LONG=48 (read per call): the hub's pairs -- its diagonal pair holds every landmark it sees -- take the four-wave variant of the assembly, the band's
    short pairs the one-wave kernel, in one call."""
    p, _ = S.shape(name)
    free = p["fixed"][p["edge_cam"]] == 0
    assert np.bincount(p["edge_cam"][free]).max() > 48          # (a camera's diagonal pair has one entry per landmark it observes: longer than the forced limit)
    monkeypatch.setenv("EAO_BA_PAIR_LONG", "48")
    r = S.run_library(gpu, "ba_plain", p)
    _hold(r, _oracle(cache, oracle, name, "ba_plain"), p, "ba_plain", "%s, four-wave pairs" % name)


# ------------------------------------------------------------------------------------------------ map planes beside the irregular point graph
def _with_planes(name, lone_edge):
    """Four map planes on the shape; plane edges only on cameras that have point edges -- and, with lone_edge, ONE plane edge on the free camera that has none (its block
    is that one edge's 6 x 6 of rank 3, plus lambda)."""
    p, _ = S.shape(name)
    q = synth.add_ba_planes(p, n_planes=4, seed=7100)
    deg = S.census(p)["cam_deg"]
    keep = deg[q["pedge_cam"]] > 0
    if lone_edge:
        empty = np.flatnonzero((deg == 0) & (p["fixed"] == 0))
        mine = np.flatnonzero(q["pedge_cam"] == empty[0])
        assert len(mine), "no plane of this draw is seen by camera %d" % empty[0]
        keep[mine[0]] = True
    for k in ("pedge_plane", "pedge_cam", "pedge_obs"):
        q[k] = np.ascontiguousarray(q[k][keep])
    return q


@pytest.mark.parametrize("lone_edge", [False, True])
@pytest.mark.parametrize("name", ["skewed", "thin_map"])
def test_shapes_with_map_planes(gpu, oracle, cache, name, lone_edge):
    q = _with_planes(name, lone_edge)
    its = S.ba_iterations(q)
    r, o = gpu.Optimizer.BundleAdjustment(q, its, bRobust=True), oracle.bundle_adjustment(q, its, True)
    what = "%s with planes%s" % (name, ", one plane edge on the camera without point edges" if lone_edge else "")
    assert list(r["iters"]) == [int(o["iters"][0]), 0], what
    _check_trace(r, o, rel=CHI2_REL_PLANES)
    _hold_updates(r, o, q, what)
    _check_updates(r["planes"], o["planes"], q["planes"], "planes")
    assert np.all(np.isfinite(r["poses"])) and np.all(np.isfinite(r["points"])) and np.all(np.isfinite(r["planes"]))
    f = q["fixed"].astype(bool)
    assert np.array_equal(r["poses"][f], o["poses"][f])
    if not lone_edge:
        still = S.census(q)["cam_deg"] == 0
        assert still.any() and np.array_equal(r["poses"][still].view(np.uint32), o["poses"][still].view(np.uint32)), "%s: a camera without any edge differs from the oracle's" % what


# ------------------------------------------------------------------------------------------------ edge order
@pytest.mark.parametrize("name", ["single_observer", "thin_map"])
def test_shapes_with_shuffled_edge_lists(gpu, oracle, cache, name):
    """The general set-up paths (an edge list that is NOT grouped by landmark) on graphs with one-entry and empty lists: against the oracle on the same shuffled problem,
    and -- through the permutation -- the outlier table of the ordered problem."""
    p, _ = S.shape(name)
    q, perm = _shuffle_edges(p, 5800)
    r, o = S.run_library(gpu, "local_ba", q), _oracle(cache, oracle, name, "local_ba", p=q, tag="shuffled")
    _hold(r, o, q, "local_ba", "%s, shuffled" % name)
    assert np.array_equal(r["edge_outlier"], _default(cache, gpu, name, "local_ba")["edge_outlier"][perm])
