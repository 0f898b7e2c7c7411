"""The yardstick of the plane segmentation (tests/plane_segmentation_reference.py) held to itself, without a device: every scene of
tests/plane_segmentation_scenes.py reaches the branch it claims; both eigen-solve variants (the chosen Jacobi and numpy.linalg.eigh) give the same block flags,
merge sequence, membership image and kept set on every scene; the vectorised forms equal the literal loops; the literals are the reference text's
(tests/golden/plane_segmentation_constants.json, held to that text by tests/test_reference_literals.py); the golden files are what the yardstick computes."""
import math
import os
import re
import sys

import numpy as np
import pytest

import plane_segmentation_reference as R
import plane_segmentation_scenes as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from reference_literals import literals  # noqa: E402

SCENES = SC.scenes()
_runs = {}


def run(name, eig="jacobi"):
    if (name, eig) not in _runs:
        s = SCENES[name]
        _runs[(name, eig)] = R.run(s["cfg"], s["depth"], eig=eig, vectorised=name not in SC.SMALL)
    return _runs[(name, eig)]


def _on_face(scene, r, pixels):
    """every listed pixel is a member of plane 0, its float z times the float 20 is an exact integer (the product is exact, so floor() decides ON the face), the
    pixel lands in the upper cell, and the cell below it is occupied too (the face separates two voxels of the cloud)"""
    c, depth = scene["cfg"], scene["depth"]
    inv = np.float32(1.0) / c.leaf
    flat = r["membership"].reshape(-1)
    pix = np.flatnonzero(flat == 0)
    pts = R.plane_points(c, depth, pix, False)
    zk = np.floor(pts[:, 2] * inv).astype(np.int64)
    ok = True
    for p in pixels:
        k = int(np.searchsorted(pix, p))
        z = pts[k, 2]
        prod = np.float32(z * inv)
        ok = ok and flat[p] == 0 and float(prod) == float(z) * float(inv) and float(prod) == math.floor(float(prod)) and zk[k] == int(prod) and (zk == int(prod) - 1).any()
    return ok


@pytest.mark.parametrize("name", list(SCENES))
def test_scene_reaches_what_it_claims(name):
    r, claims = run(name), SCENES[name]["claims"]
    sg = r["seg"]
    flags = np.array([b["flag"] for b in r["records"]])
    kept = [p["kept"] for p in r["planes"]]
    assert not any(p["flipped"] for p in r["planes"])      # coef[3] < 0 before the flip is unreachable: d = -(n . c) >= 0 by the fit's own rule
    checks = dict(
        min_planes=lambda v: len(kept) >= v, n_planes=lambda v: len(kept) == v, n_kept=lambda v: sum(kept) == v, n_first=lambda v: len(sg.old) == v,
        stopped=lambda v: sg.n_stopped > 0, retaken=lambda v: sg.n_retaken > 0, connects=lambda v: len(sg.connects) > 0 and len(sg.merges) > sg.n_merges_first,
        eroded_planes=lambda v: not all(sg.valid_plane), missing_blocks=lambda v: np.flatnonzero(flags & 1).tolist() == v,
        discontinuity_blocks=lambda v: np.flatnonzero(flags & 2).tolist() == v, n_voxels=lambda v: [len(p["cloud"]) for p in r["planes"]] == [v],
        n_voxels_min=lambda v: all(len(p["cloud"]) >= v for p in r["planes"]),
        on_face=lambda v: _on_face(SCENES[name], r, v),
        ragged_claimed=lambda v: bool((r["membership"][:, SCENES[name]["cfg"].width - SCENES[name]["cfg"].width % 10:] >= 0).any()) == v)
    for k, v in claims.items():
        assert checks[k](v), (name, k, v)
    if name == "eroded":
        assert sg.valid_plane == [False] and sg.old[0].N >= SCENES[name]["cfg"].min_support
    if name == "limits":      # 0.2f and 4.0f and the floats inside are valid; the floats outside, 0, NaN, inf and a negative depth are not
        assert (flags[[0, 1, 3, 4]] & 1 == 0).all() and (flags[[2, 5, 6, 7, 8, 9]] & 1 == 1).all()
    if name == "tdz_at":
        assert (flags == 0).all()


@pytest.mark.parametrize("name", list(SCENES))
def test_both_eigen_solves_agree_on_every_decision(name):
    a, b = run(name, "jacobi"), run(name, "eigh")
    assert [x["flag"] for x in a["records"]] == [x["flag"] for x in b["records"]]
    assert a["merges"] == b["merges"]
    assert np.array_equal(a["membership"], b["membership"])
    assert [p["kept"] for p in a["planes"]] == [p["kept"] for p in b["planes"]]
    # the figure DESIGN.md section 4k records (no gate rests on it): the largest normal angle and relative mse difference between the variants
    ang, rel = 0.0, 0.0
    for p, q in zip(a["planes"], b["planes"]):
        dot = min(1.0, abs(sum(x * y for x, y in zip(p["normal"], q["normal"]))))
        ang = max(ang, math.acos(dot))
        if q["mse"] != 0:
            rel = max(rel, abs(p["mse"] - q["mse"]) / abs(q["mse"]))
    print("%s: planes' largest normal angle %.3e rad, relative mse difference %.3e" % (name, ang, rel))


def test_jacobi_is_an_eigen_decomposition():
    rs = np.random.RandomState(3)
    for k in range(50):
        A = rs.standard_normal((3, 3)) * 10.0 ** rs.randint(-6, 3)
        K = (A @ A.T).tolist()
        if k == 0:
            K = [[2.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 3.0]]      # nothing to rotate: only the ordering acts
        l, V = R.eig3_jacobi(K)
        V = np.array(V)
        assert l[0] <= l[1] <= l[2]
        scale = max(abs(np.array(K)).max(), 1e-300)
        assert np.abs(V @ np.diag(l) @ V.T - np.array(K)).max() <= 1e-13 * scale and np.abs(V.T @ V - np.eye(3)).max() <= 1e-14
        assert np.abs(np.array(l) - np.linalg.eigvalsh(np.array(K))).max() <= 1e-13 * scale


@pytest.mark.parametrize("name", SC.SMALL)
def test_vectorised_forms_equal_the_literal_loops(name):
    s, r = SCENES[name], run(name)
    c, depth = s["cfg"], s["depth"]
    assert R.records_array(R.block_records_vec(c, depth)).tobytes() == R.records_array(r["records"]).tobytes()
    flat = r["membership"].reshape(-1)
    for j, p in enumerate(r["planes"]):
        pix = np.flatnonzero(flat == j)
        lit, vec = R.plane_points(c, depth, pix, False), R.plane_points(c, depth, pix, True)
        assert lit.tobytes() == vec.tobytes()
        assert R.voxel_centroids_vec(lit, c.leaf).tobytes() == p["cloud"].tobytes() == R.voxel_centroids(lit, c.leaf).tobytes()


def test_voxel_grid_by_hand():
    inv = np.float32(1.0) / np.float32(0.05)
    assert inv == np.float32(20.0)
    # 0.25f * 20 is exactly 5: the point lies ON the face between cells 4 and 5 and belongs to 5
    pts = np.array([[0.25, 0.0, 1.0], [0.2499, 0.0, 1.0], [0.26, 0.01, 1.01], [0.01, 0.0, 1.0]], np.float32)
    got = R.voxel_centroids(pts, np.float32(0.05))
    assert len(got) == 3      # cells 0, 4 and 5 along x
    assert got[2].tobytes() == ((pts[0] + pts[2]) / np.float32(2)).tobytes() and got[1].tobytes() == pts[1].tobytes() and got[0].tobytes() == pts[3].tobytes()
    # the sum inside a voxel runs in ascending point index: a large value first swallows the small ones, last it does not
    big = np.array([[3.0e7, 0, 0]] + [[1.0, 0, 0]] * 4, np.float32)
    a = R.voxel_centroids(big, np.float32(1.0e9))
    b = R.voxel_centroids(big[::-1].copy(), np.float32(1.0e9))
    assert a[0, 0] == np.float32(3.0e7) / np.float32(5) and b[0, 0] == np.float32(3.0e7 + 4) / np.float32(5) and a[0, 0] != b[0, 0]
    assert R.voxel_centroids_vec(big, np.float32(1.0e9)).tobytes() == a.tobytes()
    with pytest.raises(ValueError):
        R.voxel_centroids(np.array([[0, 0, 0], [1e4, 1e4, 1e4]], np.float32), np.float32(0.001))


def test_literals_match_the_reference_text():
    lit = literals("plane_segmentation")      # (held to the reference text by tests/test_reference_literals.py)
    c = R.default_cfg()
    assert (c.depth_max, c.depth_min, float(c.leaf)) == (float(lit["DEPTH_MAX"]), float(lit["DEPTH_MIN"]), float(np.float32(float(lit["LEAF"]))))
    assert (R.SEEN_DIST, R.SEEN_ANGLE) == (float(lit["SEEN_DIST"]), float(lit["SEEN_ANGLE"]))
    assert (c.max_step, c.min_support, c.window) == (int(lit["MAX_STEP"]), int(lit["MIN_SUPPORT"]), int(lit["WINDOW"])) and lit["WINDOW_HEIGHT"] == lit["WINDOW"]
    assert (R.TRAIL_STOP, R.DIST_FACTOR, R.DIST_EPS) == (int(lit["TRAIL_STOP"]), int(lit["DIST_FACTOR"]), float(lit["DIST_EPS"]))
    assert (c.depth_sigma, c.std_tol_init, c.std_tol_merge, c.z_near, c.z_far) == tuple(float(lit[k]) for k in ("DEPTH_SIGMA", "STD_TOL_INIT", "STD_TOL_MERGE", "Z_NEAR", "Z_FAR"))
    assert (c.angle_near, c.angle_far) == (float(lit["ANGLE_NEAR_DEG"]) * math.pi / 180.0, float(lit["ANGLE_FAR_DEG"]) * math.pi / 180.0)
    assert c.similarity_merge == math.cos(float(lit["SIMILARITY_MERGE_DEG"]) * math.pi / 180.0)
    assert c.similarity_refine == math.cos(float(lit["SIMILARITY_REFINE_DEG"]) * math.pi / 180.0)
    assert (c.depth_alpha, c.depth_change_tol) == (float(lit["DEPTH_ALPHA"]), float(lit["DEPTH_CHANGE_TOL"]))
    # after clipping T_ang(P_INIT) is one value for every depth in metres: the cosine of (about) fifteen degrees
    assert R.t_ang_init(c, 0.2) == R.t_ang_init(c, 4.0) and abs(R.t_ang_init(c, 1.0) - math.cos(math.radians(15))) < 1e-15
    internal = open(os.path.join(ROOT, "eao_fusion_amd", "csrc", "plane_seg_internal.h")).read()
    assert "kTrailStop = %s;" % lit["TRAIL_STOP"] in internal and "kDistFactor = %s, kDistEps = %s;" % (lit["DIST_FACTOR"], lit["DIST_EPS"]) in internal
    assert "kSeenDist = %s, kSeenAngle = %s;" % (lit["SEEN_DIST"], lit["SEEN_ANGLE"]) in internal and "kJacobiSweeps = %d;" % R.JACOBI_SWEEPS in internal
    hip = open(os.path.join(ROOT, "eao_fusion_amd", "csrc", "plane_seg.hip")).read()
    for text in ("c->window = %s; c->min_support = %s; c->max_step = %s;" % (lit["WINDOW"], lit["MIN_SUPPORT"], lit["MAX_STEP"]),
                 "c->depth_min = %s; c->depth_max = %s; c->leaf = %sf;" % (lit["DEPTH_MIN"], lit["DEPTH_MAX"], lit["LEAF"]),
                 "c->depth_sigma = %s; c->std_tol_init = %s; c->std_tol_merge = %s;" % (lit["DEPTH_SIGMA"], lit["STD_TOL_INIT"], lit["STD_TOL_MERGE"]),
                 "c->z_near = %s; c->z_far = %s;" % (lit["Z_NEAR"], lit["Z_FAR"]),
                 "c->angle_near = (%s) * M_PI / 180.0; c->angle_far = (%s) * M_PI / 180.0;" % (lit["ANGLE_NEAR_DEG"], lit["ANGLE_FAR_DEG"]),
                 "c->similarity_merge = std::cos((%s) * M_PI / 180.0);" % lit["SIMILARITY_MERGE_DEG"],
                 "c->similarity_refine = std::cos((%s) * M_PI / 180.0);" % lit["SIMILARITY_REFINE_DEG"],
                 "c->depth_alpha = %s; c->depth_change_tol = %s;" % (lit["DEPTH_ALPHA"], lit["DEPTH_CHANGE_TOL"])):
        assert text in hip, text
    hdr = open(os.path.join(ROOT, "include", "eao_fusion.h")).read()
    for sym in ("eao_plane_seg_cfg_default", "eao_plane_seg_create", "eao_plane_seg_run", "eao_plane_seg_planes", "eao_plane_seg_cloud", "eao_plane_seg_membership",
                "eao_plane_seg_blocks", "eao_plane_map_add_from_seg", "eao_plane_map_update_boundary_from_seg"):
        assert re.search(r"\b%s\s*\(" % sym, hdr), sym
    assert "src/Frame.cc:381-460" in hdr and "AHCPlaneFitter.hpp" in hdr
    import ctypes
    from eao_fusion_amd import _lib
    assert ctypes.sizeof(_lib.PlaneSegCfg) == 144 and ctypes.sizeof(_lib.PlaneSegPlane) == 104


@pytest.mark.parametrize("name", list(SCENES))
def test_golden_files_are_the_yardsticks(name):
    z = np.load(os.path.join(ROOT, "tests", "golden", "plane_segmentation", name + ".npz"))
    a = R.result_arrays(run(name))
    if name not in SC.SMALL:
        for k in R.BULK:
            a["sha256_" + k] = R.digest(a.pop(k))
    assert sorted(z.files) == sorted(a)
    for k in a:
        assert z[k].dtype == a[k].dtype and z[k].tobytes() == a[k].tobytes(), k
