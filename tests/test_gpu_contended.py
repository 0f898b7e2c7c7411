"""GPU parity on contended scenes (synth.synth_tracking_contended / synth_search_scene_contended): duplicated landmarks, corners detected at two
octaves, exact distance ties, chains of map points each wanting its predecessor's keypoint, rotation-histogram ties, prior matches on contested
keypoints.  On these scenes the greedy order of the guided searches decides a large share of the matches (tests/contention.py measures it, the CPU
suite holds the oracle to a brute force there), so the device's emulations of that order -- the host replays, the tracker's assignment rounds with
their single-wave tail, the vocabulary-node kernel's (distance, position) keys -- are held to the oracle where they can be wrong.  Integer tables
bit for bit, the pose within the LM bound."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import contention
from eao_fusion_amd import synth
from test_gpu_track import KP, _OracleCalls, _ProductCalls, _bow_case, _chain, _chain_bow, _chain_motion, _device_buffers, _pose_close, _tracker
from test_oracle_match import CONTENDED

pytestmark = pytest.mark.gpu
LDS_LISTS = 28 * 1024          # csrc/track.hip kLdsLists: candidate-list entries the assignment step keeps in LDS
ASSIGN_THREADS = 1024          # csrc/track.hip kAssignThreads: PER = 4 / 8 / 16 points per thread up to 4096 / 8192 / 16384 points
TAIL = 64                      # the last undecided points go to one wave


@pytest.fixture(scope="module")
def gpu():
    import eao_fusion_amd as E
    assert E.load().eao_device_check() == 0, E.load().eao_last_error()
    return E


# ---- host-array searches (eao_search_by_projection_points / _frames) ------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["dups-chains-ties", "long-chains"])
@pytest.mark.parametrize("th", [1.0, 3.0])
def test_points_search_contended(gpu, oracle, name, th):
    cur, last, mps = synth.synth_tracking_contended(**CONTENDED[name])
    for ratio in (0.8, 0.6):
        nm, got = gpu.ORBmatcher(ratio, True).SearchByProjectionPoints(cur, mps, th)
        onm, ref = oracle.search_by_projection_points(cur, mps, th, ratio)
        assert nm == onm and np.array_equal(got, ref), ratio
    assert nm > 0.5 * len(mps["level"])


@pytest.mark.parametrize("name", list(CONTENDED))
@pytest.mark.parametrize("mono", [False, True])
def test_frames_search_contended(gpu, oracle, name, mono):
    cur, last, _ = synth.synth_tracking_contended(**CONTENDED[name])
    for th, check in ((7.0, True), (15.0, True), (7.0, False)):
        nm, got = gpu.ORBmatcher(0.9, check).SearchByProjectionFrames(cur, last, th, mono)
        onm, ref = oracle.search_by_projection_frames(cur, last, th, mono, check)
        assert nm == onm and np.array_equal(got, ref), (th, check)
    assert nm > 20


# ---- the tracker chain --------------------------------------------------------------------------------------------------------------------------

def _scene(gen_kw, prior_on_contested=True, seed=0):
    """test_gpu_track._scene's frame / local map / depth image from a contended tracking scene: a keypoint's depth is that of the landmark its right
    coordinate was drawn from (0 where the scene says monocular), and every keypoint the scene marks occupied becomes a prior match (to a map point the
    prior then takes out of the search) -- those are contested keypoints of the duplicate groups."""
    cur, last, _ = synth.synth_tracking_contended(**gen_kw)
    rng = np.random.default_rng(gen_kw.get("seed", 0) + 11 + seed)
    N = len(cur["kp_x"])
    ok = (cur["kp_x"] >= 1) & (cur["kp_x"] < 638) & (cur["kp_y"] >= 1) & (cur["kp_y"] < 478)
    kx, ky = np.where(ok, cur["kp_x"], 5.5).astype(np.float32), np.where(ok, cur["kp_y"], 7.25).astype(np.float32)
    kps = np.zeros(N, KP)
    kps["x"], kps["y"], kps["angle"], kps["octave"], kps["size"], kps["class_id"] = kx, ky, cur["kp_angle"], cur["kp_octave"], 31, -1
    depth = rng.uniform(1.5, 6.0, (480, 640)).astype(np.float32)
    ur = cur["u_right"]
    z = np.where(ur > 0, cur["mbf"] / np.maximum(kx - ur, 1e-3), 0.0).astype(np.float32)
    depth[ky.astype(int), kx.astype(int)] = z
    Xw = last["Xw"]
    M = len(Xw)
    dist = np.linalg.norm(Xw, axis=1).astype(np.float32)
    normal = (Xw / np.maximum(dist, 1e-3)[:, None]).astype(np.float32)
    pts = dict(active=np.ones(M, np.uint8), Xw=Xw, normal=normal, min_dist_inv=(0.6 * dist).astype(np.float32), max_dist_inv=(1.7 * dist).astype(np.float32),
               max_dist=(dist * np.float32(1.2) ** (last["octave"] - 0.5)).astype(np.float32), descriptors=last["descriptors"])
    prior = None
    occ = np.nonzero(cur["occupied"])[0]
    if prior_on_contested and len(occ):
        prior = np.full(N, -1, np.int32)
        prior[occ] = rng.choice(M, len(occ), replace=False)
    return cur, last, kps, np.ascontiguousarray(cur["descriptors"]), depth, pts, prior


def _run_local_map(oracle, gen_kw, th, nnratio=0.8, prior_on_contested=True):
    cur, last, kps, desc, depth, pts, prior = _scene(gen_kw, prior_on_contested)
    want = _chain(_OracleCalls(oracle), cur, kps, desc, depth, pts, prior, th, nnratio)
    N, M = len(kps), len(pts["Xw"])
    cap = 2048 if N <= 2048 else 4096
    trk = _tracker(cur, cap, max(2048, M))
    trk.set_local_map(pts)
    d_kps, d_desc, d_n, d_depth = _device_buffers(kps, desc, depth, cap)
    got = trk.track_local_map(d_kps.data_ptr(), d_desc.data_ptr(), d_n.data_ptr(), d_depth.data_ptr(), 640, 640, 480, cur["Tcw"], prior, th, nnratio,
                              torch.cuda.current_stream().cuda_stream)
    return cur, kps, pts, prior, want, got


def _same_chain(got, want, cur):
    assert np.array_equal(got["u_right"], want["u_right"]) and np.array_equal(got["depth"], want["depth"])
    assert got["n_matches"] == want["n_matches"]
    assert np.array_equal(got["kp_map_point"], want["kp_map_point"]), np.nonzero(got["kp_map_point"] != want["kp_map_point"])[0][:8]
    assert got["n_edges"] == want["n_edges"] and got["n_inliers"] == want["n_inliers"]
    assert np.array_equal(got["kp_outlier"], want["kp_outlier"])
    ok, err, upd = _pose_close(got["Tcw"], want["Tcw"], cur["Tcw"])
    assert ok, "pose: |gpu - oracle| %.3e vs update %.3e" % (err, upd)


LOCAL_MAP_CASES = {
    # name: (generator arguments, th, nnratio, expected path: lists in LDS?, PER)
    "lds-per4": (dict(CONTENDED["dups-chains-ties"]), 1.0, 0.8, True, 4),
    "lds-per4-chains-tail": (dict(CONTENDED["long-chains"]), 3.0, 0.8, True, 4),
    "lds-per4-ratio06": (dict(CONTENDED["dups-chains-ties"], seed=7610), 3.0, 0.6, True, 4),
    "lds-per8": (dict(seed=7611, extra_points=4000), 3.0, 0.8, True, 8),
    "global-per16": (dict(seed=7612, n=1200, dup_groups=60, chains=(150,), ratio_chains=(80,), extra_points=7600), 8.0, 0.8, False, 16),
}


@pytest.mark.parametrize("name", list(LOCAL_MAP_CASES))
def test_local_map_contended(oracle, gpu, name):
    """eao_tracker_track_local_map against the oracle chain on contended scenes, over the assignment step's paths: candidate lists in LDS and in global
    memory (beyond 28 672 entries), 4, 8 and 16 points per thread (local maps beyond 4096 and 8192 points), chains of 120-200 dependent points (one round
    per link: the single-wave tail takes over the last 64), prior matches on contested keypoints.  Which path ran is asserted from sizes."""
    gen_kw, th, nnratio, lds, per = LOCAL_MAP_CASES[name]
    cur, kps, pts, prior, want, got = _run_local_map(oracle, gen_kw, th, nnratio)
    frame, mps = want["search_args"]
    total = sum(len(c) for c in contention.points_candidates(frame, mps, th))
    M = len(pts["Xw"])
    assert (total <= LDS_LISTS) == lds, total
    assert M <= per * ASSIGN_THREADS and (per == 4 or M > per // 2 * ASSIGN_THREADS), M
    chains = gen_kw.get("chains", (120,)) + gen_kw.get("ratio_chains", (60,))
    assert max(chains) > TAIL                                        # a chain longer than the tail: both the workgroup rounds and the wave's run
    assert prior is not None and (prior >= 0).sum() > 0
    meter = contention.meter_points(frame, mps, th, nnratio)
    print("contention chain %s: %s, candidates %d, map points %d" % (name, meter, total, M))
    assert meter["differ"] >= 0.1 * meter["matched"] and meter["differ_ratio"] > 0, meter
    _same_chain(got, want, cur)


def test_local_map_contended_equals_host_hops(oracle, gpu):
    """The same chain through the product's host-hop calls (the host replay of the points search): the device chain's tables and pose bit for bit."""
    cur, kps, pts, prior, want, got = _run_local_map(oracle, CONTENDED["long-chains"], 3.0)
    cur, last, kps, desc, depth, pts, prior = _scene(CONTENDED["long-chains"])
    hop = _chain(_ProductCalls(gpu), cur, kps, desc, depth, pts, prior, 3.0, 0.8)
    for k in ("n_matches", "n_edges", "n_inliers"):
        assert hop[k] == got[k] == want[k], k
    assert np.array_equal(hop["kp_map_point"], got["kp_map_point"]) and np.array_equal(hop["kp_outlier"], got["kp_outlier"])
    assert np.array_equal(hop["Tcw"], got["Tcw"])


@pytest.mark.parametrize("name", ["dups-chains-ties", "long-chains", "hist-equal", "hist-contended"])
@pytest.mark.parametrize("mono", [False, True])
def test_motion_model_contended(oracle, gpu, name, mono):
    """eao_tracker_track_with_motion_model (the assignment rounds without a ratio test, then the rotation filter) against the oracle chain on contended
    scenes and on histograms whose kept bins are decided by equal counts, by a count of exactly a tenth of the fullest bin and by angles half-way
    between bins."""
    cur, last, kps, desc, depth, pts, _ = _scene(CONTENDED[name], False)
    if mono:
        depth = np.zeros_like(depth)
    th = 7.0
    want = _chain_motion(_OracleCalls(oracle), lambda f, l, t, m: oracle.search_by_projection_frames(f, l, t, m, True), cur, kps, desc, depth, last, th, mono, True)
    cap = 2048
    d_kps, d_desc, d_n, d_depth = _device_buffers(kps, desc, depth, cap)
    trk = _tracker(cur, cap, 2048)
    got = trk.track_with_motion_model(d_kps.data_ptr(), d_desc.data_ptr(), d_n.data_ptr(), d_depth.data_ptr(), 640, 640, 480, cur["Tcw"], last, th, mono, True, True,
                                      torch.cuda.current_stream().cuda_stream)
    _same_chain(got, want, cur)
    assert want["n_matches"] > 20


@pytest.mark.parametrize("case", [dict(seed=7620, n=800, n_nodes=60), dict(seed=7621, n=600, n_nodes=9), dict(seed=7622, n=900, n_nodes=1, ratio=0.9)])
def test_reference_keyframe_stage_contended(oracle, gpu, case):
    """eao_tracker_track_reference_keyframe (SearchByBoW(KeyFrame, Frame) on the device) against the oracle chain on a contended keyframe pair:
    duplicated corners (equal or near-equal descriptors, one node) on both sides."""
    sc, cam, kps, desc, depth, kf = _bow_case(case["seed"], case["n"], case["n_nodes"], gen=synth.synth_search_scene_contended)
    ratio = case.get("ratio", 0.7)
    want = _chain_bow(oracle, cam, kps, desc, depth, kf, sc["fv2"], ratio, True, True)
    cap = 2048
    d_kps, d_desc, d_n, d_depth = _device_buffers(kps, desc, depth, cap)
    trk = _tracker(cam, cap, 2048)
    got = trk.track_reference_keyframe(d_kps.data_ptr(), d_desc.data_ptr(), d_n.data_ptr(), d_depth.data_ptr(), 640, 640, 480, cam["Tcw"], kf, sc["fv2"], ratio, True, True,
                                       torch.cuda.current_stream().cuda_stream)
    _same_chain(got, want, cam)
    assert want["n_matches"] >= 15


def test_contended_chain_with_every_lister_counted():
    """EAO_TRACK_ALL_LISTERS=1 (every lister a competitor, no TH_HIGH shortcut in the finalisation test): the same semantics, so the contended sweep
    of the chain must give the oracle's tables too.  In a process of its own: the switch is read once per process."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, EAO_TRACK_ALL_LISTERS="1")
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "sweep_track.py"), "23", "6", "contended"], env=env, cwd=root, capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "tracker sweep: 6 frames, 0 mismatches" in out.stdout, out.stdout[-2000:]
