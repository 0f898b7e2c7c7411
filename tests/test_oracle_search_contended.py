"""CPU: tests/test_oracle_search.py's brute-force replays of the remaining guided searches (BoW x2, triangulation, initialisation, Fuse,
Sim3, the keyframe projections) on contended keyframes (synth.synth_search_scene_contended: landmarks created twice, corners detected at
two octaves with equal or nearly equal descriptors), where a match claimed by an earlier query changes what a later one gets."""
import pytest

from eao_fusion_amd import synth
from test_oracle_search import *  # noqa: F401,F403  (the same tests, collected here against the scene below)


@pytest.fixture(scope="module", params=[dict(n=220, seed=8100, n_nodes=25), dict(n=300, seed=8102, n_nodes=12, dup_points=0.4, dup_keypoints=0.4)],
                ids=["dup-20pct", "dup-40pct-coarse-vocabulary"])
def scene(request):
    return synth.synth_search_scene_contended(**request.param)
