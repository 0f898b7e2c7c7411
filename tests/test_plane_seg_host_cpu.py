"""csrc/plane_seg_internal.h, the host's share of eao_plane_seg_run, as the stand-alone program tools/plane_segmentation_walk.cpp built with
-fsanitize=address,undefined: it must print the yardstick's bits (tests/plane_segmentation_reference.py) on every scene of at most 160 x 120 and on the VGA room,
and its `cluster` command must order hand-built ties as the yardstick does.  Nothing here is loaded into Python; no GPU."""
import numpy as np
import pytest

import plane_segmentation_reference as R
import plane_segmentation_scenes as SC
import plane_segmentation_walk as WALK

SCENES = SC.scenes()


@pytest.fixture(scope="module")
def walk():
    return WALK.build(True)


@pytest.mark.parametrize("name", list(SCENES))
def test_walk_prints_the_yardsticks_bits(walk, name):
    s = SCENES[name]
    want = R.script_text(R.run(s["cfg"], s["depth"], vectorised=name not in SC.SMALL))
    got = WALK.run(walk, "script", R.scene_bytes(s["cfg"], s["depth"]))
    if got != want:
        g, w = got.split("\n"), want.split("\n")
        first = next((i for i, (a, b) in enumerate(zip(g, w)) if a != b), min(len(g), len(w)))
        pytest.fail("%s: line %d of %d / %d differs:\n got  %s\n want %s" % (name, first, len(g), len(w), g[first][:200] if first < len(g) else "", w[first][:200] if first < len(w) else ""))


def _patch(x0, y0, z, n=10, tilt=0.0):
    """n x n points of the plane z + tilt * x, 1 cm apart"""
    return [(x0 + 0.01 * i, y0 + 0.01 * j, z + tilt * (x0 + 0.01 * i)) for j in range(n) for i in range(n)]


def _both(walk, nodes, edges, min_support):
    c = R.default_cfg(min_support=min_support)
    res = R.cluster_graph(c, nodes, edges)
    assert WALK.run(walk, "cluster", R.graph_text(nodes, edges, min_support)) == R.cluster_text(res)
    return res


def test_cluster_equal_mse_pops_in_creation_sequence(walk):
    # two disconnected nodes with the same sums (hence the same mse) and a third: equal mse leaves the queue in creation sequence, so the extraction order, which
    # the stable size sort keeps for equal N, is 0 before 1 whichever rid they carry
    s = R.sums_of(_patch(0.0, 0.0, 1.0, tilt=0.1))
    for rids in ((5, 3, 9), (3, 5, 9)):
        nodes = [(rids[0], 100, s), (rids[1], 100, s), (rids[2], 100, R.sums_of(_patch(0.5, 0.0, 1.2)))]
        steps, merges, extracted = _both(walk, nodes, [], 100)
        assert merges == [] and steps == 3
        same = [e for e in extracted if e[3] == extracted[[e[0] for e in extracted].index(0)][3]]
        assert [e[0] for e in same] == [0, 1]


def test_cluster_equal_N_keeps_extraction_order(walk):
    # three separate planes of equal N and different mse: extracted by ascending mse, and the size sort (stable, equal N) leaves that order
    nodes = [(0, 100, R.sums_of(_patch(0.0, 0.0, 1.0, tilt=0.3))), (1, 100, R.sums_of(_patch(0.0, 0.0, 1.0))), (2, 100, R.sums_of(_patch(0.0, 0.0, 2.0, tilt=0.1)))]
    steps, merges, extracted = _both(walk, nodes, [], 100)
    assert merges == [] and [e[3] for e in extracted] == sorted(e[3] for e in extracted)
    # a larger one comes first whatever its mse
    nodes.append((3, 200, R.sums_of(_patch(0.0, 0.0, 1.5, tilt=0.2) + _patch(0.1, 0.0, 1.5, tilt=0.2))))
    _, _, extracted = _both(walk, nodes, [], 100)
    assert extracted[0][0] == 3 and [e[3] for e in extracted[1:]] == sorted(e[3] for e in extracted[1:])


@pytest.mark.parametrize("order", [(0, 1, 2), (0, 2, 1)])
def test_cluster_neighbour_set_in_both_creation_orders(walk, order):
    # a centre block with a left and a right neighbour that mirror each other: both merges have the same statistics up to the sign of x, hence (here) the same
    # mse, and `cand_merge->N < merge->mse` (200 < mse) is false, so the neighbour that was CREATED first wins, not the one with the smaller rid
    centre = _patch(-0.045, 0.0, 1.0)
    left, right = _patch(-0.145, 0.0, 1.0), _patch(0.055, 0.0, 1.0)
    blocks = [(10, 100, R.sums_of(centre)), (11, 100, R.sums_of(left)), (12, 100, R.sums_of(right))]
    nodes = [blocks[k] for k in order]
    pos = {k: i for i, k in enumerate(order)}
    edges = [(pos[0], pos[1]), (pos[0], pos[2])]
    c = R.default_cfg(min_support=100)
    ml = R.fit([a + b for a, b in zip(blocks[0][2], blocks[1][2])], 200, R.eig3_jacobi)[2]
    mr = R.fit([a + b for a, b in zip(blocks[0][2], blocks[2][2])], 200, R.eig3_jacobi)[2]
    steps, merges, extracted = _both(walk, nodes, edges, 100)
    assert len(merges) == 2 and extracted[0][2] == 300 and len(extracted) == 1
    first = [nodes[i][0] for i in range(3) if nodes[i][0] in merges[0][:2]]
    if ml == mr:      # the tie this scene is for: the flat patches give exactly 0 on both sides
        # whoever is popped first (equal mse: creation sequence) merges with its first-created neighbour
        popped = nodes[0][0]
        assert merges[0][0] == popped
        nbs = sorted(pos[k] for k in ((1, 2) if popped == 10 else (0,)))
        assert merges[0][1] == nodes[nbs[0]][0]
    assert set(first) <= {10, 11, 12}
