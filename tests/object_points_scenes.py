"""Seeded scenes of the object layer's point-list update (tests/object_points_reference.py is their yardstick).  A scene is a desc (the keys of
eao_object_points_desc, what is missing is zero) with `claims`: the outputs the scene is there for, which tests/test_object_points_reference_cpu.py holds the
yardstick to.  A claim is a record field, an output array, or `variant`."""
import numpy as np

import object_points_reference as Y

f32, f64 = np.float32, np.float64
TILE, CAND_BLOCK, CHUNK, BLOCK = 1024, 256, 1024, 1024      # kTile, kCandBlock, kChunk, kBlock of csrc/object_points.hip

# a camera at the origin looking down z with unit focal length: a point (x, y, 1) projects to (x, y) exactly
CAMERA = dict(fx=1.0, fy=1.0, cx=0.0, cy=0.0, cols=640, rows=480)


def scene(map_points, cand_points, claims=None, **fields):
    d = dict(map_points=np.ascontiguousarray(map_points, f32).reshape(-1, 3), cand_points=np.ascontiguousarray(cand_points, f32).reshape(-1, 3), claims=claims or {})
    d.update(fields)
    return d


def cloud(rng, n, centre=(0.5, -0.3, 2.0), spread=(0.3, 0.2, 0.4)):
    return (np.asarray(centre) + rng.standard_normal((n, 3)) * np.asarray(spread)).astype(f32)


def pixels(uv, z=1.0):
    """points that project under CAMERA to the given pixels exactly"""
    uv = np.asarray(uv, f32).reshape(-1, 2)
    return np.concatenate([uv, np.full((len(uv), 1), z, f32)], 1)


def yaw_pose(angle, t):
    return dict(pose_q=[0.0, 0.0, np.sin(angle / 2), np.cos(angle / 2)], pose_t=t)


def frame_update(rng, M, C, repeats, rejected=False, **more):
    """a DataAssociateUpdate as the tracker sees it: a camera in front of the object, `repeats` of the candidates are list entries seen again.  ProjectRect1 is the
    mixed box itself (fIou = 1) unless the change gate is to reject."""
    mp = cloud(rng, M)
    cp = cloud(rng, C)
    pick = rng.choice(M, min(repeats, M, C), replace=False) if M else np.zeros(0, np.int64)
    cp[:len(pick)] = mp[pick]
    cp = cp[rng.permutation(C)]
    d = scene(mp, cp, fx=520.0, fy=520.0, cx=320.0, cy=240.0, cols=640, rows=480, change_gate=1, gate=Y.GATE_RADIUS, erase=Y.ERASE_PROJECTION, box_off_edge=1,
              project_rect1=[300, 100, 260, 200], box_rect=[330, 120, 180, 150], center=[0.5, -0.3, 2.0], rmax=0.9, n_frames_after_push=7,
              map_count=rng.integers(0, 14, M), cand_count=rng.integers(0, 12, C), sum_pos=mp.sum(axis=0) if M else np.zeros(3))
    d.update(more)
    rec = np.zeros((), Y.RECORD_DTYPE)
    Y.change_gate(Y.full(d), rec, sort=False)
    d["project_rect1"] = [0, 0, 10, 10] if rejected else rec["rect2"].copy()
    return d


def scenes():
    out = {}
    rng = np.random.default_rng(20240921)
    R = dict(gate=Y.GATE_RADIUS, center=[0.0, 0.0, 0.0], rmax=5.0)
    # ---- the append
    out["empty_list"] = scene(np.zeros((0, 3)), cloud(rng, 10, (0, 0, 0)), dict(n_appended=10, n_list=10, target=[-1] * 10), **R)
    out["empty_candidates"] = scene(cloud(rng, 20), np.zeros((0, 3)), dict(n_gated=0, n_list=20, n_survivors=20), **R)
    out["nothing_at_all"] = scene(np.zeros((0, 3)), np.zeros((0, 3)), dict(status=Y.DONE, n_list=0), **R)
    out["all_gated_out"] = scene(cloud(rng, 12), cloud(rng, 9, (40, 0, 0)), dict(n_gated=0, n_appended=0, gate=[0] * 9), **R)
    # sqrt(9 + 16) is exactly 5: `>` is strict; the next float above 4 on y is outside
    out["exactly_at_the_radius"] = scene(np.zeros((0, 3)), [[3, 4, 0], [3, np.nextafter(f32(4), f32(5)), 0]], dict(gate=[1, 0]), **R)
    th = [[4.5, 0, 0], [4.6, 0, 0], [5.0, 0, 0], [5.1, 0, 0]]      # (float)0.9 * 5 rounds to 4.5
    out["th_few_frames"] = scene(np.zeros((0, 3)), th, dict(gate=[1, 1, 1, 0]), n_frames_after_push=5, **R)
    out["th_many_frames"] = scene(np.zeros((0, 3)), th, dict(gate=[1, 0, 0, 0]), n_frames_after_push=6, **R)
    mp = cloud(rng, 30, (0, 0, 0))
    out["candidate_equals_an_entry"] = scene(mp, [mp[17], [1, 1, 1], mp[3]], dict(target=[17, -1, 3], n_appended=1, list=[[0, k] for k in range(30)] + [[1, 1]]), **R)
    out["entry_twice_first_wins"] = scene(np.concatenate([mp[:5], mp[2:3], mp[5:]]), [mp[2]], dict(target=[2]), **R)
    out["two_equal_candidates"] = scene(mp, [[1, 1, 1], [2, 2, 2], [1, 1, 1]], dict(target=[-1, -1, 30], n_appended=2), **R)
    # three equal candidates under the CUBOID gate of a rotated pose: equal positions share their gate, so the first cannot be out and the others in
    out["three_equal_candidates_cuboid"] = scene(mp, [[0.3, 0.2, 0.1]] * 3 + [[3.0, 0.2, 0.1]], dict(gate=[1, 1, 1, 0], target=[-1, 30, 30, -1]), gate=Y.GATE_CUBOID,
                                                 lenth=2.0, width=2.0, height=2.0, **yaw_pose(0.7, [0.1, -0.1, 0.05]))
    out["cuboid_gate_each_axis"] = scene(np.zeros((0, 3)), [[1.09, 0, 0], [1.11, 0, 0], [0, 0.54, 0], [0, 0.56, 0], [0, 0, -0.27], [0, 0, -0.28]],
                                         dict(gate=[1, 0, 1, 0, 1, 0]), gate=Y.GATE_CUBOID, lenth=2.0, width=1.0, height=0.5)
    out["zero_signs_are_equal"] = scene([[0.0, 1, 2], [-0.0, -0.0, 3]], [[-0.0, 1, 2], [0.0, 0.0, 3], [-0.0, 0.0, -0.0], [0.0, -0.0, 0.0]],
                                        dict(target=[0, 1, -1, 2], n_appended=1), **R)
    one = f32(1.0)
    out["last_bit"] = scene([[1, 1, 1]], [[np.nextafter(one, f32(2)), 1, 1], [1, np.nextafter(one, f32(0)), 1], [1, 1, 1]], dict(target=[-1, -1, 0], n_appended=2), **R)
    tiny = np.nextafter(f32(0), f32(1))      # the smallest subnormal
    out["subnormal_differences"] = scene([[tiny, 0, 0], [0, 0, 0]], [[0, tiny, 0], [tiny, 0, 0], [2 * tiny, 0, 0], [0, 0, 0]], dict(target=[-1, 0, -1, 1]), **R)
    out["gate_none_ignores_candidates"] = scene(mp, cloud(rng, 5, (0, 0, 0)), dict(n_gated=0, n_list=30, gate=[0] * 5, count=[4] * 5), cand_count=[4] * 5)
    # ---- the erase by projection (box 10 .. 20 x 10 .. 20)
    P = dict(CAMERA, erase=Y.ERASE_PROJECTION, box_off_edge=1, box_rect=[10, 10, 10, 10])
    out["counts_8_and_9"] = scene(pixels([[50, 50]] * 4), pixels([[60, 60]] * 1 + [[61, 61]]), dict(erased=[1, 1, 0, 0, 1, 0], n_erased=3), map_count=[0, 8, 9, 100],
                                  cand_count=[7, 8], sum_pos=[200, 200, 4], **dict(P, **dict(R, rmax=1000.0)))
    out["on_the_image_border"] = scene(pixels([[0, 50], [640, 50], [50, 0], [50, 480], [np.nextafter(f32(640), f32(0)), 50], [50, np.nextafter(f32(0), f32(1))], [-3, 50]]),
                                       np.zeros((0, 3)), dict(erased=[0, 0, 0, 0, 1, 1, 0]), **P)
    out["half_to_even_on_the_far_edge"] = scene(pixels([[19.5, 15], [18.5, 15], [20.5, 15], [15, 19.5], [9.5, 15], [10.5, 15], [15, 9.5]]), np.zeros((0, 3)),
                                                dict(erased=[1, 0, 1, 1, 0, 0, 0], variant=True), **P)
    out["on_the_image_edge_flag_off"] = scene(pixels([[50, 50], [15, 15]]), np.zeros((0, 3)), dict(erased=[0, 0]), **dict(P, box_off_edge=0))
    # z == 0 is a division by zero, infinite and so defined (outside the image); 0 * inf is a NaN and compares false: both stay
    out["z_zero_in_the_erase"] = scene([[1, 1, 0], [0, 0, 0], [50, 50, 1]], np.zeros((0, 3)), dict(erased=[0, 0, 1]), **P)
    # ---- the change gate: the points span 100 .. 200 on both axes, rect2 = (100, 100, 100, 100)
    G = dict(CAMERA, change_gate=1, sum_pos=[1, 2, 3])
    span = pixels([[100, 100], [200, 200], [150, 120]])
    for name, r1, box, status in (("iou_at_half", [100, 100, 100, 50], [0, 0, 1, 1], Y.DONE), ("iou_below_half_former_at_0p8", [100, 100, 100, 49], [100, 100, 100, 80], Y.DONE),
                                  ("both_below", [100, 100, 100, 49], [100, 100, 100, 79], Y.REJECTED), ("former_above", [0, 0, 10, 10], [90, 90, 200, 200], Y.DONE)):
        out["change_gate_" + name] = scene(span[:1], span[1:], dict(status=status, rect2=[100, 100, 100, 100]), project_rect1=r1, box_rect=box, **dict(G, **R))
    out["change_gate_zero_area"] = scene(span[:1], span[:1], dict(status=Y.DONE, rect2=[100, 100, 0, 0], iou=0.0, iou2=np.nan), project_rect1=[100, 100, 10, 10],
                                         box_rect=[100, 100, 10, 10], **G)
    out["change_gate_zero_over_zero_twice"] = scene(span[:1], span[:1], dict(status=Y.DONE, iou=np.nan, iou2=np.nan), project_rect1=[0, 0, 0, 0], box_rect=[0, 0, 0, 0], **G)
    out["change_gate_clamps"] = scene(pixels([[-5.5, -7], [700, 500]]), np.zeros((0, 3)), dict(status=Y.DONE, rect2=[0, 0, 640, 480]), project_rect1=[0, 0, 640, 480], **G)
    out["change_gate_truncates"] = scene(pixels([[10.9, 20.9], [30.8, 50.2]]), np.zeros((0, 3)), dict(rect2=[10, 20, 19, 29], variant=True), project_rect1=[10, 20, 19, 29], **G)
    out["change_gate_z_zero"] = scene([[1, 1, 0], [100, 100, 1]], [[-1, -1, 0]], dict(status=Y.DONE, rect2=[0, 0, 640, 480]), project_rect1=[0, 0, 640, 480], **G)
    out["change_gate_nan"] = scene([[100, 100, 1], [0, 5, 0]], span, dict(status=Y.UNDEFINED), project_rect1=[0, 0, 640, 480], **G)
    out["change_gate_all_infinite"] = scene([[1, 1, 0]], np.zeros((0, 3)), dict(status=Y.UNDEFINED), **G)
    out["change_gate_no_points"] = scene(np.zeros((0, 3)), np.zeros((0, 3)), dict(status=Y.UNDEFINED), **G)
    # ---- the two box erases
    B = dict(erase=Y.ERASE_BOX, bounds=[0, 1, 0, 1, 0, 1], sum_pos=[9, 9, 9])
    out["box_on_a_bound"] = scene([[0.5, 0.5, 0.5], [0, 0.5, 0.5], [0.5, 1, 0.5], [0.5, 0.5, np.nextafter(f32(1), f32(0))], [2, 2, 2]], np.zeros((0, 3)),
                                  dict(erased=[1, 0, 0, 1, 0], sum_pos=[9, 9, 9]), **B)
    S = dict(erase=Y.ERASE_SHRUNK, cuboid_center=[1.0, 1.0, 1.0], lenth=2.0, width=2.0, height=2.0)
    out["shrunk_on_a_bound"] = scene([[1, 1, 1], [0.5, 1, 1], [1.5, 1, 1], [1, np.nextafter(f32(1.5), f32(0)), 1], [1, 1, 0.4]], np.zeros((0, 3)), dict(erased=[1, 0, 0, 1, 0]),
                                     overlap=[1.0, 1.0, 1.0], **S)
    out["shrunk_inverted"] = scene([[1, 1, 1], [0.9, 1.1, 1]], np.zeros((0, 3)), dict(erased=[0, 0]), overlap=[2.5, 1.0, 1.0], **S)
    out["append_then_box"] = scene(cloud(rng, 40, (0.5, 0.5, 0.5), (0.4, 0.4, 0.4)), cloud(rng, 25, (0.5, 0.5, 0.5), (0.4, 0.4, 0.4)), {}, **dict(B, **R))
    # ---- sizes: one below, at and above the wavefront, the workgroup, the candidate block, the tile and the chunk
    k = 0
    for M, C in ((1, 1), (63, 1), (64, 2), (65, 3), (255, 5), (256, 7), (257, 9), (BLOCK - 1, 0), (BLOCK, 0), (BLOCK + 1, 0), (0, CAND_BLOCK - 1), (3, CAND_BLOCK), (5, CAND_BLOCK + 1),
                 (TILE - 2, 1), (TILE - 1, 2), (TILE, 3), (TILE + 1, 3), (TILE - 60, 63), (TILE - 60, 64), (TILE - 60, 65), (2 * TILE + 7, 2 * CAND_BLOCK + 3)):
        out["frame_M%d_C%d" % (M, C)] = frame_update(rng, M, C, repeats=C // 3, n_frames_after_push=5 + k % 2, box_off_edge=int(k % 5 != 4))
        k += 1
    out["frame_rejected"] = frame_update(rng, 300, 40, repeats=10, rejected=True)
    out["frame_rejected"]["claims"] = dict(status=Y.REJECTED, n_list=0, sum_pos=out["frame_rejected"]["sum_pos"])
    for C in (CHUNK - 1, CHUNK, CHUNK + 1):      # that many appended positions
        d = frame_update(rng, 9, C, repeats=0, erase=Y.ERASE_NONE, change_gate=0, rmax=50.0)
        d["claims"] = dict(n_appended=C)
        out["appended_%d" % C] = d
    mp = cloud(rng, 500, (0, 0, 0))
    out["merge_cuboid_500_300"] = scene(mp, np.concatenate([mp[rng.choice(500, 100, replace=False)], cloud(rng, 200, (0, 0, 0), (0.8, 0.8, 0.8))]), {}, gate=Y.GATE_CUBOID,
                                        lenth=1.2, width=0.9, height=1.5, sum_pos=mp.sum(axis=0), cand_count=rng.integers(0, 3, 300), **yaw_pose(-1.1, [0.05, 0.02, -0.1]))
    return out


def mixed_batch(n=64):
    """descs over every combination of the stages"""
    rng = np.random.default_rng(77)
    out = []
    for k in range(n):
        gate, erase, cg = k % 3, (k // 3) % 4, (k // 12) % 2
        M, C = int(rng.integers(0, 400)), int(rng.integers(0, 120))
        d = frame_update(rng, M, C, repeats=C // 2, rejected=k % 5 == 0, change_gate=cg, gate=gate, erase=erase, lenth=1.0, width=0.8, height=1.4, bounds=[0.3, 0.8, -0.5, -0.1, 1.6, 2.3],
                         cuboid_center=[0.5, -0.3, 2.0], overlap=[0.2, 0.1, 0.3], pose_t=[0.5, -0.3, 2.0])
        out.append(d)
    return out


def large(M=1 << 16, C=1 << 12):
    """one desc whose compare is spread over several workgroups"""
    rng = np.random.default_rng(4711)
    d = frame_update(rng, M, C, repeats=C // 2, rmax=1.2)
    d["cand_points"][-C // 8:] = d["cand_points"][:C // 8]      # candidates seen twice in one call: the second targets the first's appended slot
    return d
