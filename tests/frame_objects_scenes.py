"""Seeded scenes for a frame's 2D objects (tests/frame_objects_reference.py is the yardstick).  scenes() -> {name: (frame, reaches)}: `reaches` takes the
yardstick's result and says whether the scene got to the branch it was made for (tests/test_frame_objects_reference_cpu.py asserts it for every scene)."""
import numpy as np

f32 = np.float32
CAM = dict(fx=517.3, fy=516.5, cx=318.6, cy=255.3, cols=640, rows=480)
IDENTITY = np.eye(4, dtype=np.float32)


def pose(seed=1):
    """a small rotation and translation: no product of Rcw * X + tcw is trivial"""
    rs = np.random.RandomState(seed)
    w = rs.normal(0, 0.05, 3)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    R = np.eye(3) + K + K @ K / 2
    R, _ = np.linalg.qr(R)
    R = R * np.sign(np.diag(R))
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, rs.normal(0, 0.1, 3)
    return T.astype(np.float32)


def frame(kp, xyz, boxes, score=None, ids=None, Tcw=None, **cam):
    kp, xyz, boxes = np.asarray(kp, f32).reshape(-1, 2), np.asarray(xyz, f32).reshape(-1, 3), np.asarray(boxes, np.int32).reshape(-1, 4)
    fr = dict(CAM, **cam)
    fr.update(kp_x=np.ascontiguousarray(kp[:, 0]), kp_y=np.ascontiguousarray(kp[:, 1]), mp_xyz=xyz, boxes=boxes,
              mp_id=np.arange(len(kp), dtype=np.int32) if ids is None else np.asarray(ids, np.int32),
              score=np.linspace(0.9, 0.5, len(boxes)).astype(f32) if score is None else np.asarray(score, f32),
              Tcw=pose() if Tcw is None else np.asarray(Tcw, f32))
    return fr


def cloud(rs, n, z=2.0, spread=0.3):
    return np.column_stack([rs.normal(0, spread, n), rs.normal(0, spread, n), rs.normal(z, spread, n)]).astype(f32)


def inside(rs, box, n):
    """n keypoints well inside a box (a margin of one pixel)"""
    x, y, w, h = box
    return np.column_stack([rs.uniform(x + 1, x + w - 2, n), rs.uniform(y + 1, y + h - 2, n)]).astype(f32)


def boxes_with_points(rs, boxes, counts, **kw):
    """every box with its own count of keypoints inside (the boxes may overlap: a keypoint then also falls into the others)"""
    kp = np.concatenate([inside(rs, b, c) for b, c in zip(boxes, counts)] + [np.zeros((0, 2), f32)])
    return frame(kp, cloud(rs, len(kp)), boxes, **kw)


def lists(res, k=0, which="assigned"):
    return [int(i) for i in res[which][k]]


def scenes():
    S = {}
    rs = np.random.RandomState(20241)

    # left / top inclusive, right / bottom exclusive (:3046)
    box = (100, 100, 50, 40)
    kp = [(100, 120), (149, 120), (150, 120), (99, 120), (120, 100), (120, 139), (120, 140), (120, 99), (100, 100), (149, 139), (150, 140)]
    S["box_edges"] = (frame(kp, cloud(rs, len(kp)), [box]), lambda r: lists(r) == [0, 1, 4, 5, 8, 9])

    # x.5 at even and odd integers: cvRound goes to the even neighbour
    kp = [(99.5, 55), (100.5, 55), (101.5, 55), (98.5, 55), (100, 49.5), (100, 50.5), (100, 59.5), (100, 58.5), (0.5, 0.5), (1.5, 1.5)]
    S["ties_to_even"] = (frame(kp, cloud(rs, len(kp)), [(100, 50, 2, 10), (0, 0, 2, 2)]), lambda r: lists(r) == [0, 1, 4, 5, 7] and lists(r, 1) == [8])

    # negative coordinates: -0.5 rounds to -0, -10.5 to -10, -11.5 to -12, (-9.5, 9.5) to (-10, 10): below the box; the feature box clamps at 0
    kp = [(-0.5, -0.5), (-10.5, -3), (-11.5, 0), (-9.5, 9.5), (5, 5), (9.49, -10.49), (10.5, 0)]
    S["negative_coordinates"] = (frame(kp, cloud(rs, len(kp)), [(-10, -10, 20, 20)]),
                                 lambda r: lists(r) == [0, 1, 4, 5] and [int(v) for v in r["records"]["feature_rect"][0]] == [0, 0, 9, 5])

    # one keypoint in three boxes: it joins three lists and three sums
    S["point_in_three_boxes"] = (frame([(200, 200), (150, 150), (250, 250)], cloud(rs, 3), [(140, 140, 100, 100), (180, 180, 100, 100), (190, 100, 30, 120)]),
                                 lambda r: all(0 in lists(r, k) for k in range(3)))

    # one map point at two keypoints: `feature` is the LAST keypoint that lay in any box, also for the list of the box only the first one is in
    kp = np.concatenate([inside(rs, (100, 100, 60, 60), 5), [(400.25, 300.75)], [(620, 20)]]).astype(f32)
    ids = [0, 1, 2, 3, 4, 2, 3]      # keypoint 5 (in box 1) holds map point 2 again; keypoint 6 (in no box) holds map point 3 again
    S["map_point_at_two_keypoints"] = (frame(kp, cloud(rs, 7), [(100, 100, 60, 60), (380, 280, 60, 60)], ids=ids),
                                       lambda r: lists(r) == [0, 1, 2, 3, 4] and lists(r, 1) == [5] and int(r["records"]["feature_rect"][0][2]) > 200)

    # the same frame with ids beyond the library's direct table of map point ids
    S["map_point_at_two_keypoints_large_ids"] = (frame(kp, S["map_point_at_two_keypoints"][0]["mp_xyz"], [(100, 100, 60, 60), (380, 280, 60, 60)],
                                                       ids=np.asarray(ids) + 2 ** 30), S["map_point_at_two_keypoints"][1])

    # a box without points: n = 0, _Pos = 0 * inf
    S["box_without_points"] = (boxes_with_points(rs, [(100, 100, 80, 80), (400, 300, 80, 80)], [12, 0]),
                               lambda r: int(r["records"]["n"][1]) == 0 and bool(np.isnan(r["records"]["pos"][1]).all()) and bool(np.isnan(r["records"]["std"][1]).all()))

    # 3 / 4 points: the feature box; 7 / 8 points: the boxplot
    S["three_four_seven_eight_points"] = (boxes_with_points(rs, [(40, 40, 80, 80), (200, 40, 80, 80), (40, 200, 80, 80), (200, 200, 80, 80)], [3, 4, 7, 8]),
                                          lambda r: [int(v) for v in r["records"]["has_feature_rect"]] == [0, 1, 1, 1] and
                                          [int(v) for v in r["records"]["boxplot_ran"]] == [0, 0, 0, 1])

    # z ties at Q1 and Q3 (the identity pose: z is the world z): n = 12, ranks 3 and 9
    z = [1.0, 2.0, 1.5, 1.0, 2.0, 0.5, 1.0, 2.0, 2.5, 0.75, 1.0, 2.0]
    xyz = np.column_stack([rs.normal(0, 0.3, 12), rs.normal(0, 0.3, 12), z]).astype(f32)
    S["z_ties_at_quartiles"] = (frame(inside(rs, (100, 100, 80, 80), 12), xyz, [(100, 100, 80, 80)], Tcw=IDENTITY),
                                lambda r: float(r["records"]["q1"][0]) == 1.0 and float(r["records"]["q3"][0]) == 2.0)

    # -0.0f and +0.0f tie at Q1: z = -0.0 needs every term of the row negative zero (x, y < 0, tz = -0.0)
    T = IDENTITY.copy()
    T[2, 3] = -0.0
    z = [1.0, -0.0, 0.0, -1.0, -0.0, 2.0, 3.0, 0.0, 4.0, 5.0, -2.0, 6.0]
    xyz = np.column_stack([-np.abs(rs.normal(1, 0.1, 12)), -np.abs(rs.normal(1, 0.1, 12)), z]).astype(f32)
    S["zero_signs_at_quartile"] = (frame(inside(rs, (100, 100, 80, 80), 12), xyz, [(100, 100, 80, 80)], Tcw=T),
                                   lambda r: float(r["records"]["q1"][0]) == 0.0 and float(r["records"]["q3"][0]) == 4.0)

    # a z exactly equal to max_th stays: Q1 = 1, Q3 = 2, max_th = 3.5
    z = [1.0, 2.0, 1.0, 2.0, 3.5, 1.0, 2.0, 3.75, 0.5, 1.0, 2.0, 0.5]
    xyz = np.column_stack([rs.normal(0, 0.3, 12), rs.normal(0, 0.3, 12), z]).astype(f32)
    S["z_equal_to_max_th"] = (frame(inside(rs, (100, 100, 80, 80), 12), xyz, [(100, 100, 80, 80)], Tcw=IDENTITY),
                              lambda r: float(r["records"]["max_th"][0]) == 3.5 and lists(r, 0, "kept") == [0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 11])

    # the quirk: two far points leave, sum_pos_3d keeps them, and _Pos lies behind every point that stayed
    xyz = np.concatenate([cloud(rs, 10, 1.0, 0.05), cloud(rs, 2, 200.0, 0.05)])[[0, 10, 1, 2, 3, 4, 5, 6, 11, 7, 8, 9]]
    S["pos_leaves_the_hull"] = (frame(inside(rs, (100, 100, 80, 80), 12), xyz, [(100, 100, 80, 80)], Tcw=IDENTITY),
                                lambda r: int(r["records"]["n"][0]) == 10 and lists(r, 0, "kept") == [0, 2, 3, 4, 5, 6, 7, 9, 10, 11] and float(r["records"]["pos"][0][2]) > 30.0)

    # the passes of 256 keypoints and the 64-lane waves within: a box of all keypoints and one of about a third
    for n in (63, 64, 65, 255, 256, 257):
        kp = np.column_stack([rs.uniform(10, 600, n), rs.uniform(10, 450, n)]).astype(f32)
        ids = np.arange(n, dtype=np.int32)
        ids[rs.rand(n) < 0.1] = -1
        S["n_kp_%d" % n] = (frame(kp, cloud(rs, n), [(0, 0, 640, 480), (5, 5, 200, 470)], ids=ids),
                            lambda r, n=n, ids=ids: int(r["records"]["n_assigned"][0]) == int((ids >= 0).sum()) and 0 < int(r["records"]["n_assigned"][1]) < n)

    # a box that holds all 4096 keypoints (and one that holds some)
    kp = np.column_stack([rs.uniform(0, 639, 4096), rs.uniform(0, 479, 4096)]).astype(f32)
    S["all_4096_in_one_box"] = (frame(kp, cloud(rs, 4096), [(0, 0, 640, 480), (300, 200, 40, 40)]), lambda r: int(r["records"]["n_assigned"][0]) == 4096)

    # zero-area boxes: no points, and 0 / 0 in the overlap ratios
    S["zero_area_boxes"] = (boxes_with_points(rs, [(100, 100, 80, 80), (120, 120, 0, 30), (130, 130, 30, 0), (140, 140, 0, 0)], [12, 0, 0, 0]),
                            lambda r: [int(v) for v in r["records"]["n_assigned"][1:]] == [0, 0, 0] and int(r["records"]["num_overlaps"][0]) == 0)

    # more than four overlaps: the crowded box is bad before the second loop
    crowd = [(200, 150, 120, 120)] + [(180 + 30 * k, 140 + 20 * k, 60, 60) for k in range(5)] + [(500, 350, 60, 60)]
    S["more_than_four_overlaps"] = (boxes_with_points(rs, crowd, [12] * 7), lambda r: int(r["records"]["num_overlaps"][0]) == 5 and int(r["records"]["bad"][0]) == 1)

    # equal scores: `>=` removes the later box
    pair = [(200, 200, 100, 100), (240, 200, 100, 100)]
    S["equal_scores"] = (boxes_with_points(rs, pair, [12, 12], score=[0.7, 0.7]), lambda r: [int(v) for v in r["records"]["bad"]] == [0, 1])
    # a NaN score: neither branch fires, both stay
    S["nan_score"] = (boxes_with_points(rs, pair, [12, 12], score=[np.nan, 0.7]), lambda r: [int(v) for v in r["records"]["bad"]] == [0, 0])

    # box 0 loses to box 1, turns bad in mid-body, and still removes box 2
    trio = [(200, 200, 100, 100), (240, 200, 100, 100), (160, 200, 100, 100)]
    S["bad_in_mid_body"] = (boxes_with_points(rs, trio, [12, 12, 12], score=[0.6, 0.9, 0.5]), lambda r: [int(v) for v in r["records"]["bad"]] == [1, 0, 1])

    # the 5-pixel edge mark and the `< 5` / `5 .. 9 near a 20-pixel edge` rules, at and beside their bounds (cols 640, rows 480)
    edge = [(4, 100, 60, 40), (5, 160, 60, 40), (575, 100, 60, 40), (576, 160, 60, 40), (19, 300, 60, 40), (20, 360, 60, 40), (19, 420, 60, 39), (200, 300, 60, 40),
            (300, 300, 60, 40), (400, 300, 60, 40), (400, 420, 60, 40), (500, 420, 60, 41)]
    S["edge_rules"] = (boxes_with_points(rs, edge, [12, 12, 12, 12, 9, 9, 10, 4, 5, 9, 9, 9]),
                       lambda r: [int(v) for v in r["records"]["on_edge"]] == [1, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0] and
                       [int(v) for v in r["records"]["bad"]] == [0, 0, 0, 0, 1, 0, 0, 1, 0, 0, 0, 1])

    # more than half of the image
    S["large_box"] = (boxes_with_points(rs, [(30, 30, 500, 400), (560, 30, 50, 50)], [12, 12]), lambda r: [int(v) for v in r["records"]["bad"]] == [1, 0])

    # the feature box truncates: 10.7 -> 10, 50.9 - 10.7 = 40.2 -> 40 (rounding would give 11 and 40, 20.6 -> 20 and 70.9 - 20.6 -> 50)
    kp = [(10.7, 20.6), (50.9, 30.2), (30.3, 70.9), (25.5, 40.4), (45.1, 60.6)]
    S["feature_box_truncates"] = (frame(kp, cloud(rs, 5), [(0, 0, 100, 100)]), lambda r: [int(v) for v in r["records"]["feature_rect"][0]] == [10, 20, 40, 50])

    # no keypoints at all, and no boxes at all
    S["frame_without_keypoints"] = (frame(np.zeros((0, 2)), np.zeros((0, 3)), [(100, 100, 50, 50)]), lambda r: int(r["records"]["n_assigned"][0]) == 0)
    S["frame_without_boxes"] = (frame(inside(rs, (100, 100, 50, 50), 8), cloud(rs, 8), np.zeros((0, 4))), lambda r: len(r["records"]) == 0)

    S["timing_shape"] = (timing_frame(7), lambda r: len(r["records"]) == 16 and int(r["records"]["boxplot_ran"].sum()) >= 8)
    return S


def timing_frame(seed):
    """one frame of the timing workload's shape: 1500 keypoints, 16 boxes, nine in ten keypoints with a map point, a far tail in the depths"""
    rs = np.random.RandomState(seed)
    n = 1500
    kp = np.column_stack([rs.uniform(0, 640, n), rs.uniform(0, 480, n)]).astype(f32)
    ids = np.arange(n, dtype=np.int32)
    ids[rs.rand(n) < 0.1] = -1
    xyz = cloud(rs, n, 2.5, 0.6)
    far = rs.rand(n) < 0.05
    xyz[far, 2] += rs.uniform(3, 10, int(far.sum())).astype(f32)
    boxes = [(int(rs.randint(0, 440)), int(rs.randint(0, 300)), int(rs.randint(60, 200)), int(rs.randint(60, 180))) for _ in range(16)]
    return frame(kp, xyz, boxes, score=rs.uniform(0.3, 0.95, 16), ids=ids, Tcw=pose(seed))
