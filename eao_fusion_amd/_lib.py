"""ctypes binding of libeaofusion_hip.so (the C-ABI in include/eao_fusion.h).

The library is the product; this module only loads it.  There is no CPU fallback anywhere in this package:
if the shared object is missing or no MI355X is visible, calls fail loudly.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("EAO_LIB_PATH") or os.path.join(HERE, "libeaofusion_hip.so")      # (EAO_LIB_PATH: A/B runs against another build of the library)

EAO_OK, EAO_ERR_INVALID, EAO_ERR_NO_DEVICE, EAO_ERR_CAPACITY, EAO_ERR_INTERNAL = 0, -1, -2, -3, -4


class EaoError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__("eao status %d: %s" % (status, msg))
        self.status = status


class OrbCfg(C.Structure):
    _fields_ = [("nfeatures", C.c_int32), ("scale_factor", C.c_float), ("nlevels", C.c_int32),
                ("ini_th_fast", C.c_int32), ("min_th_fast", C.c_int32)]


class OrbSlot(C.Structure):   # eao_orb_slot
    _fields_ = [("frames", C.c_void_p), ("stride", C.c_int32), ("frame_stride", C.c_int64), ("kps", C.c_void_p), ("desc", C.c_void_p),
                ("n", C.c_void_p), ("cap", C.c_int32)]


class OrbLevelView(C.Structure):   # eao_orb_level_view
    _fields_ = [("data", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32), ("step", C.c_int32)]


class FrameView(C.Structure):
    _fields_ = [("n", C.c_int32), ("kp_x", C.c_void_p), ("kp_y", C.c_void_p), ("kp_octave", C.c_void_p), ("kp_angle", C.c_void_p),
                ("u_right", C.c_void_p), ("descriptors", C.c_void_p), ("occupied", C.c_void_p),
                ("min_x", C.c_float), ("min_y", C.c_float), ("max_x", C.c_float), ("max_y", C.c_float),
                ("grid_inv_w", C.c_float), ("grid_inv_h", C.c_float), ("grid_cols", C.c_int32), ("grid_rows", C.c_int32),
                ("scale_factors", C.c_void_p), ("nlevels", C.c_int32),
                ("log_scale_factor", C.c_float), ("level_sigma2", C.c_void_p), ("inv_level_sigma2", C.c_void_p)]


class PoseProblem(C.Structure):
    _fields_ = [("n", C.c_int32), ("Tcw", C.c_void_p), ("Xw", C.c_void_p), ("obs", C.c_void_p),
                ("inv_sigma2", C.c_void_p), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float),
                ("cy", C.c_float), ("bf", C.c_float),
                ("n_planes", C.c_int32), ("plane_world", C.c_void_p), ("plane_obs", C.c_void_p), ("plane_seen", C.c_void_p)]


class PoseResult(C.Structure):
    _fields_ = [("Tcw", C.c_float * 16), ("outlier", C.c_void_p), ("n_inliers", C.c_int32),
                ("lm_iterations", C.c_int32), ("plane_outlier", C.c_void_p)]


class BAProblem(C.Structure):
    _fields_ = [("n_cams", C.c_int32), ("n_points", C.c_int32), ("n_edges", C.c_int32),
                ("cam_Tcw", C.c_void_p), ("cam_fixed", C.c_void_p), ("points", C.c_void_p),
                ("edge_cam", C.c_void_p), ("edge_point", C.c_void_p), ("edge_obs", C.c_void_p),
                ("edge_inv_sigma2", C.c_void_p), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float),
                ("cy", C.c_float), ("bf", C.c_float), ("its_first", C.c_int32), ("its_second", C.c_int32)]


class BAPlanes(C.Structure):   # eao_ba_planes
    _fields_ = [("n_planes", C.c_int32), ("plane_world", C.c_void_p), ("n_pedges", C.c_int32), ("pedge_plane", C.c_void_p),
                ("pedge_cam", C.c_void_p), ("pedge_obs", C.c_void_p)]


class BAResult(C.Structure):
    _fields_ = [("cam_Tcw", C.c_void_p), ("points", C.c_void_p), ("edge_outlier", C.c_void_p),
                ("iters", C.c_int32 * 2), ("aborted", C.c_int32), ("chi2", C.c_double * 2)]


class Sim3Problem(C.Structure):   # eao_sim3_problem
    _fields_ = [("n", C.c_int32), ("T1w", C.c_void_p), ("T2w", C.c_void_p), ("Xw1", C.c_void_p), ("Xw2", C.c_void_p),
                ("obs1", C.c_void_p), ("obs2", C.c_void_p), ("inv_sigma2_1", C.c_void_p), ("inv_sigma2_2", C.c_void_p),
                ("fx1", C.c_float), ("fy1", C.c_float), ("cx1", C.c_float), ("cy1", C.c_float),
                ("fx2", C.c_float), ("fy2", C.c_float), ("cx2", C.c_float), ("cy2", C.c_float),
                ("q", C.c_double * 4), ("t", C.c_double * 3), ("s", C.c_double), ("th2", C.c_float), ("fix_scale", C.c_int32)]


class Sim3Result(C.Structure):   # eao_sim3_result
    _fields_ = [("q", C.c_double * 4), ("t", C.c_double * 3), ("s", C.c_double), ("removed", C.c_void_p),
                ("n_inliers", C.c_int32), ("lm_iterations", C.c_int32 * 2), ("early_exit", C.c_int32)]


class Sim3SolverProblem(C.Structure):   # eao_sim3_solver_problem
    _fields_ = [("n", C.c_int32), ("T1w", C.c_void_p), ("T2w", C.c_void_p), ("Xw1", C.c_void_p), ("Xw2", C.c_void_p),
                ("sigma2_1", C.c_void_p), ("sigma2_2", C.c_void_p),
                ("fx1", C.c_float), ("fy1", C.c_float), ("cx1", C.c_float), ("cy1", C.c_float),
                ("fx2", C.c_float), ("fy2", C.c_float), ("cx2", C.c_float), ("cy2", C.c_float), ("fix_scale", C.c_int32)]


class Sim3SolverState(C.Structure):   # eao_sim3_solver_state
    _fields_ = [("iterations", C.c_int32), ("best_inliers", C.c_int32), ("best_T12", C.c_float * 16), ("best_R", C.c_float * 9),
                ("best_t", C.c_float * 3), ("best_s", C.c_float)]


class Sim3SolverResult(C.Structure):   # eao_sim3_solver_result
    _fields_ = [("returned", C.c_int32), ("n_inliers", C.c_int32), ("T12", C.c_float * 16), ("inlier", C.c_void_p), ("no_more", C.c_int32),
                ("hyp_inliers", C.c_void_p), ("hyp_T12", C.c_void_p), ("hyp_T21", C.c_void_p), ("hyp_inlier", C.c_void_p)]


class InitializerProblem(C.Structure):   # eao_initializer_problem
    _fields_ = [("n1", C.c_int32), ("n2", C.c_int32), ("keys1_xy", C.c_void_p), ("keys2_xy", C.c_void_p), ("n_matches", C.c_int32), ("matches12", C.c_void_p),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("sigma", C.c_float), ("min_parallax", C.c_float),
                ("min_triangulated", C.c_int32)]


class InitializerResult(C.Structure):   # eao_initializer_result
    _fields_ = [("returned", C.c_int32), ("branch", C.c_int32), ("no_model", C.c_int32), ("degenerate", C.c_int32),
                ("SH", C.c_float), ("SF", C.c_float), ("RH", C.c_float), ("best_h", C.c_int32), ("best_f", C.c_int32),
                ("H21", C.c_float * 9), ("F21", C.c_float * 9), ("R21", C.c_float * 9), ("t21", C.c_float * 3),
                ("parallax", C.c_float), ("cos_parallax", C.c_float), ("n_good", C.c_int32), ("motion", C.c_int32), ("n_motions", C.c_int32),
                ("n_inliers", C.c_int32), ("p3d", C.c_void_p), ("triangulated", C.c_void_p),
                ("hyp_H21", C.c_void_p), ("hyp_H12", C.c_void_p), ("hyp_F21", C.c_void_p), ("hyp_SH", C.c_void_p), ("hyp_SF", C.c_void_p),
                ("hyp_inlier_H", C.c_void_p), ("hyp_inlier_F", C.c_void_p), ("inlier", C.c_void_p),
                ("mot_R", C.c_void_p), ("mot_t", C.c_void_p), ("mot_n_good", C.c_void_p), ("mot_cos", C.c_void_p), ("mot_good", C.c_void_p),
                ("mot_p3d", C.c_void_p)]


class PnpSolverProblem(C.Structure):   # eao_pnp_solver_problem
    _fields_ = [("n", C.c_int32), ("p3d_w", C.c_void_p), ("p2d", C.c_void_p), ("sigma2", C.c_void_p),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("th2", C.c_float)]


class PnpSolverState(C.Structure):   # eao_pnp_solver_state
    _fields_ = [("iterations", C.c_int32), ("best_inliers", C.c_int32), ("best_Tcw", C.c_float * 16), ("best_inlier", C.c_void_p)]


class PnpSolverResult(C.Structure):   # eao_pnp_solver_result
    _fields_ = [("returned", C.c_int32), ("refined", C.c_int32), ("n_inliers", C.c_int32), ("Tcw", C.c_float * 16), ("inlier", C.c_void_p),
                ("no_more", C.c_int32), ("n_records", C.c_int32),
                ("hyp_R", C.c_void_p), ("hyp_t", C.c_void_p), ("hyp_rep_err", C.c_void_p), ("hyp_choice", C.c_void_p), ("hyp_inliers", C.c_void_p),
                ("hyp_inlier", C.c_void_p),
                ("rec_hyp", C.c_void_p), ("rec_R", C.c_void_p), ("rec_t", C.c_void_p), ("rec_inliers", C.c_void_p), ("rec_inlier", C.c_void_p)]


class EssentialGraphProblem(C.Structure):   # eao_essential_graph_problem
    _fields_ = [("n", C.c_int32), ("fixed", C.c_int32), ("fix_scale", C.c_int32), ("Scw", C.c_void_p), ("has_nc", C.c_void_p), ("Snc", C.c_void_p),
                ("n_edges", C.c_int32), ("edges", C.c_void_p), ("n_points", C.c_int32), ("Xw", C.c_void_p), ("ref", C.c_void_p)]


class EssentialGraphResult(C.Structure):   # eao_essential_graph_result
    _fields_ = [("Scw", C.c_void_p), ("Tiw", C.c_void_p), ("Xw_corrected", C.c_void_p), ("lm_iterations", C.c_int32), ("trials", C.c_int32 * 20),
                ("lambda_", C.c_double * 20), ("chi2", C.c_double * 20), ("chi2_initial", C.c_double), ("n_active", C.c_int32)]


class VocabularyDesc(C.Structure):   # eao_vocabulary_desc
    _fields_ = [("n_nodes", C.c_int32), ("parent", C.c_void_p), ("descriptor", C.c_void_p), ("weight", C.c_void_p), ("is_leaf", C.c_void_p),
                ("weighting", C.c_int32), ("norm", C.c_int32)]


class BowResult(C.Structure):   # eao_bow_result
    _fields_ = [("n_words", C.c_int32), ("word_id", C.c_void_p), ("word_value", C.c_void_p),
                ("n_fv_nodes", C.c_int32), ("node_id", C.c_void_p), ("node_start", C.c_void_p), ("index", C.c_void_p),
                ("feat_word", C.c_void_p), ("feat_node", C.c_void_p), ("feat_stopped", C.c_void_p)]


class KeyFrameDbQuery(C.Structure):   # eao_keyframe_db_query
    _fields_ = [("kind", C.c_int32), ("query_id", C.c_uint64), ("nq", C.c_int32), ("q_id", C.c_void_p), ("q_val", C.c_void_p),
                ("n_connected", C.c_int32), ("connected_id", C.c_void_p), ("min_score", C.c_float)]


class KeyFrameDbScored(C.Structure):   # eao_keyframe_db_scored
    _fields_ = [("n_sharing", C.c_int32), ("sharing_id", C.c_void_p), ("sharing_words", C.c_void_p),
                ("max_common_words", C.c_int32), ("min_common_words", C.c_int32), ("n_scores", C.c_int32),
                ("n_scored", C.c_int32), ("scored_id", C.c_void_p), ("scored_score", C.c_void_p)]


class PlaneSegCfg(C.Structure):   # eao_plane_seg_cfg
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("window", C.c_int32), ("min_support", C.c_int32), ("max_step", C.c_int32), ("leaf", C.c_float),
                ("depth_min", C.c_double), ("depth_max", C.c_double), ("depth_sigma", C.c_double), ("std_tol_init", C.c_double), ("std_tol_merge", C.c_double),
                ("z_near", C.c_double), ("z_far", C.c_double), ("angle_near", C.c_double), ("angle_far", C.c_double),
                ("similarity_merge", C.c_double), ("similarity_refine", C.c_double), ("depth_alpha", C.c_double), ("depth_change_tol", C.c_double)]


class PlaneSegPlane(C.Structure):   # eao_plane_seg_plane
    _fields_ = [("normal", C.c_double * 3), ("center", C.c_double * 3), ("mse", C.c_double), ("curvature", C.c_double), ("N", C.c_int32), ("rid", C.c_int32),
                ("coef", C.c_float * 4), ("kept", C.c_int32), ("cloud_offset", C.c_int32), ("cloud_count", C.c_int32), ("n_pixels", C.c_int32)]


class DetnetDesc(C.Structure):   # eao_detnet_desc
    _fields_ = [("classes", C.c_int32), ("anchors", C.c_int32), ("tensors", C.c_int32), ("ops", C.c_int32), ("input_size", C.c_int32), ("max_batch", C.c_int32),
                ("weight_bytes", C.c_int64), ("activation_bytes", C.c_int64), ("flops", C.c_double)]


class ObjectCuboidDesc(C.Structure):   # eao_object_cuboid_desc
    _fields_ = [("n_points", C.c_int32), ("points", C.c_void_p), ("n_centroids", C.c_int32), ("centroids", C.c_void_p), ("Ryaw", C.c_float * 9),
                ("prev_cuboid_center", C.c_double * 3)]


class ObjectCuboidRec(C.Structure):   # eao_object_cuboid_rec
    _fields_ = [("status", C.c_int32), ("bounds_written", C.c_int32), ("sum_pos", C.c_float * 3), ("center", C.c_float * 3), ("standar", C.c_float * 3),
                ("center_standar", C.c_float * 3), ("center_standar_dis", C.c_float), ("bounds", C.c_float * 6),
                ("lenth", C.c_float), ("width", C.c_float), ("height", C.c_float), ("rmax", C.c_float), ("reserved", C.c_int32),
                ("Twobj", C.c_float * 16), ("Twobj_without_yaw", C.c_float * 16), ("cuboid_center", C.c_double * 3),
                ("corners", C.c_double * 3 * 8), ("corners_w", C.c_double * 3 * 8), ("pose_q", C.c_double * 4), ("pose_t", C.c_double * 3),
                ("pose_without_yaw_q", C.c_double * 4), ("pose_without_yaw_t", C.c_double * 3)]


class ObjectOverlapRow(C.Structure):   # eao_object_overlap_row
    _fields_ = [("cuboid_center", C.c_double * 3), ("lenth", C.c_float), ("width", C.c_float), ("height", C.c_float), ("reserved", C.c_int32)]


class ObjectPointsDesc(C.Structure):   # eao_object_points_desc
    _fields_ = [("change_gate", C.c_int32), ("gate", C.c_int32), ("erase", C.c_int32), ("box_off_edge", C.c_int32), ("n_map", C.c_int32), ("n_cand", C.c_int32),
                ("map_points", C.c_void_p), ("map_count", C.c_void_p), ("cand_points", C.c_void_p), ("cand_count", C.c_void_p), ("Tcw", C.c_float * 16),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("cols", C.c_int32), ("rows", C.c_int32),
                ("project_rect1", C.c_int32 * 4), ("box_rect", C.c_int32 * 4), ("center", C.c_float * 3), ("rmax", C.c_float), ("n_frames_after_push", C.c_int32),
                ("lenth", C.c_float), ("width", C.c_float), ("height", C.c_float), ("pose_q", C.c_double * 4), ("pose_t", C.c_double * 3),
                ("cuboid_center", C.c_double * 3), ("bounds", C.c_float * 6), ("overlap", C.c_float * 3), ("sum_pos", C.c_float * 3), ("reserved", C.c_int32),
                ("survivors", C.c_void_p)]


class ObjectPointsRec(C.Structure):   # eao_object_points_rec
    _fields_ = [("status", C.c_int32), ("n_gated", C.c_int32), ("n_appended", C.c_int32), ("n_list", C.c_int32), ("n_erased", C.c_int32), ("n_survivors", C.c_int32),
                ("rect2", C.c_int32 * 4), ("iou", C.c_float), ("iou2", C.c_float), ("sum_pos_appended", C.c_float * 3), ("sum_pos", C.c_float * 3),
                ("reserved", C.c_int32 * 2)]


class ObjectPointsOut(C.Structure):   # eao_object_points_out
    _fields_ = [("rec", C.c_void_p), ("gate", C.c_void_p), ("target", C.c_void_p), ("count", C.c_void_p), ("list", C.c_void_p), ("erased", C.c_void_p),
                ("survivors", C.c_void_p)]


class ObjectChainDesc(C.Structure):   # eao_object_chain_desc
    _fields_ = [("points", ObjectPointsDesc), ("map_bad", C.c_void_p), ("cand_bad", C.c_void_p), ("cand_alias", C.c_void_p), ("n_centroids", C.c_int32),
                ("class_id", C.c_int32), ("centroids", C.c_void_p), ("Ryaw", C.c_float * 9), ("bi_forest", C.c_int32), ("prev_cuboid_center", C.c_double * 3)]


class ObjectChainRec(C.Structure):   # eao_object_chain_rec
    _fields_ = [("n_final", C.c_int32), ("forest_status", C.c_int32), ("removed", C.c_int32), ("reserved", C.c_int32)]


class ObjectChainOut(C.Structure):   # eao_object_chain_out
    _fields_ = [("points", ObjectPointsOut), ("rec", C.c_void_p), ("final", C.c_void_p), ("cuboid", C.c_void_p), ("forest_flags", C.c_void_p), ("scores", C.c_void_p)]


class YoloxCfg(C.Structure):   # eao_yolox_cfg
    _fields_ = [("input_size", C.c_int32), ("num_classes", C.c_int32), ("conf_thresh", C.c_float), ("nms_thresh", C.c_float),
                ("max_proposals", C.c_int32), ("max_batch", C.c_int32)]


class FrameObjectsDesc(C.Structure):   # eao_frame_objects_desc
    _fields_ = [("n_kp", C.c_int32), ("kp_x", C.c_void_p), ("kp_y", C.c_void_p), ("mp_id", C.c_void_p), ("mp_xyz", C.c_void_p),
                ("n_box", C.c_int32), ("boxes", C.c_void_p), ("score", C.c_void_p), ("Tcw", C.c_float * 16),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("cols", C.c_int32), ("rows", C.c_int32)]


class FrameObjectRecord(C.Structure):   # eao_frame_object_record
    _fields_ = [("n_assigned", C.c_int32), ("n", C.c_int32), ("sum_pos", C.c_float * 3), ("pos", C.c_float * 3), ("std", C.c_float * 3),
                ("q1", C.c_float), ("q3", C.c_float), ("max_th", C.c_float), ("boxplot_ran", C.c_int32), ("center_2d", C.c_float * 2),
                ("has_feature_rect", C.c_int32), ("feature_rect", C.c_int32 * 4), ("num_overlaps", C.c_int32), ("bad", C.c_int32), ("on_edge", C.c_int32)]


class FrameObjectsOut(C.Structure):   # eao_frame_objects_out
    _fields_ = [("records", C.c_void_p), ("assigned_start", C.c_void_p), ("assigned", C.c_void_p), ("assigned_cap", C.c_int64),
                ("kept_start", C.c_void_p), ("kept", C.c_void_p), ("kept_cap", C.c_int64)]


# every symbol include/eao_fusion.h declares: (restype, argtypes)
_P = C.c_void_p
_I = C.c_int32
SYMBOLS = {
    "eao_last_error": (C.c_char_p, []),
    "eao_device_check": (_I, []),
    "eao_version": (C.c_char_p, []),
    "eao_orb_create": (_I, [C.POINTER(OrbCfg), C.POINTER(_P)]),
    "eao_orb_destroy": (None, [_P]),
    "eao_orb_tables": (_I, [_P, _P, _P, _P, _P, _P]),
    "eao_orb_max_keypoints": (_I, [_P, _I, _I, C.POINTER(_I)]),
    "eao_orb_extract": (_I, [_P, _P, _I, _I, _I, _P, _P, _I, C.POINTER(_I)]),
    "eao_orb_extract_batch": (_I, [_P, _P, _I, _I, _I, C.c_int64, _I, _P, _P, _I, _P]),
    "eao_orb_extract_batch_device": (_I, [_P, _P, _I, _I, _I, C.c_int64, _I, _P, _P, _I, _P, _P]),
    "eao_orb_stream_create": (_I, [_P, _I, _I, _I, _I]),
    "eao_orb_stream_slot": (_I, [_P, _I, C.POINTER(OrbSlot)]),
    "eao_orb_stream_submit": (_I, [_P, _I, _I]),
    "eao_orb_stream_wait": (_I, [_P, _I]),
    "eao_orb_level": (_I, [_P, _I, _I, _I, C.POINTER(_I), C.POINTER(_I), _P]),
    "eao_orb_pyramid": (_I, [_P, _I, _I, C.POINTER(OrbLevelView)]),
    "eao_orb_set_keep_pyramid": (_I, [_P, _I]),
    "eao_orb_extract_ref": (_I, [_P, _P, _I, _I, _I, C.POINTER(_P), C.POINTER(_P), C.POINTER(_I)]),
    "eao_orb_level_candidates": (_I, [_P, _I, _I, _P, _I, C.POINTER(_I)]),
    "eao_orb_set_profiling": (_I, [_P, _I]),
    "eao_orb_last_timing": (_I, [_P, _P]),
    "eao_orb_lanes": (_I, [_I]),
    "eao_hamming_matrix": (_I, [_P, _I, _P, _I, _P]),
    "eao_hamming_best2": (_I, [_P, _I, _P, _I, _P, _P]),
    "eao_hamming_matrix_device": (_I, [_P, _I, _P, _I, _I, _P, _P]),
    "eao_hamming_best2_device": (_I, [_P, _I, _P, _I, _I, _P, _P, _P]),
    "eao_hamming_best2_sequence_device": (_I, [_P, _I, _P, _I, _P, _I, _P, _P]),
    "eao_search_by_projection_points": (_I, [C.POINTER(FrameView), _I, _P, _P, _P, _P, _P, _P, _P, C.c_float, C.c_float, _P, C.POINTER(_I)]),
    "eao_search_by_projection_frames": (_I, [C.POINTER(FrameView), _P, _P, _I, _P, _P, _P, _P, _P] + [C.c_float] * 7 + [_I, _I, _P, C.POINTER(_I)]),
    # the remaining guided searches: argument lists live in search.py (SEARCH_ARGTYPES), bound there
    "eao_search_by_projection_sim3": None, "eao_search_by_projection_kf": None, "eao_search_by_bow": None,
    "eao_search_for_triangulation": None, "eao_search_for_initialization": None, "eao_fuse_search": None, "eao_search_by_sim3": None,
    "eao_search_for_triangulation_batch": None, "eao_fuse_search_batch": None,
    # keyframe handles (round 5): argument lists live in search.py (HandleBinding)
    "eao_keyframe_create": None, "eao_keyframe_update_points": None, "eao_keyframe_destroy": None, "eao_keyframe_size": None,
    "eao_kf_search_by_bow": None, "eao_kf_search_for_triangulation": None, "eao_kf_fuse_search": None, "eao_kf_search_by_projection_sim3": None,
    "eao_kf_search_by_projection_kf": None, "eao_kf_search_for_initialization": None, "eao_kf_search_by_sim3": None,
    # the triangulation half of CreateNewMapPoints: argument lists live in search.py (TriangulationBinding)
    "eao_triangulate_matches_batch": None, "eao_keyframe_set_depth": None, "eao_kf_create_new_map_points": None,
    "eao_kf_last_triangulation_ms": (_I, [C.POINTER(C.c_float)]),
    # f1, second half (the device-resident tracked frame): argument lists live in tracker.py
    "eao_tracker_create": None, "eao_tracker_destroy": None, "eao_tracker_set_local_map": None, "eao_tracker_track_local_map": None, "eao_tracker_set_options": None, "eao_tracker_set_distortion": None,
    "eao_tracker_track_with_motion_model": None, "eao_tracker_track_reference_keyframe": None, "eao_abi_version": (_I, []),
    # f1 (Frame glue): argument lists live in frame.py
    "eao_frame_is_in_frustum": None, "eao_assign_features_to_grid": None, "eao_compute_stereo_from_rgbd": None, "eao_undistort_keypoints": None,
    "eao_compute_image_bounds": None,
    "eao_distinctive_descriptors": (_I, [_I, _P, _P, _P]),
    "eao_compute_stereo_matches": (_I, [_P, _P, _I, _I, _P, _P, _I, _P, _P, C.c_float, C.c_float, _P, _P]),
    "eao_pose_optimization": (_I, [C.POINTER(PoseProblem), C.POINTER(PoseResult)]),
    "eao_pose_optimization_batch": (_I, [C.POINTER(PoseProblem), C.c_int32, C.POINTER(PoseResult)]),
    "eao_local_ba": (_I, [C.POINTER(BAProblem), _P, C.POINTER(BAResult)]),
    "eao_local_ba_batch": (_I, [C.POINTER(BAProblem), _I, _P, C.POINTER(BAResult)]),
    "eao_bundle_adjustment": (_I, [C.POINTER(BAProblem), _I, _P, C.POINTER(BAResult)]),
    "eao_bundle_adjustment_planes": (_I, [C.POINTER(BAProblem), C.POINTER(BAPlanes), _I, _P, C.POINTER(BAResult), _P]),
    "eao_last_lm_trace": (_I, [_P, _P, _P, _I, C.POINTER(_I)]),
    "eao_last_pose_rounds": (_I, [_I, _P, _P, _P, _I, C.POINTER(_I), _P, C.POINTER(_I)]),
    "eao_last_lm_timing": (_I, [C.POINTER(C.c_float), C.POINTER(_I)]),
    "eao_optimize_sim3": (_I, [C.POINTER(Sim3Problem), C.POINTER(Sim3Result)]),
    "eao_optimize_sim3_batch": (_I, [C.POINTER(Sim3Problem), _I, C.POINTER(Sim3Result)]),
    "eao_sim3_solver_iterate": (_I, [C.POINTER(Sim3SolverProblem), _I, _I, C.POINTER(Sim3SolverState), _P, _I, C.POINTER(Sim3SolverResult)]),
    "eao_sim3_solver_iterate_batch": (_I, [_I, C.POINTER(Sim3SolverProblem), _P, _P, C.POINTER(Sim3SolverState), _P, _P, C.POINTER(Sim3SolverResult)]),
    "eao_initializer_initialize": (_I, [C.POINTER(InitializerProblem), _P, _I, C.POINTER(InitializerResult)]),
    "eao_initializer_last_kernel_ms": (_I, [_P]),
    "eao_pnp_solver_iterate": (_I, [C.POINTER(PnpSolverProblem), _I, _I, _I, C.POINTER(PnpSolverState), _P, _I, C.POINTER(PnpSolverResult)]),
    "eao_pnp_solver_iterate_batch": (_I, [_I, C.POINTER(PnpSolverProblem), _P, _P, _P, C.POINTER(PnpSolverState), _P, _P, C.POINTER(PnpSolverResult)]),
    "eao_pnp_solver_last_kernel_ms": (_I, [_P]),
    "eao_optimize_essential_graph": (_I, [C.POINTER(EssentialGraphProblem), C.POINTER(EssentialGraphResult)]),
    "eao_essential_graph_plan": (_I, [C.POINTER(EssentialGraphProblem), _P, _P, _P, _I]),
    "eao_vocabulary_create": (_I, [C.POINTER(VocabularyDesc), C.POINTER(_P)]),
    "eao_vocabulary_destroy": (None, [_P]),
    "eao_vocabulary_info": (_I, [_P, C.POINTER(_I), C.POINTER(_I), C.POINTER(_I), C.POINTER(_I)]),
    "eao_vocabulary_transform": (_I, [_P, _P, _I, _I, C.POINTER(BowResult)]),
    "eao_vocabulary_transform_batch": (_I, [_P, _I, _P, _P, _I, C.POINTER(BowResult)]),
    "eao_vocabulary_transform_device": (_I, [_P, _P, _P, _I, _I, C.POINTER(BowResult), _P]),
    "eao_bow_score_l1": (_I, [_I, _P, _P, _I, _P, _P, _P, _P]),
    "eao_keyframe_db_create": (_I, [_I, C.POINTER(_P)]),
    "eao_keyframe_db_destroy": (None, [_P]),
    "eao_keyframe_db_clear": (_I, [_P]),
    "eao_keyframe_db_info": (_I, [_P, C.POINTER(_I), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "eao_keyframe_db_add": (_I, [_P, C.c_uint64, _I, _P, _P]),
    "eao_keyframe_db_erase": (_I, [_P, C.c_uint64]),
    "eao_keyframe_db_intersect": (_I, [_P, _I, _P, _P, _I, _P, _P, _P, _P, C.POINTER(_I)]),
    "eao_keyframe_db_query_scores": (_I, [_P, C.POINTER(KeyFrameDbQuery), _I, C.POINTER(KeyFrameDbScored)]),
    "eao_keyframe_db_candidates": (_I, [_P, _I, C.c_uint64, _I, C.c_float, _I, _P, _P, _P, _P, _P, C.POINTER(_I), _P, _P, C.POINTER(_I)]),
    "eao_plane_map_create": (_I, [C.POINTER(_P)]),
    "eao_plane_map_destroy": (None, [_P]),
    "eao_plane_map_clear": (_I, [_P]),
    "eao_plane_map_info": (_I, [_P, C.POINTER(_I), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "eao_plane_map_add": (_I, [_P, C.c_uint64, _P, _I, _P, _P]),
    "eao_plane_map_update_boundary": (_I, [_P, C.c_uint64, _I, _P, _P]),
    "eao_plane_map_set_world_pos": (_I, [_P, C.c_uint64, _P]),
    "eao_plane_map_erase": (_I, [_P, C.c_uint64]),
    "eao_plane_map_boundary": (_I, [_P, C.c_uint64, _I, _P, C.POINTER(_I), _P]),
    "eao_plane_map_associate": (_I, [_P, _I, _P, _P, _P, _I, _P, C.c_float, C.c_float, _P, _P, _P, _P, _P]),
    "eao_plane_seg_cfg_default": (None, [C.POINTER(PlaneSegCfg), _I, _I, C.c_float, C.c_float, C.c_float, C.c_float]),
    "eao_plane_seg_create": (_I, [C.POINTER(PlaneSegCfg), C.POINTER(_P)]),
    "eao_plane_seg_destroy": (None, [_P]),
    "eao_plane_seg_run": (_I, [_P, _P, _I]),
    "eao_plane_seg_set_profiling": (_I, [_P, _I]),
    "eao_plane_seg_last_timing": (_I, [_P, _P]),
    "eao_plane_seg_info": (_I, [_P, C.POINTER(_I), C.POINTER(_I), C.POINTER(_I), C.POINTER(_I)]),
    "eao_plane_seg_planes": (_I, [_P, _I, _P, C.POINTER(_I)]),
    "eao_plane_seg_cloud": (_I, [_P, _I, _I, _P, C.POINTER(_I)]),
    "eao_plane_seg_membership": (_I, [_P, _P]),
    "eao_plane_seg_blocks": (_I, [_P, _I, _P, C.POINTER(_I)]),
    "eao_plane_seg_middle": (_I, [_P, _P, _I, _P, C.POINTER(_I), _I, _P, C.POINTER(_I)]),
    "eao_plane_map_add_from_seg": (_I, [_P, C.c_uint64, _P, _P, _I, _P]),
    "eao_plane_map_update_boundary_from_seg": (_I, [_P, C.c_uint64, _P, _I, _P]),
    "eao_iforest_scores_batch": (_I, [_I, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int64, _P]),
    "eao_object_iforest_outliers_batch": (_I, [_I, _P, _P, _P, _I, _P, _P, _P]),
    "eao_iforest_set_profiling": (_I, [_I]),
    "eao_iforest_last_kernel_ms": (_I, [_P]),
    "eao_iforest_last_stage_us": (_I, [_P]),
    "eao_object_np_counts_batch": (_I, [_I, _P, _P, _I, _P, _P, _P, _I, _P, _P, _P, _P]),
    "eao_object_np_association_batch": (_I, [_I, _P, _P, _I, _P, _P, _P, _I, _P, _P, _P, _P, _P]),
    "eao_object_project_rects_batch": (_I, [_I, _P, _P, _P] + [C.c_float] * 4 + [_I, _I, _P, _P, _P]),
    "eao_object_assoc_set_profiling": (_I, [_I]),
    "eao_object_assoc_last_kernel_ms": (_I, [_P]),
    "eao_frame_objects_batch": (_I, [_I, C.POINTER(FrameObjectsDesc), C.POINTER(FrameObjectsOut)]),
    "eao_frame_objects": (_I, [C.POINTER(FrameObjectsDesc), C.POINTER(FrameObjectsOut)]),
    "eao_frame_objects_set_profiling": (_I, [_I]),
    "eao_frame_objects_last_kernel_ms": (_I, [_P]),
    "eao_object_cuboids_batch": (_I, [_I, C.POINTER(ObjectCuboidDesc), _P]),
    "eao_object_cuboids": (_I, [C.POINTER(ObjectCuboidDesc), _P]),
    "eao_object_overlaps": (_I, [_I, _P, _P, _P, _P]),
    "eao_object_cuboid_set_profiling": (_I, [_I]),
    "eao_object_cuboid_last_kernel_ms": (_I, [_P]),
    "eao_object_points_update_batch": (_I, [_I, C.POINTER(ObjectPointsDesc), C.POINTER(ObjectPointsOut)]),
    "eao_object_points_update": (_I, [C.POINTER(ObjectPointsDesc), C.POINTER(ObjectPointsOut)]),
    "eao_object_points_set_profiling": (_I, [_I]),
    "eao_object_points_last_kernel_ms": (_I, [_P]),
    "eao_object_update_chain_batch": (_I, [_I, C.POINTER(ObjectChainDesc), C.POINTER(ObjectChainOut)]),
    "eao_object_update_chain": (_I, [C.POINTER(ObjectChainDesc), C.POINTER(ObjectChainOut)]),
    "eao_object_chain_set_profiling": (_I, [_I]),
    "eao_object_chain_last_kernel_ms": (_I, [_P]),
    "eao_yolox_cfg_default": (None, [C.POINTER(YoloxCfg)]),
    "eao_yolox_create": (_I, [C.POINTER(YoloxCfg), C.POINTER(_P)]),
    "eao_yolox_destroy": (None, [_P]),
    "eao_yolox_preprocess": (_I, [_P, _P, _I, _I, _I, C.c_int64, _I, _I, _P, _I]),
    "eao_yolox_preprocess_device": (_I, [_P, _P, _I, _I, _I, C.c_int64, _I, _I, _P, _P, _I, _P]),
    "eao_yolox_decode": (_I, [_P, _P, _I, _P, _P, _P, _I, _P, _P, _P]),
    "eao_yolox_decode_device": (_I, [_P, _P, _I, _P, _P, _P, _I, _P, _P, _P, _P]),
    "eao_yolox_buffers": (_I, [_P, C.POINTER(_P), C.POINTER(_P), C.POINTER(_P)]),
    "eao_yolox_head": (_I, [_P, _P, _I, _P, _P]),
    "eao_yolox_blob": (_I, [_P, _I, _P]),
    "eao_yolox_proposals": (_I, [_P, _I, _P, _I, C.POINTER(_I)]),
    "eao_yolox_set_profiling": (_I, [_P, _I]),
    "eao_yolox_last_kernel_ms": (_I, [_P, _P]),
    "eao_detnet_create": (_I, [_P, C.c_int64, _I, _I, C.POINTER(_P)]),
    "eao_detnet_create_from_file": (_I, [C.c_char_p, _I, _I, C.POINTER(_P)]),
    "eao_detnet_destroy": (None, [_P]),
    "eao_detnet_info": (_I, [_P, C.POINTER(DetnetDesc)]),
    "eao_detnet_forward": (_I, [_P, _P, _P, _I, _P]),
    "eao_detnet_tensor": (_I, [_P, _I, _I, _P]),
    "eao_detnet_set_tensor": (_I, [_P, _I, _I, _P]),
    "eao_detnet_set_profiling": (_I, [_P, _I]),
    "eao_detnet_last_op_ms": (_I, [_P, _P, _I]),
    "eao_bundle_adjustment_plan": (_I, [_I, _I, _P, _P, _I, _P, _P, _P, _I, _P, _I, _P, _I, _P, _I, _P, _I, _P, _I]),
}

_lib = None


def load():
    """Load the shared object (after torch, if torch is in the process, so that both resolve the same
    libamdhip64.so.7 -- see DESIGN.md 'process model')."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(hipcc --offload-arch=gfx950); there is no CPU fallback" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        for name, sig in SYMBOLS.items():
            fn = getattr(L, name)  # AttributeError = ABI drift, fail loudly
            if sig is not None:
                fn.restype, fn.argtypes = sig
        _lib = L
    return _lib


def check(status):
    if status != EAO_OK:
        raise EaoError(status, load().eao_last_error().decode("utf-8", "replace"))


def ptr(a):
    return None if a is None else a.ctypes.data
