#!/usr/bin/env python3
"""Reads the reference's numeric literals (thresholds, gates, iteration counts) out of its text into tests/golden/<feature>_constants.json: name, literal and
file:line only.  Every feature has one table here; tests/test_reference_literals.py holds each fixture to its table (and, where a reference tree is present, to the
text), and the feature tests hold our code -- kernel constant blocks, internal headers, adapters, Python mirrors, yardsticks -- to the fixture through literals().

    python tools/reference_literals.py <reference tree> [feature ...]          # writes the fixtures (every feature by default)
    python tools/reference_literals.py <reference tree> --check [feature ...]  # compares, writes nothing

ref_constants.json also carries a C type and a note per row and comes with two generated headers: tools/gen_ref_constants.py writes it, through parse() here.
"""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def one_file(rel, rows):
    """(name, line, regex) rows of a single-file feature -> (name, file, line, regex, group)"""
    return [(name, rel, line, rx, 1) for name, line, rx in rows]


def one_group(rows):
    """(name, file, line, regex) rows -> (name, file, line, regex, group)"""
    return [row + (1,) for row in rows]


_ORBMATCHER, _OPTIMIZER, _ORBEXTRACTOR = "src/ORBmatcher.cc", "src/Optimizer.cc", "src/ORBextractor.cc"
_LEVENBERG = "Thirdparty/g2o/g2o/core/optimization_algorithm_levenberg.cpp"
_FRAME, _FITTER, _PARAMS = "src/Frame.cc", "include/PEAC/AHCPlaneFitter.hpp", "include/PEAC/AHCParamSet.hpp"
_N = r"([0-9.e+-]+)"
_R1 = r"float r1 = %s \* m \* \(m \+ n \+ 1\) - %s \* sqrt\(m \* n \* \(m \+ n \+ 1\) / %s\);"
_R2 = r"float r2 = %s \* m \* \(m \+ n \+ 1\) \+ %s \* sqrt\(m \* n \* \(m \+ n \+ 1\) / %s\);"
_NUM, _GRP = r"[0-9.]+", r"([0-9.]+)"
_NUMF = r"([0-9.]+f?)"
_PNP_DEFAULTS = r"double probability = %s, int minInliers = %s , int maxIterations = %s, int minSet = %s, float epsilon = %s," % ((_NUMF,) * 5)
_PNP_RELOC = r"SetRansacParameters\(%s, %s, %s, %s, %s, %s\);" % ((_NUMF,) * 6)

_YOLOX_MEAN = r"std::vector<float> mean = \{%s, %s, %s\};" % ((_GRP,) * 3)
_YOLOX_STD = r"std::vector<float> std = \{%s, %s, %s\};" % ((_GRP,) * 3)
_YOLOX_STRIDES = r"std::vector<int> strides = \{(\d+), (\d+), (\d+)\};"
_YOLOX_CLASSES = r"if \(" + " && ".join([r"objInfo\.label != (\d+)"] * 14) + r"\)"

# feature -> rows of (name, file, line, the expression around the literal, the capture group that holds it)
TABLES = {
    # the hot path's thresholds, gates and schedules (tools/gen_ref_constants.py adds a C type and a note to each and emits the two ref_constants.inc)
    "ref": one_group([
        ("TH_HIGH", _ORBMATCHER, 37, r"const int ORBmatcher::TH_HIGH = (\d+);"),
        ("TH_LOW", _ORBMATCHER, 38, r"const int ORBmatcher::TH_LOW = (\d+);"),
        ("HISTO_LENGTH", _ORBMATCHER, 39, r"const int ORBmatcher::HISTO_LENGTH = (\d+);"),
        ("VIEWCOS_NARROW", _ORBMATCHER, 133, r"if\(viewCos>([\d.]+)\)"),
        ("RADIUS_NARROW", _ORBMATCHER, 134, r"return ([\d.]+);"),
        ("RADIUS_WIDE", _ORBMATCHER, 136, r"return ([\d.]+);"),
        ("EPIPOLAR_CHI2", _ORBMATCHER, 156, r"return dsqr<([\d.]+)\*pKF2->mvLevelSigma2"),
        ("FUSE_CHI2_STEREO", _ORBMATCHER, 925, r"mvInvLevelSigma2\[kpLevel\]>([\d.]+)\)"),
        ("FUSE_CHI2_MONO", _ORBMATCHER, 936, r"mvInvLevelSigma2\[kpLevel\]>([\d.]+)\)"),
        ("GBA_HUBER2_MONO", _OPTIMIZER, 98, r"const float thHuber2D = sqrt\(([\d.]+)\);"),
        ("GBA_HUBER2_STEREO", _OPTIMIZER, 99, r"const float thHuber3D = sqrt\(([\d.]+)\);"),
        ("PLANE_ANGLE_INFO", _OPTIMIZER, 464, r"double angleInfo = ([\d.]+) / \(1\.0 \* 1\.0\);"),
        ("PLANE_DIST_INFO_ROOT", _OPTIMIZER, 465, r"double disInfo = ([\d.]+) \* 100\.0;"),
        ("PLANE_CHI2", _OPTIMIZER, 466, r"double planeChi = ([\d.]+);"),
        ("POSE_HUBER2_MONO", _OPTIMIZER, 361, r"const float deltaMono = sqrt\(([\d.]+)\);"),
        ("POSE_HUBER2_STEREO", _OPTIMIZER, 362, r"const float deltaStereo = sqrt\(([\d.]+)\);"),
        ("POSE_CHI2_MONO", _OPTIMIZER, 539, r"const float chi2Mono\[4\]=\{([\d.]+),\1,\1,\1\};"),
        ("POSE_CHI2_STEREO", _OPTIMIZER, 540, r"const float chi2Stereo\[4\]=\{([\d.]+),\1,\1, \1\};"),
        ("POSE_ROUNDS", _OPTIMIZER, 541, r"const int its\[(\d+)\]=\{10,10,10,10\};"),
        ("POSE_ITS", _OPTIMIZER, 541, r"const int its\[4\]=\{(\d+),\1,\1,\1\};"),
        ("POSE_UNROBUST_ROUND", _OPTIMIZER, 620, r"if \(it == (\d+)\)"),
        ("LBA_HUBER2_MONO", _OPTIMIZER, 820, r"const float thHuberMono = sqrt\(([\d.]+)\);"),
        ("LBA_HUBER2_STEREO", _OPTIMIZER, 821, r"const float thHuberStereo = sqrt\(([\d.]+)\);"),
        ("LBA_ITS_FIRST", _OPTIMIZER, 966, r"optimizer\.optimize\((\d+)\);"),
        ("LBA_CHI2_MONO", _OPTIMIZER, 986, r"if\(e->chi2\(\)>([\d.]+) \|\| !e->isDepthPositive\(\)\)"),
        ("LBA_CHI2_STEREO", _OPTIMIZER, 1002, r"if\(e->chi2\(\)>([\d.]+) \|\| !e->isDepthPositive\(\)\)"),
        ("LBA_ITS_SECOND", _OPTIMIZER, 1027, r"optimizer\.optimize\((\d+)\);"),
        ("LM_TAU", _LEVENBERG, 47, r"_tau = ([\de.-]+);"),
        ("LM_MAX_TRIALS", _LEVENBERG, 51, r"\"maxTrialsAfterFailure\", (\d+)\)"),
        ("LM_NI", _LEVENBERG, 52, r"_ni=([\d.]+);"),
        ("PATCH_SIZE", _ORBEXTRACTOR, 72, r"const int PATCH_SIZE = (\d+);"),
        ("HALF_PATCH_SIZE", _ORBEXTRACTOR, 73, r"const int HALF_PATCH_SIZE = (\d+);"),
        ("EDGE_THRESHOLD", _ORBEXTRACTOR, 74, r"const int EDGE_THRESHOLD = (\d+);"),
        ("FAST_CELL", _ORBEXTRACTOR, 769, r"const float W = (\d+);"),
    ]),
    # the triangulation loop of LocalMapping::CreateNewMapPoints
    "triangulation": one_file("src/LocalMapping.cc", [
        ("RATIO_FACTOR_BASE", 236, r"ratioFactor = ([0-9.]+)f\*mpCurrentKeyFrame->mfScaleFactor"),
        ("LOW_PARALLAX_COS", 323, r"cosParallaxRays<([0-9.]+)\)"),
        ("CHI2_MONO", 378, r"\(errX1\*errX1\+errY1\*errY1\)>([0-9.]+)\*sigmaSquare1"),
        ("CHI2_STEREO", 389, r"\+errX1_r\*errX1_r\)>([0-9.]+)\*sigmaSquare1"),
        ("CHI2_MONO", 404, r"\(errX2\*errX2\+errY2\*errY2\)>([0-9.]+)\*sigmaSquare2"),
        ("CHI2_STEREO", 415, r"\+errX2_r\*errX2_r\)>([0-9.]+)\*sigmaSquare2"),
    ]),
    # Initializer
    "initializer": one_file("src/Initializer.cc", [
        ("RATIO_H", 115, r"if\(RH>([0-9.]+)\)"),
        ("MIN_PARALLAX", 116, r"ReconstructH\(.*vbTriangulated,([0-9.]+),[0-9]+\)"),
        ("MIN_TRIANGULATED", 116, r"ReconstructH\(.*vbTriangulated,[0-9.]+,([0-9]+)\)"),
        ("MIN_PARALLAX", 118, r"ReconstructF\(.*vbTriangulated,([0-9.]+),[0-9]+\)"),
        ("MIN_TRIANGULATED", 118, r"ReconstructF\(.*vbTriangulated,[0-9.]+,([0-9]+)\)"),
        ("CHI2_H", 333, r"const float th = ([0-9.]+);"),
        ("CHI2_F", 408, r"const float th = ([0-9.]+);"),
        ("CHI2_SCORE", 409, r"const float thScore = ([0-9.]+);"),
        ("REPROJ_FACTOR", 494, r"vP3D1, ([0-9.]+)\*mSigma2"),
        ("MIN_GOOD_FRACTION", 504, r"static_cast<int>\(([0-9.]+)\*N\)"),
        ("SIMILAR", 507, r"nGood1>([0-9.]+)\*maxGood"),
        ("DEGENERATE", 597, r"d1/d2<([0-9.]+) \|\| d2/d3<\1\)"),
        ("REPROJ_FACTOR", 703, r"vP3Di, ([0-9.]+)\*mSigma2"),
        ("SECOND_BEST", 721, r"secondBestGood<([0-9.]+)\*bestGood"),
        ("MIN_GOOD_FRACTION", 721, r"bestGood>([0-9.]+)\*N\)"),
        ("COS_PARALLAX", 857, r"cosParallax<([0-9.]+)\)"),
        ("COS_PARALLAX", 863, r"cosParallax<([0-9.]+)\)"),
        ("COS_PARALLAX", 892, r"cosParallax<([0-9.]+)\)"),
        ("PARALLAX_RANK", 900, r"min\(([0-9]+),int\(vCosParallax\.size\(\)-1\)\)"),
    ]),
    # PnPsolver and its call in Tracking::Relocalization
    "pnp_solver": [
        ("GN_ITERATIONS", "src/PnPsolver.cc", 843, r"const int iterations_number = ([0-9]+);", 1),
        ("ALPHA_ONE", "src/PnPsolver.cc", 432, r"a\[0\] = " + _NUMF + r" - a\[1\] - a\[2\] - a\[3\];", 1),
        ("L_TWO", "src/PnPsolver.cc", 790, r"row\[1\] = " + _NUMF + r" \* dot\(dv\[0\]\[i\], dv\[1\]\[i\]\);", 1),
        ("L_TWO", "src/PnPsolver.cc", 792, r"row\[3\] = " + _NUMF + r" \* dot", 1),
        ("L_TWO", "src/PnPsolver.cc", 793, r"row\[4\] = " + _NUMF + r" \* dot", 1),
        ("L_TWO", "src/PnPsolver.cc", 795, r"row\[6\] = " + _NUMF + r" \* dot", 1),
        ("L_TWO", "src/PnPsolver.cc", 796, r"row\[7\] = " + _NUMF + r" \* dot", 1),
        ("L_TWO", "src/PnPsolver.cc", 797, r"row\[8\] = " + _NUMF + r" \* dot", 1),
        ("DEFAULT_PROBABILITY", "include/PnPsolver.h", 67, _PNP_DEFAULTS, 1),
        ("DEFAULT_MIN_INLIERS", "include/PnPsolver.h", 67, _PNP_DEFAULTS, 2),
        ("DEFAULT_MAX_ITERATIONS", "include/PnPsolver.h", 67, _PNP_DEFAULTS, 3),
        ("DEFAULT_MIN_SET", "include/PnPsolver.h", 67, _PNP_DEFAULTS, 4),
        ("DEFAULT_EPSILON", "include/PnPsolver.h", 67, _PNP_DEFAULTS, 5),
        ("DEFAULT_TH2", "include/PnPsolver.h", 68, r"float th2 = " + _NUMF + r"\);", 1),
        ("RELOC_PROBABILITY", "src/Tracking.cc", 2831, _PNP_RELOC, 1),
        ("RELOC_MIN_INLIERS", "src/Tracking.cc", 2831, _PNP_RELOC, 2),
        ("RELOC_MAX_ITERATIONS", "src/Tracking.cc", 2831, _PNP_RELOC, 3),
        ("RELOC_MIN_SET", "src/Tracking.cc", 2831, _PNP_RELOC, 4),
        ("RELOC_EPSILON", "src/Tracking.cc", 2831, _PNP_RELOC, 5),
        ("RELOC_TH2", "src/Tracking.cc", 2831, _PNP_RELOC, 6),
    ],
    # KeyFrameDatabase: DetectLoopCandidates, then DetectRelocalizationCandidates
    "keyframe_database": one_file("src/KeyFrameDatabase.cc", [
        ("MIN_COMMON_WORDS_FACTOR", 119, r"int minCommonWords = maxCommonWords\*([0-9.]+f);"),
        ("N_NEIGHBOURS", 150, r"GetBestCovisibilityKeyFrames\(([0-9]+)\);"),
        ("MIN_SCORE_TO_RETAIN_FACTOR", 175, r"float minScoreToRetain = ([0-9.]+f)\*bestAccScore;"),
        ("MIN_COMMON_WORDS_FACTOR", 234, r"int minCommonWords = maxCommonWords\*([0-9.]+f);"),
        ("N_NEIGHBOURS", 264, r"GetBestCovisibilityKeyFrames\(([0-9]+)\);"),
        ("MIN_SCORE_TO_RETAIN_FACTOR", 289, r"float minScoreToRetain = ([0-9.]+f)\*bestAccScore;"),
    ]),
    # the plane association (Map::AssociatePlanesByBoundary)
    "plane_association": one_file("src/Map.cc", [
        ("DIS_TH", 22, r"mfDisTh = ([0-9.]+);"),
        ("ANGLE_TH", 23, r"mfAngleTh = ([0-9.]+);"),
        ("NO_DISTANCE", 219, r"double res = ([0-9.]+);"),
    ]),
    # the plane segmentation (Frame::ComputePlanesFromPEAC)
    "plane_segmentation": one_group([
        ("DEPTH_MAX", _FRAME, 396, r"d > " + _N + r" \|\|"),
        ("DEPTH_MIN", _FRAME, 396, r"d < " + _N + r" \)"),
        ("LEAF", _FRAME, 436, r"setLeafSize\(" + _N + r","),
        ("SEEN_DIST", _FRAME, 362, r"d > " + _N + r" \|\|"),
        ("SEEN_ANGLE", _FRAME, 365, r"angle < " + _N + r" &&"),
        ("MAX_STEP", _FITTER, 153, r"maxStep\(" + _N + r"\)"),
        ("MIN_SUPPORT", _FITTER, 153, r"minSupport\(" + _N + r"\)"),
        ("WINDOW", _FITTER, 154, r"windowWidth\(" + _N + r"\)"),
        ("WINDOW_HEIGHT", _FITTER, 154, r"windowHeight\(" + _N + r"\)"),
        ("TRAIL_STOP", _FITTER, 443, r"trail<=(-[0-9]+)\)"),
        ("DIST_FACTOR", _FITTER, 453, r"<([0-9]+)\*pl\.mse"),
        ("DIST_EPS", _FITTER, 453, r"pl\.mse\+" + _N + r"\)"),
        ("DEPTH_SIGMA", _PARAMS, 68, r"depthSigma\(" + _N + r"\)"),
        ("STD_TOL_INIT", _PARAMS, 69, r"stdTol_init\(" + _N + r"\)"),
        ("STD_TOL_MERGE", _PARAMS, 69, r"stdTol_merge\(" + _N + r"\)"),
        ("Z_NEAR", _PARAMS, 70, r"z_near\(" + _N + r"\)"),
        ("Z_FAR", _PARAMS, 70, r"z_far\(" + _N + r"\)"),
        ("ANGLE_NEAR_DEG", _PARAMS, 71, r"angle_near\(MACRO_DEG2RAD\(" + _N + r"\)\)"),
        ("ANGLE_FAR_DEG", _PARAMS, 71, r"angle_far\(MACRO_DEG2RAD\(" + _N + r"\)\)"),
        ("SIMILARITY_MERGE_DEG", _PARAMS, 72, r"similarityTh_merge\(std::cos\(MACRO_DEG2RAD\(" + _N + r"\)\)\)"),
        ("SIMILARITY_REFINE_DEG", _PARAMS, 73, r"similarityTh_refine\(std::cos\(MACRO_DEG2RAD\(" + _N + r"\)\)\)"),
        ("DEPTH_ALPHA", _PARAMS, 74, r"depthAlpha\(" + _N + r"\)"),
        ("DEPTH_CHANGE_TOL", _PARAMS, 74, r"depthChangeTol\(" + _N + r"\)"),
    ]),
    # Object_Map::IsolationForestDeleteOutliers
    "isolation_forest": one_file("src/Object.cc", [
        ("EXEMPT_CLASS_A", 1245, r"\(this->mnClass == (\d+)\) \|\| \(this->mnClass == \d+\) \|\| \(this->mnClass == \d+\)"),
        ("EXEMPT_CLASS_B", 1245, r"\(this->mnClass == \d+\) \|\| \(this->mnClass == (\d+)\) \|\| \(this->mnClass == \d+\)"),
        ("EXEMPT_CLASS_C", 1245, r"\(this->mnClass == \d+\) \|\| \(this->mnClass == \d+\) \|\| \(this->mnClass == (\d+)\)"),
        ("THRESHOLD", 1248, r"float th = ([0-9.]+);"),
        ("THRESHOLD_CLASS", 1249, r"if \(this->mnClass == (\d+)\)"),
        ("THRESHOLD_OF_CLASS", 1250, r"th = ([0-9.]+);"),
        ("MIN_POINTS", 1256, r"mvpMapObjectMappoints.size\(\) < (\d+)\)"),
        ("TREE_COUNT", 1296, r"forest.Build\((\d+), \d+, data,"),
        ("SEED", 1296, r"forest.Build\(\d+, (\d+), data,"),
        ("SAMPLE_DIVISOR", 1296, r"\(\(int\)mvpMapObjectMappoints.size\(\) / (\d+)\)"),
    ]),
    # Object_2D::NoParaDataAssociation
    "object_association": one_file("src/Object.cc", [
        ("MIN_DET_POINTS", 760, r"if \(m < (\d+)\)"),
        ("MIN_MAP_POINTS", 764, r"if \(n < (\d+)\)"),
        ("SAMPLE_RATIO", 776, r"if \(n > (\d+) \* m\)"),
        ("SAMPLE_RATIO_N", 778, r"n = (\d+) \* m;"),
        ("HALF", 942, _R1 % (_GRP, _NUM, _NUM)),
        ("CRITICAL", 942, _R1 % (_NUM, _GRP, _NUM)),
        ("VARIANCE_DIVISOR", 942, _R1 % (_NUM, _NUM, _GRP)),
        ("HALF_R2", 943, _R2 % (_GRP, _NUM, _NUM)),
        ("CRITICAL_R2", 943, _R2 % (_NUM, _GRP, _NUM)),
        ("VARIANCE_DIVISOR_R2", 943, _R2 % (_NUM, _NUM, _GRP)),
    ]),
    # a frame's 2D objects: steps 4, 5 and 6 of the object layer in Tracking::TrackWithMotionModel and Object_2D::RemoveOutliersByBoxPlot
    "frame_objects": one_group([
        ("BOXPLOT_MIN_POINTS", "src/Tracking.cc", 1782, r"if \(obj->Obj_c_MapPonits\.size\(\) < (\d+)\)"),
        ("QUARTILE_DIVISOR", "src/Object.cc", 134, r"float Q1 = z_c\[\(int\)\(z_c\.size\(\) / (\d+)\)\];"),
        ("IQR_FACTOR", "src/Object.cc", 139, r"float max_th = Q3 \+ ([0-9.]+) \* IQR;"),
        ("CROWD_RATIO", "src/Tracking.cc", 1876, r"mBoxRect\) > ([0-9.]+)\)"),
        ("CROWD_MAX", "src/Tracking.cc", 1880, r"if \(num > (\d+)\)"),
        ("LARGE_AREA_RATIO", "src/Tracking.cc", 1893, r"\(image\.cols \* image\.rows\) > ([0-9.]+)\)"),
        ("FEW_POINTS", "src/Tracking.cc", 1897, r"Obj_c_MapPonits\.size\(\) < (\d+)\)"),
        ("FEW_POINTS_ON_EDGE", "src/Tracking.cc", 1901, r"&& \(objs_2d\[f\]->Obj_c_MapPonits\.size\(\) < (\d+)\)\)"),
        ("FEW_POINTS_EDGE_PIXELS", "src/Tracking.cc", 1903, r"\(objs_2d\[f\]->mBox\.x < (\d+)\)"),
        ("ON_EDGE_PIXELS", "src/Tracking.cc", 1912, r"\(objs_2d\[f\]->mBox\.x < (\d+)\)"),
        ("SAME_OBJECT_IOU", "src/Tracking.cc", 1929, r"mBoxRect\) > ([0-9.]+)\)"),
        ("SURROUND_IOU", "src/Tracking.cc", 1937, r"mBoxRect\) > ([0-9.]+)\)"),
        ("SURROUND_RATIO", "src/Tracking.cc", 1939, r"mBoxRect\) > ([0-9.]+)\)"),
        ("SURROUND_RATIO", "src/Tracking.cc", 1941, r"mBoxRect\) > ([0-9.]+)\)"),
        ("FEATURE_RECT_MIN_POINTS", "src/Tracking.cc", 1830, r"if \(x_pt\.size\(\) < (\d+)\)"),
    ]),
    # a map object's cuboid: Object_Map::ComputeMeanAndStandard, UpdateObjPose and WhetherOverlap.  CORNER_<x><y><z>: the number of the corner that takes the
    # named extremum on each axis (both the world-frame and the object-frame assignments)
    "object_cuboid": [
        ("FEW_FRAMES", "src/Object.cc", 1071, r"if \(this->mObjectFrame\.size\(\) < (\d+)\)", 1),
        ("CENTER_DIVISOR", "src/Object.cc", 1093, r"\(x_max \+ x_min\) / (\d+), \(y_max \+ y_min\) / (\d+), \(z_max \+ z_min\) / (\d+)\);", 1),
    ] + [("CORNER_%s" % key, "src/Object.cc", first + k, r"mCuboid3D\.corner_(\d+)%s = %sEigen::Vector3d\(x_%s%s, y_%s%s, z_%s%s\);"
          % ((tail, mid) + tuple(v for axis in key.split("_") for v in (axis.lower(), suffix))), 1)
         for first, tail, mid, suffix in ((1106, "", "", ""), (1115, "_w", "", ""), (1160, "", r"this->mCuboid3D\.pose \* ", "_obj"),
                                          (1170, "_w", r"this->mCuboid3D\.pose_without_yaw \* ", "_obj"))
         for k, key in enumerate(["MIN_MIN_MIN", "MAX_MIN_MIN", "MAX_MAX_MIN", "MIN_MAX_MIN", "MIN_MIN_MAX", "MAX_MIN_MAX", "MAX_MAX_MAX", "MIN_MAX_MAX"])] + [
        ("CORNER_FAR_A", "src/Object.cc", 1185, r"cuboidCenter = \(mCuboid3D\.corner_(\d+) \+ mCuboid3D\.corner_(\d+)\) / (\d+);", 1),
        ("CORNER_FAR_B", "src/Object.cc", 1185, r"cuboidCenter = \(mCuboid3D\.corner_(\d+) \+ mCuboid3D\.corner_(\d+)\) / (\d+);", 2),
        ("CENTER_DIVISOR", "src/Object.cc", 1185, r"cuboidCenter = \(mCuboid3D\.corner_(\d+) \+ mCuboid3D\.corner_(\d+)\) / (\d+);", 3),
        ("WITHOUT_YAW_X_FROM_CENTER3D", "src/Object.cc", 2293, r"Twobj_without_yaw\.at<float>\(0, 3\) = mCenter3D\.at<float>\((\d+)\);", 1),
        ("WITHOUT_YAW_Y_FROM_CUBOID_CENTER", "src/Object.cc", 2294, r"Twobj_without_yaw\.at<float>\(1, 3\) = mCuboid3D\.cuboidCenter\[(\d+)\];", 1),
        ("WITHOUT_YAW_Z_FROM_CENTER3D", "src/Object.cc", 2295, r"Twobj_without_yaw\.at<float>\(2, 3\) = mCenter3D\.at<float>\((\d+)\);", 1),
        ("OVERLAP_HALF", "src/Object.cc", 1961, r"float sum_lenth_half = mCuboid3D\.lenth / (\d+) \+ CompareObj->mCuboid3D\.lenth / (\d+);", 1),
        ("OVERLAP_HALF", "src/LocalMapping.cc", 862, r"float sum_lenth_half = Obj->mCuboid3D\.lenth/(\d+) \+ Obj2->mCuboid3D\.lenth/(\d+);", 1),
    ],
    # the update of a map object's point list: Object_Map::DataAssociateUpdate, MergeTwoMapObjs
    "object_points": [
        ("MIN_IOU", "src/Object.cc", 1434, r"if \(\(fIou < ([0-9.]+)\) && \(fIou2 < ([0-9.]+)\)\)", 1),
        ("MIN_IOU_FORMER", "src/Object.cc", 1434, r"if \(\(fIou < ([0-9.]+)\) && \(fIou2 < ([0-9.]+)\)\)", 2),
        ("MANY_FRAMES", "src/Object.cc", 1469, r"if \(mObjectFrame\.size\(\) > (\d+)\)", 1),
        ("TH_MANY_FRAMES", "src/Object.cc", 1470, r"th = ([0-9.]+);", 1),
        ("EDGE_PIXELS", "src/Object.cc", 1538, r"if \(\(ObjectFrame->mBox\.x > (\d+)\) && \(ObjectFrame->mBox\.y > (\d+)\) &&", 1),
        ("EDGE_PIXELS", "src/Object.cc", 1538, r"if \(\(ObjectFrame->mBox\.x > (\d+)\) && \(ObjectFrame->mBox\.y > (\d+)\) &&", 2),
        ("EDGE_PIXELS", "src/Object.cc", 1539, r"mBox\.width < image\.cols - (\d+)\) &&", 1),
        ("EDGE_PIXELS", "src/Object.cc", 1540, r"mBox\.height < image\.rows - (\d+)\)\)", 1),
        ("KEEP_COUNT", "src/Object.cc", 1555, r"if \(sit_sec > (\d+)\)", 1),
        ("CUBOID_SLACK", "src/Object.cc", 1772, r"abs\(scale\[0\]\) > ([0-9.]+) \* this->mCuboid3D\.lenth / 2\)", 1),
        ("CUBOID_SLACK", "src/Object.cc", 1773, r"abs\(scale\[1\]\) > ([0-9.]+) \* this->mCuboid3D\.width / 2\)", 1),
        ("CUBOID_SLACK", "src/Object.cc", 1774, r"abs\(scale\[2\]\) > ([0-9.]+) \* this->mCuboid3D\.height / 2\)\)", 1),
    ],
    # YOLOX::Detect around the network, and what Tracking::GrabImageRGBD keeps of its result
    "yolox": [
        ("NMS_THRESH", "include/YOLOX.h", 33, r"#define NMS_THRESH ([0-9.]+)", 1),
        ("BBOX_CONF_THRESH", "include/YOLOX.h", 34, r"#define BBOX_CONF_THRESH ([0-9.]+)", 1),
        ("INPUT_W", "include/YOLOX.h", 71, r"const int INPUT_W = (\d+);", 1),
        ("INPUT_H", "include/YOLOX.h", 72, r"const int INPUT_H = (\d+);", 1),
        ("PAD", "src/YOLOX.cc", 59, r"cv::Scalar\((\d+), \1, \1\)\);", 1),
        ("NUM_CLASS", "src/YOLOX.cc", 168, r"const int num_class = (\d+);", 1),
        ("MEAN_R", "src/YOLOX.cc", 219, _YOLOX_MEAN, 1), ("MEAN_G", "src/YOLOX.cc", 219, _YOLOX_MEAN, 2), ("MEAN_B", "src/YOLOX.cc", 219, _YOLOX_MEAN, 3),
        ("STD_R", "src/YOLOX.cc", 220, _YOLOX_STD, 1), ("STD_G", "src/YOLOX.cc", 220, _YOLOX_STD, 2), ("STD_B", "src/YOLOX.cc", 220, _YOLOX_STD, 3),
        ("STRIDE_0", "src/YOLOX.cc", 238, _YOLOX_STRIDES, 1), ("STRIDE_1", "src/YOLOX.cc", 238, _YOLOX_STRIDES, 2), ("STRIDE_2", "src/YOLOX.cc", 238, _YOLOX_STRIDES, 3),
        ("HALF", "src/YOLOX.cc", 185, r"float x0 = x_center - w \* ([0-9.]+f);", 1),
        ("TRACKING_MIN_PROB", "src/Tracking.cc", 434, r"if \(objInfo\.prob < ([0-9.]+)\)", 1),
    ] + [("TRACKING_CLASS_%d" % k, "src/Tracking.cc", 439, _YOLOX_CLASSES, k + 1) for k in range(14)],
}


def fixture_path(feature):
    return os.path.join(ROOT, "tests", "golden", feature + "_constants.json")


def two_spellings(rows):
    """the names that the rows give more than one literal"""
    by = {}
    return sorted({r["name"] for r in rows if by.setdefault(r["name"], r["literal"]) != r["literal"]})


def parse(reference_dir, feature):
    """[{name, literal, where}] in table order, as the reference tree's text reads on each row's line"""
    text, out = {}, []
    for name, rel, line, rx, group in TABLES[feature]:
        if rel not in text:
            text[rel] = open(os.path.join(reference_dir, rel), errors="replace").read().split("\n")
        m = re.search(rx, text[rel][line - 1])
        if not m:
            raise SystemExit("%s:%d does not read `%s`" % (rel, line, rx))
        out.append({"name": name, "literal": m.group(group), "where": "%s:%d" % (rel, line)})
    if two_spellings(out):
        raise SystemExit("%s spelled two ways in the reference text" % ", ".join(two_spellings(out)))
    return out


def load(feature):
    """the rows of the committed fixture"""
    return json.load(open(fixture_path(feature)))["constants"]


def literals(feature):
    """name -> literal of the committed fixture"""
    return {r["name"]: r["literal"] for r in load(feature)}


def main():
    args = [a for a in sys.argv[1:] if a != "--check"]
    if not args:
        raise SystemExit(__doc__)
    if set(args[1:]) - set(TABLES):
        raise SystemExit("no such feature: %s (the tables: %s)" % (", ".join(sorted(set(args[1:]) - set(TABLES))), ", ".join(TABLES)))
    for feature in args[1:] or list(TABLES):
        got = parse(args[0], feature)
        if "--check" in sys.argv:
            if [{k: r[k] for k in ("name", "literal", "where")} for r in load(feature)] != got:
                raise SystemExit("%s: fixture and reference text differ" % feature)
            print("ok", feature)
        elif feature == "ref":
            print("ref: written by tools/gen_ref_constants.py (typed rows and two headers)")
        else:
            with open(fixture_path(feature), "w") as f:
                json.dump({"constants": got}, f, indent=1)
                f.write("\n")
            print("wrote", fixture_path(feature))


if __name__ == "__main__":
    main()
