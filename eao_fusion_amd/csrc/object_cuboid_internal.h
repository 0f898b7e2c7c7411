// object_cuboid_internal.h -- a map object's cuboid: Object_Map::ComputeMeanAndStandard (reference src/Object.cc:999-1235) with Object_Map::UpdateObjPose
// (:2243-2303), and the pairwise overlap test that reads its result (Object_Map::WhetherOverlap, :1954-1970; LocalMapping::WhetherOverlapObject,
// src/LocalMapping.cc:858-877).  HIP-free: csrc/object_cuboid.hip includes it for the checks in front of its kernels and for the scalar steps one lane runs
// between the passes (the functions marked EAO_OC_HD compile for both sides, so the device and the host form share ONE transcription of them);
// tools/object_cuboid_walk.cpp includes it alone, walks objects in upstream's literal form (push_back, std::sort, the early returns) and runs under the sanitizers.
//
// The arithmetic conventions (DESIGN.md sections 2 and 4q): `mSumPointsPos / n` is convertTo with alpha = 1.0 / n, i.e. src * (float)alpha + 0.0f in float;
// `Rcw * Ryaw` accumulates in double from +0.0 and rounds once; Eigen's and g2o's double code is transcribed operation by operation; everything else is float,
// operation by operation (-ffp-contract=off).  Divisions and square roots are IEEE's (no reciprocal shortcuts, csrc/sim3_internal.h:19).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/eao_fusion.h"

#if defined(__HIPCC__)
#define EAO_OC_HD __host__ __device__ inline
#else
#define EAO_OC_HD inline
#endif

namespace eao {
namespace object_cuboid {

// ---- the literals (tests/golden/object_cuboid_constants.json holds them to the reference text)
constexpr int32_t kFewFrames = 5;                 // src/Object.cc:1071: below it the bounds come from the world-frame points
constexpr int32_t kCornerFarA = 2, kCornerFarB = 8; // :1185: cuboidCenter = (corner_2 + corner_8) / 2
// the corner numbering of :1106-1113 and :1160-1167: corner k + 1 takes x / y / z from the maximum where the bit is set
constexpr uint8_t kCornerMaxX = 0x66, kCornerMaxY = 0xCC, kCornerMaxZ = 0xF0;

constexpr int32_t kMaxObjects = EAO_OBJECT_CUBOID_MAX_OBJECTS, kMaxOverlapRows = EAO_OBJECT_OVERLAP_MAX_ROWS;
constexpr int64_t kMaxBatchEntries = (int64_t)1 << 27;      // points plus centroids of one call: the staging block stays below 2 GB

struct Pose {
    double q[4];      // x y z w
    double t[3];
};

EAO_OC_HD float sqrt_f(float v) { return (float)::sqrt((double)v); }      // (sqrt through double is the same float)

// `mSumPointsPos / size()` (:1027).  n == 0: 0 * inf = NaN, as upstream.
EAO_OC_HD float mat_div(float sum, int32_t n) {
    const float alpha = (float)(1.0 / (double)n);
    return sum * alpha + 0.0f;
}

// Eigen::Quaterniond(const Matrix3d&), m row-major: the reading of csrc/sim3_internal.h::quat_from_R_eigen (0.5 / t is a division, a strict > moves to the later
// diagonal entry)
EAO_OC_HD void quat_from_R(const double* m, double* q) {
    double t = m[0] + m[4] + m[8];
    if (t > 0) {
        t = ::sqrt(t + 1.0);
        q[3] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (m[7] - m[5]) * t; q[1] = (m[2] - m[6]) * t; q[2] = (m[3] - m[1]) * t;
        return;
    }
    int i = 0;
    if (m[4] > m[0]) i = 1;
    if (m[8] > (i == 1 ? m[4] : m[0])) i = 2;
    if (i == 0) {
        t = ::sqrt(m[0] - m[4] - m[8] + 1.0);
        q[0] = 0.5 * t; t = 0.5 / t;
        q[3] = (m[7] - m[5]) * t; q[1] = (m[3] + m[1]) * t; q[2] = (m[6] + m[2]) * t;
    } else if (i == 1) {
        t = ::sqrt(m[4] - m[8] - m[0] + 1.0);
        q[1] = 0.5 * t; t = 0.5 / t;
        q[3] = (m[2] - m[6]) * t; q[2] = (m[7] + m[5]) * t; q[0] = (m[1] + m[3]) * t;
    } else {
        t = ::sqrt(m[8] - m[0] - m[4] + 1.0);
        q[2] = 0.5 * t; t = 0.5 / t;
        q[3] = (m[3] - m[1]) * t; q[0] = (m[2] + m[6]) * t; q[1] = (m[5] + m[7]) * t;
    }
}

// Converter::toSE3Quat (src/Converter.cc:28-38) -> g2o::SE3Quat(R, t) (Thirdparty/g2o/g2o/types/se3quat.h:58-60): Quaterniond(R), then normalizeRotation
// (:280-285): coeffs *= -1 where w < 0, then coeffs /= sqrt(x x + y y + z z + w w)
EAO_OC_HD void se3_from_T(const float* T, Pose& P) {
    double R[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) R[3 * i + j] = (double)T[4 * i + j];
    for (int i = 0; i < 3; i++) P.t[i] = (double)T[4 * i + 3];
    quat_from_R(R, P.q);
    if (P.q[3] < 0)
        for (int k = 0; k < 4; k++) P.q[k] = P.q[k] * -1.0;
    const double n2 = ((P.q[0] * P.q[0] + P.q[1] * P.q[1]) + P.q[2] * P.q[2]) + P.q[3] * P.q[3];
    const double n = ::sqrt(n2);
    for (int k = 0; k < 4; k++) P.q[k] = P.q[k] / n;
}

// Eigen's Quaterniond * Vector3d: uv = vec x v; uv += uv; v + w * uv + vec x uv
EAO_OC_HD void quat_rotate(const double* q, const double* v, double* out) {
    double uv[3] = {q[1] * v[2] - q[2] * v[1], q[2] * v[0] - q[0] * v[2], q[0] * v[1] - q[1] * v[0]};
    for (int k = 0; k < 3; k++) uv[k] = uv[k] + uv[k];
    const double c[3] = {q[1] * uv[2] - q[2] * uv[1], q[2] * uv[0] - q[0] * uv[2], q[0] * uv[1] - q[1] * uv[0]};
    for (int k = 0; k < 3; k++) out[k] = (v[k] + q[3] * uv[k]) + c[k];
}

// SE3Quat::inverse (se3quat.h:123-128): r = conjugate, t = r * (t * -1.)
EAO_OC_HD void pose_inverse(const Pose& P, Pose& I) {
    I.q[0] = -P.q[0]; I.q[1] = -P.q[1]; I.q[2] = -P.q[2]; I.q[3] = P.q[3];
    const double m[3] = {P.t[0] * -1.0, P.t[1] * -1.0, P.t[2] * -1.0};
    quat_rotate(I.q, m, I.t);
}

// SE3Quat::operator*(Vector3d) (:119-121): _t + _r * v
EAO_OC_HD void pose_apply(const Pose& P, const double* v, double* out) {
    double r[3];
    quat_rotate(P.q, v, r);
    for (int k = 0; k < 3; k++) out[k] = P.t[k] + r[k];
}

// :1137-1140: pose.inverse() * p in double, narrowed by the push_back
EAO_OC_HD void to_object_frame(const Pose& inv, const float* p, float* out) {
    const double w[3] = {(double)p[0], (double)p[1], (double)p[2]};
    double o[3];
    pose_apply(inv, w, o);
    for (int k = 0; k < 3; k++) out[k] = (float)o[k];
}

// Object_Map::UpdateObjPose (:2243-2303) behind the nine floats of Ryaw: both float matrices into the record, both poses out
EAO_OC_HD void update_obj_pose(const float* Ryaw, eao_object_cuboid_rec& r, Pose& pose, Pose& pose_wy) {
    float* T = r.Twobj;
    float* W = r.Twobj_without_yaw;
    for (int k = 0; k < 16; k++) T[k] = W[k] = (k % 5 == 0) ? 1.0f : 0.0f;      // cv::Mat::eye(4, 4, CV_32F)
    float res[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {      // Rcw * Ryaw, Rcw = the identity block of Twobj (:2264-2266)
            double acc = 0.0;
            for (int k = 0; k < 3; k++) acc = acc + (double)T[4 * i + k] * (double)Ryaw[3 * k + j];
            res[3 * i + j] = (float)acc;
        }
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) T[4 * i + j] = res[3 * i + j];
        T[4 * i + 3] = (float)r.cuboid_center[i];      // :2273: the narrowing is part of the arithmetic
    }
    W[3] = r.center[0];                                // :2293-2295: mCenter3D, cuboidCenter[1], mCenter3D
    W[7] = (float)r.cuboid_center[1];
    W[11] = r.center[2];
    se3_from_T(T, pose);
    se3_from_T(W, pose_wy);
    for (int k = 0; k < 4; k++) { r.pose_q[k] = pose.q[k]; r.pose_without_yaw_q[k] = pose_wy.q[k]; }
    for (int k = 0; k < 3; k++) { r.pose_t[k] = pose.t[k]; r.pose_without_yaw_t[k] = pose_wy.t[k]; }
}

// :1083-1122: ext = x_min x_max y_min y_max z_min z_max of the world-frame points
EAO_OC_HD void world_box(const float* ext, eao_object_cuboid_rec& r) {
    for (int a = 0; a < 3; a++) r.cuboid_center[a] = (double)((ext[2 * a + 1] + ext[2 * a]) / 2);
    for (int k = 0; k < 6; k++) r.bounds[k] = ext[k];
    r.lenth = ext[1] - ext[0];
    r.width = ext[3] - ext[2];
    r.height = ext[5] - ext[4];
    for (int c = 0; c < 8; c++) {
        const double x = (double)ext[(kCornerMaxX >> c) & 1], y = (double)ext[2 + ((kCornerMaxY >> c) & 1)], z = (double)ext[4 + ((kCornerMaxZ >> c) & 1)];
        r.corners[c][0] = r.corners_w[c][0] = x;
        r.corners[c][1] = r.corners_w[c][1] = y;
        r.corners[c][2] = r.corners_w[c][2] = z;
    }
    r.bounds_written = 1;
}

// :1160-1217: ext = the six extrema in the object frame; pose and pose_wy are those of the first UpdateObjPose and leave as those of the second
EAO_OC_HD void object_box(const float* Ryaw, const float* ext, Pose& pose, Pose& pose_wy, eao_object_cuboid_rec& r) {
    for (int c = 0; c < 8; c++) {
        const double v[3] = {(double)ext[(kCornerMaxX >> c) & 1], (double)ext[2 + ((kCornerMaxY >> c) & 1)], (double)ext[4 + ((kCornerMaxZ >> c) & 1)]};
        pose_apply(pose, v, r.corners[c]);
        pose_apply(pose_wy, v, r.corners_w[c]);
    }
    r.lenth = ext[1] - ext[0];
    r.width = ext[3] - ext[2];
    r.height = ext[5] - ext[4];
    for (int a = 0; a < 3; a++) r.cuboid_center[a] = (r.corners[kCornerFarA - 1][a] + r.corners[kCornerFarB - 1][a]) / 2.0;
    update_obj_pose(Ryaw, r, pose, pose_wy);
    float fRMax = 0.0f;
    for (int c = 0; c < 8; c++) {
        const float d0 = r.center[0] - (float)r.corners[c][0], d1 = r.center[1] - (float)r.corners[c][1], d2 = r.center[2] - (float)r.corners[c][2];
        const float fTmp = sqrt_f(d0 * d0 + d1 * d1 + d2 * d2);
        fRMax = (fRMax < fTmp) ? fTmp : fRMax;      // std::max
    }
    r.rmax = fRMax;
}

// one centroid's terms (:1062-1064, :1228-1232): the three squares and the distance
EAO_OC_HD void centroid_terms(const float* c, const float* center, float* sq, float* dis) {
    for (int a = 0; a < 3; a++) sq[a] = (c[a] - center[a]) * (c[a] - center[a]);
    *dis = sqrt_f(sq[0] + sq[1] + sq[2]);
}

// Object_Map::WhetherOverlap (:1957-1966) with the extents of src/LocalMapping.cc:873-875; abs() of a double is std::abs(double), narrowed by the assignment
EAO_OC_HD bool overlap(const eao_object_overlap_row& a, const eao_object_overlap_row& b, float* extents) {
    const float dis_x = (float)::fabs(a.cuboid_center[0] - b.cuboid_center[0]);
    const float dis_y = (float)::fabs(a.cuboid_center[1] - b.cuboid_center[1]);
    const float dis_z = (float)::fabs(a.cuboid_center[2] - b.cuboid_center[2]);
    const float sum_lenth_half = a.lenth / 2 + b.lenth / 2;
    const float sum_width_half = a.width / 2 + b.width / 2;
    const float sum_height_half = a.height / 2 + b.height / 2;
    extents[0] = sum_lenth_half - dis_x;
    extents[1] = sum_width_half - dis_y;
    extents[2] = sum_height_half - dis_z;
    return (dis_x < sum_lenth_half) && (dis_y < sum_width_half) && (dis_z < sum_height_half);
}

// ---- what k_object_cuboids reads per object from device memory, for the callers that enqueue it: the file's own entry writes it on the host, the plan kernel
// of csrc/object_chain.hip on the device.  An object with skip != 0 costs nothing: its workgroup leaves at once and stores no record.
struct ObjDev {
    int64_t pointStart, centroidStart;       // in entries of the packed lists
    int32_t n, m;
    float Ryaw[9];
    int32_t skip;
    double prev[3];
};
static_assert(sizeof(ObjDev) == 88, "ObjDev layout");

#if defined(__HIPCC__)
hipError_t enqueue_cuboids(hipStream_t stream, const ObjDev* objs, const float* points, const float* centroids, eao_object_cuboid_rec* records, unsigned n_obj);
#endif

// ---- what the entry points refuse (include/eao_fusion.h); nullptr = accepted
inline const char* object_refusal(const eao_object_cuboid_desc& D) {
    if (D.n_points < 0 || D.n_centroids < 0) return "a negative count";
    if (D.n_points > 0 && !D.points) return "points is NULL";
    if (D.n_centroids > 0 && !D.centroids) return "centroids is NULL";
    for (int k = 0; k < 9; k++)
        if (!std::isfinite(D.Ryaw[k])) return "a non-finite Ryaw";
    for (int k = 0; k < 3; k++)
        if (!std::isfinite(D.prev_cuboid_center[k])) return "a non-finite prev_cuboid_center";
    for (int64_t i = 0; i < 3 * (int64_t)D.n_points; i++)
        if (!std::isfinite(D.points[i])) return "a non-finite point";
    for (int64_t i = 0; i < 3 * (int64_t)D.n_centroids; i++)
        if (!std::isfinite(D.centroids[i])) return "a non-finite centroid";
    return nullptr;
}

inline const char* overlap_refusal(int32_t m, const eao_object_overlap_row* rows, const uint8_t* eligible, const uint8_t* verdict) {
    if (m < 0) return "a negative count";
    if (m > kMaxOverlapRows) return "more rows than EAO_OBJECT_OVERLAP_MAX_ROWS";
    if (m > 0 && !(rows && eligible && verdict)) return "a null pointer";
    for (int32_t i = 0; i < m; i++) {
        for (int k = 0; k < 3; k++)
            if (!std::isfinite(rows[i].cuboid_center[k])) return "a non-finite cuboid_center";
        if (!(std::isfinite(rows[i].lenth) && std::isfinite(rows[i].width) && std::isfinite(rows[i].height))) return "a non-finite scale";
    }
    return nullptr;
}

// ---- upstream's form, literally: the fallback no entry point takes, the sanitizer target and the -O3 baseline of tools/bench_object_cuboid.py
inline void walk_object(const eao_object_cuboid_desc& D, eao_object_cuboid_rec& r) {
    r = eao_object_cuboid_rec{};
    const size_t n = (size_t)D.n_points, m = (size_t)D.n_centroids;
    // :1001-1024 (the adapter has erased the bad points)
    for (size_t i = 0; i < n; i++)
        for (int a = 0; a < 3; a++) r.sum_pos[a] = r.sum_pos[a] + D.points[3 * i + a];
    for (int a = 0; a < 3; a++) r.center[a] = mat_div(r.sum_pos[a], (int32_t)n);
    // step 1 (:1030-1048)
    float sum2[3] = {0, 0, 0};
    std::vector<float> pt[3];
    for (size_t i = 0; i < n; i++)
        for (int a = 0; a < 3; a++) {
            sum2[a] += (D.points[3 * i + a] - r.center[a]) * (D.points[3 * i + a] - r.center[a]);
            pt[a].push_back(D.points[3 * i + a]);
        }
    for (int a = 0; a < 3; a++) r.standar[a] = sqrt_f(sum2[a] / (float)n);
    r.status = EAO_OBJECT_CUBOID_EMPTY;
    if (pt[0].size() == 0) return;      // :1050
    r.status = EAO_OBJECT_CUBOID_DONE;
    // step 2 (:1054-1068)
    float sum2c[3] = {0, 0, 0};
    for (size_t i = 0; i < m; i++)
        for (int a = 0; a < 3; a++) sum2c[a] += (D.centroids[3 * i + a] - r.center[a]) * (D.centroids[3 * i + a] - r.center[a]);
    for (int a = 0; a < 3; a++) r.center_standar[a] = sqrt_f(sum2c[a] / (float)m);
    // step 3 (:1071-1123)
    for (int a = 0; a < 3; a++) r.cuboid_center[a] = D.prev_cuboid_center[a];
    if (m < (size_t)kFewFrames) {
        float ext[6];
        for (int a = 0; a < 3; a++) {
            std::sort(pt[a].begin(), pt[a].end());
            ext[2 * a] = pt[a][0];
            ext[2 * a + 1] = pt[a][pt[a].size() - 1];
        }
        world_box(ext, r);
    }
    // step 4 (:1128-1217)
    Pose pose, pose_wy;
    update_obj_pose(D.Ryaw, r, pose, pose_wy);
    std::vector<float> obj[3];
    for (size_t i = 0; i < n; i++) {
        Pose inv;
        pose_inverse(pose, inv);
        float o[3];
        to_object_frame(inv, D.points + 3 * i, o);
        for (int a = 0; a < 3; a++) obj[a].push_back(o[a]);
    }
    float ext[6];
    const size_t s = obj[0].size();
    for (int a = 0; a < 3; a++) {
        std::sort(obj[a].begin(), obj[a].end());
        ext[2 * a] = obj[a][0];
        ext[2 * a + 1] = obj[a][s - 1];
    }
    object_box(D.Ryaw, ext, pose, pose_wy, r);
    // :1220-1234
    float dis = 0;
    for (size_t i = 0; i < m; i++) {
        float sq[3], d;
        centroid_terms(D.centroids + 3 * i, r.center, sq, &d);
        dis += d;
    }
    r.center_standar_dis = sqrt_f(dis / (float)m);
}

inline void walk_overlaps(int32_t m, const eao_object_overlap_row* rows, const uint8_t* eligible, uint8_t* verdict, float* extents) {
    for (int32_t i = 0; i < m; i++)
        for (int32_t j = 0; j < m; j++) {
            float e[3];
            const bool v = i != j && eligible[i] && eligible[j] && overlap(rows[i], rows[j], e);
            verdict[(size_t)i * m + j] = v ? 1 : 0;
            if (v && extents)
                for (int k = 0; k < 3; k++) extents[3 * ((size_t)i * m + j) + k] = e[k];
        }
}

}  // namespace object_cuboid
}  // namespace eao
