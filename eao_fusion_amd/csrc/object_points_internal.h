// object_points_internal.h -- the update of a map object's point list: steps 1, 3 and 4 of Object_Map::DataAssociateUpdate (reference src/Object.cc:1364-1436,
// :1460-1535, :1538-1589), step 1 of Object_Map::MergeTwoMapObjs (:1766-1821) and the erase loops of BigToSmall (:2070-2087) and DivideEquallyTwoObjs
// (:2096-2120).  HIP-free: csrc/object_points.hip includes it for the checks in front of its kernels and for the scalar rules its lanes run (the functions
// marked EAO_OP_HD compile for both sides, so the device and the host form share ONE transcription of them); tools/object_points_walk.cpp includes it alone,
// walks descs in upstream's literal form (a growing list, the `break`, the erase while iterating) and runs under the sanitizers.
//
// Nothing is transcribed twice: the pose arithmetic is object_cuboid_internal.h's, the projection and the rectangle are object_assoc_internal.h's, contains and
// the overlap ratios are frame_objects_internal.h's.  What is new here is float or double exactly as upstream's expressions read.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/eao_fusion.h"
#include "frame_objects_internal.h"
#include "object_assoc_internal.h"
#include "object_cuboid_internal.h"

#if defined(__HIPCC__)
#define EAO_OP_HD __host__ __device__ inline
#else
#define EAO_OP_HD inline
#endif

namespace eao {
namespace object_points {

using object_assoc::Extent;
using object_cuboid::Pose;

// ---- the literals (tests/golden/object_points_constants.json holds them to the reference text)
constexpr double kThManyFrames = 0.9;             // src/Object.cc:1470, narrowed by `float th`
constexpr int32_t kManyFrames = 5;                // :1469
constexpr int32_t kKeepCount = 8;                 // :1555
constexpr int32_t kEdgePixels = 25;               // :1538-1541 (the caller's box_off_edge; include/eaofusion/ObjectMap.h)
constexpr double kCuboidSlack = 1.1;              // :1772-1774
constexpr double kMinIou = 0.5;                   // :1434
constexpr double kMinIouFormer = 0.8;             // :1434

static_assert(kKeepCount == EAO_OBJECT_POINTS_KEEP_COUNT && kEdgePixels == EAO_OBJECT_POINTS_EDGE_PIXELS, "include/eao_fusion.h states the same literals");

constexpr int32_t kMaxDescs = EAO_OBJECT_POINTS_MAX_DESCS;
constexpr int64_t kMaxBatchPoints = (int64_t)1 << 27;      // list entries plus candidates of one call
constexpr int32_t kMaxRectField = 1 << 15;                  // rect fields and the image's sizes: x + width and the int areas stay in range

constexpr int32_t kDone = EAO_OBJECT_POINTS_DONE, kRejected = EAO_OBJECT_POINTS_REJECTED, kUndefined = EAO_OBJECT_POINTS_UNDEFINED;
constexpr int32_t kGateNone = EAO_OBJECT_POINTS_GATE_NONE, kGateRadius = EAO_OBJECT_POINTS_GATE_RADIUS, kGateCuboid = EAO_OBJECT_POINTS_GATE_CUBOID;
constexpr int32_t kEraseNone = EAO_OBJECT_POINTS_ERASE_NONE, kEraseProjection = EAO_OBJECT_POINTS_ERASE_PROJECTION, kEraseBox = EAO_OBJECT_POINTS_ERASE_BOX,
                  kEraseShrunk = EAO_OBJECT_POINTS_ERASE_SHRUNK;

// :1468-1470
EAO_OP_HD float radius_th(int32_t n_frames_after_push) {
    float th = (float)1.0;
    if (n_frames_after_push > kManyFrames) th = (float)kThManyFrames;
    return th;
}

// :1465-1473: whether the candidate stays (`>` is strict: a point exactly at th * rmax stays)
EAO_OP_HD bool radius_gate(const eao_object_points_desc& D, const float* p) {
    const float d0 = D.center[0] - p[0], d1 = D.center[1] - p[1], d2 = D.center[2] - p[2];
    const float fDis = object_cuboid::sqrt_f(d0 * d0 + d1 * d1 + d2 * d2);
    return !(fDis > radius_th(D.n_frames_after_push) * D.rmax);
}

EAO_OP_HD void pose_of(const eao_object_points_desc& D, Pose& P) {
    for (int k = 0; k < 4; k++) P.q[k] = D.pose_q[k];
    for (int k = 0; k < 3; k++) P.t[k] = D.pose_t[k];
}

// :1771-1777: inv = mCuboid3D.pose.inverse(); abs() of a double is std::abs(double), 1.1 * lenth / 2 is a double expression
EAO_OP_HD bool cuboid_gate(const eao_object_points_desc& D, const Pose& inv, const float* p) {
    const double w[3] = {(double)p[0], (double)p[1], (double)p[2]};
    double s[3];
    object_cuboid::pose_apply(inv, w, s);
    return !((::fabs(s[0]) > kCuboidSlack * (double)D.lenth / 2) || (::fabs(s[1]) > kCuboidSlack * (double)D.width / 2) ||
             (::fabs(s[2]) > kCuboidSlack * (double)D.height / 2));
}

EAO_OP_HD bool gate_of(const eao_object_points_desc& D, const Pose& inv, const float* p) {
    return D.gate == kGateRadius ? radius_gate(D, p) : cuboid_gate(D, inv, p);
}

// cv::countNonZero(a - b) == 0 over finite floats (:1515, :1803)
EAO_OP_HD bool same_point(const float* a, const float* b) { return a[0] == b[0] && a[1] == b[1] && a[2] == b[2]; }

EAO_OP_HD void project(const eao_object_points_desc& D, const float* X, float* u, float* v) { object_assoc::project_point(D.Tcw, D.fx, D.fy, D.cx, D.cy, X, u, v); }

EAO_OP_HD void extent_merge(Extent& e, const Extent& o) {
    e.anyNan |= o.anyNan;
    e.uMin = o.uMin < e.uMin ? o.uMin : e.uMin;
    e.uMax = o.uMax > e.uMax ? o.uMax : e.uMax;
    e.vMin = o.vMin < e.vMin ? o.vMin : e.vMin;
    e.vMax = o.vMax > e.vMax ? o.vMax : e.vMax;
}

// :1411-1435 behind the extrema of the n projections: the record's status, rect2, iou and iou2
EAO_OP_HD void change_verdict(const eao_object_points_desc& D, const Extent& e, int64_t n, eao_object_points_rec& r) {
    r.status = kUndefined;
    if (n == 0) return;      // x_pt[0] of an empty vector
    int32_t rect2[4];
    if (object_assoc::finish_rect(e, D.cols, D.rows, rect2) != object_assoc::kRectOk) return;
    for (int k = 0; k < 4; k++) r.rect2[k] = rect2[k];
    r.iou = frame_objects::overlap_ratio(D.project_rect1, rect2);
    r.iou2 = frame_objects::overlap_ratio_former(rect2, D.box_rect);
    r.status = (((double)r.iou < kMinIou) && ((double)r.iou2 < kMinIouFormer)) ? kRejected : kDone;
}

// whether the erase of stage 3 takes the entry at x whose object_id_vector holds `count`
EAO_OP_HD bool erase_entry(const eao_object_points_desc& D, const float* x, int32_t count) {
    if (D.erase == kEraseProjection) {      // :1543-1588
        if (!D.box_off_edge || count > kKeepCount) return false;
        float u, v;
        project(D, x, &u, &v);
        if ((u > 0 && u < D.cols) && (v > 0 && v < D.rows)) return !frame_objects::contains(D.box_rect, u, v);
        return false;
    }
    if (D.erase == kEraseBox)               // :2078-2080
        return (x[0] > D.bounds[0]) && (x[0] < D.bounds[1]) && (x[1] > D.bounds[2]) && (x[1] < D.bounds[3]) && (x[2] > D.bounds[4]) && (x[2] < D.bounds[5]);
    if (D.erase == kEraseShrunk) {          // :2105-2110: the half-extent is a float expression, the bound a double one
        const float half[3] = {D.lenth / 2 - D.overlap[0] / 2, D.width / 2 - D.overlap[1] / 2, D.height / 2 - D.overlap[2] / 2};
        for (int a = 0; a < 3; a++)
            if (!(((double)x[a] > D.cuboid_center[a] - (double)half[a]) && ((double)x[a] < D.cuboid_center[a] + (double)half[a]))) return false;
        return true;
    }
    return false;
}

// ---- what the entry points refuse (include/eao_fusion.h); nullptr = accepted
inline bool all_finite(const float* v, int64_t n) {
    for (int64_t i = 0; i < n; i++)
        if (!std::isfinite(v[i])) return false;
    return true;
}

inline bool rect_in_range(const int32_t* r) {
    return r[0] >= -kMaxRectField && r[0] <= kMaxRectField && r[1] >= -kMaxRectField && r[1] <= kMaxRectField && r[2] >= 0 && r[2] <= kMaxRectField && r[3] >= 0 &&
           r[3] <= kMaxRectField;
}

inline const char* desc_refusal(const eao_object_points_desc& D) {
    if (D.n_map < 0 || D.n_cand < 0) return "a negative count";
    if (D.gate != kGateNone && D.gate != kGateRadius && D.gate != kGateCuboid) return "an unknown gate";
    if (D.erase != kEraseNone && D.erase != kEraseProjection && D.erase != kEraseBox && D.erase != kEraseShrunk) return "an unknown erase";
    if (D.n_map > 0 && !D.map_points) return "map_points is NULL";
    if (D.n_map > 0 && D.erase == kEraseProjection && !D.map_count) return "map_count is NULL";
    if (D.n_cand > 0 && !D.cand_points) return "cand_points is NULL";
    if (D.n_cand > 0 && !D.cand_count) return "cand_count is NULL";
    if (!all_finite(D.Tcw, 16)) return "a non-finite Tcw";
    if (!(std::isfinite(D.fx) && std::isfinite(D.fy) && std::isfinite(D.cx) && std::isfinite(D.cy))) return "a non-finite intrinsic";
    if (D.cols < 0 || D.cols > kMaxRectField || D.rows < 0 || D.rows > kMaxRectField) return "cols or rows out of range";
    if (!rect_in_range(D.project_rect1) || !rect_in_range(D.box_rect)) return "a rect out of range";
    if (!all_finite(D.center, 3)) return "a non-finite center";
    if (!std::isfinite(D.rmax)) return "a non-finite rmax";
    if (!(std::isfinite(D.lenth) && std::isfinite(D.width) && std::isfinite(D.height))) return "a non-finite extent";
    for (int k = 0; k < 4; k++)
        if (!std::isfinite(D.pose_q[k])) return "a non-finite pose";
    for (int k = 0; k < 3; k++)
        if (!std::isfinite(D.pose_t[k])) return "a non-finite pose";
    for (int k = 0; k < 3; k++)
        if (!std::isfinite(D.cuboid_center[k])) return "a non-finite cuboid_center";
    if (!all_finite(D.bounds, 6)) return "a non-finite bound";
    if (!all_finite(D.overlap, 3)) return "a non-finite overlap";
    if (!all_finite(D.sum_pos, 3)) return "a non-finite sum_pos";
    if (!all_finite(D.map_points, 3 * (int64_t)D.n_map)) return "a non-finite point";
    if (!all_finite(D.cand_points, 3 * (int64_t)D.n_cand)) return "a non-finite candidate";
    return nullptr;
}

inline const char* out_refusal(const eao_object_points_desc& D, const eao_object_points_out& O) {
    if (!O.rec) return "rec is NULL";
    if (D.n_cand > 0 && !(O.gate && O.target && O.count)) return "gate, target or count is NULL";
    if ((int64_t)D.n_map + D.n_cand > 0 && !(O.list && O.erased && O.survivors)) return "list, erased or survivors is NULL";
    return nullptr;
}

// ---- what the kernels of csrc/object_points.hip read and write, for the callers that enqueue them (its own entry and csrc/object_chain.hip)
struct PtsDev {
    eao_object_points_desc d;                // the scalars; its pointers are the host's and are not read
    int64_t mapStart, candStart, listStart;  // in entries of the packed arrays
};

struct Bufs {
    const PtsDev* descs;
    const float* mapPts;
    const int32_t* mapCount;
    const float* candPts;
    const int32_t* candCount;
    int32_t *first, *rank, *app;             // per candidate (device only)
    uint8_t* gate;
    int32_t *target, *count;                 // per candidate
    int32_t* list;
    uint8_t* erased;
    int32_t* surv;
    float* survPts;                          // per list position
    eao_object_points_rec* recs;
};

#if defined(__HIPCC__)
// whether a desc of these sizes takes the call to the two-launch form
bool launch_is_split(int64_t n_map, int64_t n_cand);
// k_object_points_match over the descs of B (the two-launch form only), max_cand = the largest n_cand among them
hipError_t enqueue_match(hipStream_t stream, const Bufs& B, unsigned n_desc, int64_t max_cand);
// k_object_points (fused) or k_object_points_finish (behind enqueue_match)
hipError_t enqueue_finish(hipStream_t stream, const Bufs& B, unsigned n_desc, bool fused);
#endif

// ---- upstream's form, literally: the fallback no entry point takes, the sanitizer target and the -O3 baseline of tools/bench_object_points.py
struct Walk {
    eao_object_points_rec rec;
    std::vector<uint8_t> gate, erased;
    std::vector<int32_t> target, count, list, survivors;
    std::vector<float> points;      // the surviving positions
};

struct Entry {      // a MapPoint* of mvpMapObjectMappoints
    int32_t source, index, count;
    float pos[3];
};

inline void walk_update(const eao_object_points_desc& D, Walk& W) {
    W = Walk{};
    eao_object_points_rec& r = W.rec;
    const size_t M = (size_t)D.n_map, C = (size_t)D.n_cand;
    // step 1 (:1364-1436)
    if (D.change_gate) {
        std::vector<float> x_pt, y_pt;
        bool nan = false;
        for (size_t i = 0; i < C + M; i++) {
            float u, v;
            project(D, i < C ? D.cand_points + 3 * i : D.map_points + 3 * (i - C), &u, &v);
            nan = nan || std::isnan(u) || std::isnan(v);
            x_pt.push_back(u);
            y_pt.push_back(v);
        }
        Extent e;
        object_assoc::extent_init(e);
        e.anyNan = nan ? 1 : 0;
        if (!nan && !x_pt.empty()) {      // (std::sort over a NaN is undefined)
            std::sort(x_pt.begin(), x_pt.end());
            std::sort(y_pt.begin(), y_pt.end());
            e.uMin = x_pt[0]; e.uMax = x_pt[x_pt.size() - 1];
            e.vMin = y_pt[0]; e.vMax = y_pt[y_pt.size() - 1];
        }
        change_verdict(D, e, (int64_t)x_pt.size(), r);
        if (r.status == kUndefined) return;
        if (r.status == kRejected) {      // :1435
            for (int a = 0; a < 3; a++) r.sum_pos_appended[a] = r.sum_pos[a] = D.sum_pos[a];
            return;
        }
    }
    r.status = kDone;
    std::vector<Entry> list;
    for (size_t m = 0; m < M; m++) {
        Entry E{0, (int32_t)m, D.map_count ? D.map_count[m] : 0, {D.map_points[3 * m], D.map_points[3 * m + 1], D.map_points[3 * m + 2]}};
        list.push_back(E);
    }
    float sum[3] = {D.sum_pos[0], D.sum_pos[1], D.sum_pos[2]};
    // step 3 (:1460-1535, :1766-1821)
    W.gate.assign(C, 0);
    W.target.assign(C, -1);
    W.count.assign(C, 0);
    for (size_t j = 0; j < C && D.gate != kGateNone; j++) {
        const float* p = D.cand_points + 3 * j;
        W.count[j] = D.cand_count[j];
        Pose pose, inv;
        pose_of(D, pose);
        object_cuboid::pose_inverse(pose, inv);
        if (!gate_of(D, inv, p)) continue;
        W.gate[j] = 1;
        W.count[j] = D.cand_count[j] + 1;
        r.n_gated++;
        bool new_point = true;
        for (size_t m = 0; m < list.size(); ++m)
            if (same_point(p, list[m].pos)) {
                W.target[j] = (int32_t)m;
                new_point = false;
                break;
            }
        if (new_point) {
            Entry E{1, (int32_t)j, W.count[j], {p[0], p[1], p[2]}};
            list.push_back(E);
            r.n_appended++;
            for (int a = 0; a < 3; a++) sum[a] = sum[a] + p[a];
        }
    }
    if (D.gate == kGateNone)
        for (size_t j = 0; j < C; j++) W.count[j] = D.cand_count[j];
    for (int a = 0; a < 3; a++) r.sum_pos_appended[a] = sum[a];
    r.n_list = (int32_t)list.size();
    for (const Entry& E : list) {
        W.list.push_back(E.source);
        W.list.push_back(E.index);
    }
    // step 4 (:1543-1588, :2070-2087, :2096-2120): the erase while iterating
    W.erased.assign(list.size(), 0);
    size_t at = 0;
    for (std::vector<Entry>::iterator it = list.begin(); it != list.end(); at++) {
        if (erase_entry(D, it->pos, it->count)) {
            if (D.erase == kEraseProjection)
                for (int a = 0; a < 3; a++) sum[a] = sum[a] - it->pos[a];
            W.erased[at] = 1;
            r.n_erased++;
            it = list.erase(it);
        } else {
            ++it;
        }
    }
    for (int a = 0; a < 3; a++) r.sum_pos[a] = sum[a];
    r.n_survivors = (int32_t)list.size();
    for (const Entry& E : list) {
        W.survivors.push_back(E.source);
        W.survivors.push_back(E.index);
        for (int a = 0; a < 3; a++) W.points.push_back(E.pos[a]);
    }
}

}  // namespace object_points
}  // namespace eao
