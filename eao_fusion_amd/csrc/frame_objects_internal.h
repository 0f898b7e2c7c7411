// frame_objects_internal.h -- a frame's 2D objects, steps 2, 4, 5 and 6 of Tracking::TrackWithMotionModel's object layer (reference src/Tracking.cc:1768-1973):
// Tracking::AssociateObjAndPoints (:3031-3065), Object_2D::ComputeMeanAndStandardFrame and RemoveOutliersByBoxPlot (src/Object.cc:61-157), the feature box
// (:1801-1854) and the removal of bad boxes (:1868-1973, Converter::bboxOverlapratio{,Former,Latter}, src/Converter.cc:194-212).  HIP-free:
// csrc/frame_objects.hip includes it for the checks in front of its kernels, the same-id links and the sequential second loop of step 6 behind the download;
// tools/frame_objects_walk.cpp includes it alone, walks whole frames in upstream's literal form (vectors, sorts, erases) and runs under the sanitizers.
//
// The arithmetic conventions (DESIGN.md sections 2 and 4p): a cv::Mat product accumulates in double and rounds once; `sum_pos_3d / n` is convertTo with
// alpha = 1.0 / n, i.e. src * (float)alpha + 0.0f in float; everything else is float, operation by operation (-ffp-contract=off).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <unordered_map>
#include <vector>

#include "../../include/eao_fusion.h"

// the scalar steps csrc/object_points.hip runs on the device too compile for both sides; csrc/frame_objects.hip calls them on the host only
#if defined(__HIPCC__)
#define EAO_FO_HD __host__ __device__ inline
#else
#define EAO_FO_HD inline
#endif

namespace eao {
namespace frame_objects {

// ---- the literals (tests/golden/frame_objects_constants.json holds them to the reference text)
constexpr int32_t kBoxplotMinPoints = 8;          // src/Tracking.cc:1782
constexpr int32_t kQuartileDivisor = 4;           // src/Object.cc:134
constexpr double kIqrFactor = 1.5;                // :139
constexpr int32_t kFeatureRectMinPoints = 4;      // src/Tracking.cc:1830
constexpr double kCrowdRatio = 0.05;              // :1876
constexpr int32_t kCrowdMax = 4;                  // :1880
constexpr double kLargeAreaRatio = 0.5;           // :1893
constexpr int32_t kFewPoints = 5;                 // :1897
constexpr int32_t kFewPointsOnEdge = 10;          // :1901
constexpr int32_t kFewPointsEdgePixels = 20;      // :1903
constexpr int32_t kOnEdgePixels = 5;              // :1912
constexpr double kSameObjectIou = 0.3;            // :1929
constexpr double kSurroundIou = 0.05;             // :1937
constexpr double kSurroundRatio = 0.85;           // :1939

constexpr int32_t kMaxKeypoints = EAO_FRAME_OBJECTS_MAX_KEYPOINTS, kMaxBoxes = EAO_FRAME_OBJECTS_MAX_BOXES;
constexpr int32_t kMaxBoxField = 1 << 15;         // box fields and the image's sizes: x + width and the int areas stay in range
constexpr float kMaxKeypoint = 1073741824.0f;     // 2^30: below it cvRound and the float -> int conversions of cv::Rect are defined

// cv::Rect_<int>::contains(Point2f) (:3046): the point converts through saturate_cast<int> = cvRound (nearest, ties to even), then x <= px < x + width.
EAO_FO_HD int32_t cv_round(float v) { return (int32_t)std::nearbyintf(v); }      // (the default rounding mode; |v| < 2^30)
EAO_FO_HD bool contains(const int32_t* box, float px, float py) {
    const int32_t x = cv_round(px), y = cv_round(py);
    return box[0] <= x && x < box[0] + box[2] && box[1] <= y && y < box[1] + box[3];
}

// the third row of Rcw * Pw + tcw (src/Object.cc:118, :146), and all three for the projection of _Pos (src/Tracking.cc:1809)
inline float camera_row(const float* Tcw, int r, const float* X) {
    const double acc = (double)Tcw[4 * r] * (double)X[0] + (double)Tcw[4 * r + 1] * (double)X[1] + (double)Tcw[4 * r + 2] * (double)X[2];
    return (float)(acc + (double)Tcw[4 * r + 3]);
}

// `sum_pos_3d / n` (src/Object.cc:80, src/Tracking.cc:1806).  n == 0: 0 * inf = NaN, as upstream.
inline float mat_div(float sum, int32_t n) {
    const float alpha = (float)(1.0 / (double)n);
    return sum * alpha + 0.0f;
}

// (rect1 & rect2).area() (src/Converter.cc:196)
EAO_FO_HD int32_t area(const int32_t* b) { return b[2] * b[3]; }
EAO_FO_HD int32_t overlap_area(const int32_t* a, const int32_t* b) {
    const int32_t x1 = std::max(a[0], b[0]), y1 = std::max(a[1], b[1]);
    const int32_t w = std::min(a[0] + a[2], b[0] + b[2]) - x1, h = std::min(a[1] + a[3], b[1] + b[3]) - y1;
    return (w <= 0 || h <= 0) ? 0 : w * h;
}
EAO_FO_HD float overlap_ratio(const int32_t* a, const int32_t* b) { const int32_t o = overlap_area(a, b); return (float)o / ((float)(area(a) + area(b) - o)); }
EAO_FO_HD float overlap_ratio_former(const int32_t* a, const int32_t* b) { return (float)overlap_area(a, b) / ((float)area(a)); }
EAO_FO_HD float overlap_ratio_latter(const int32_t* a, const int32_t* b) { return (float)overlap_area(a, b) / ((float)area(b)); }

// the first loop of step 6 for one box (:1870-1878): the other boxes it overlaps by more than 0.05 of THEIR area.  0 / 0 is NaN and compares false.
inline int32_t num_overlaps(int32_t n_box, const int32_t* boxes, int32_t f) {
    int32_t num = 0;
    for (int32_t l = 0; l < n_box; l++)
        if (l != f && overlap_ratio_latter(boxes + 4 * f, boxes + 4 * l) > kCrowdRatio) num++;
    return num;
}

// The rest of step 6 (:1879-1945), statement by statement: rec[k].n and rec[k].num_overlaps are read, rec[k].bad and rec[k].on_edge are written.  The second
// loop is sequential: an f that turns bad in mid-body finishes its body, and an l that an earlier f removed is skipped.
inline void remove_bad_boxes(int32_t n_box, const int32_t* boxes, const float* score, int32_t cols, int32_t rows, eao_frame_object_record* rec) {
    for (int32_t f = 0; f < n_box; f++) {
        rec[f].bad = rec[f].num_overlaps > kCrowdMax ? 1 : 0;
        rec[f].on_edge = 0;
    }
    for (int32_t f = 0; f < n_box; f++) {
        if (rec[f].bad) continue;
        const int32_t* b = boxes + 4 * f;
        if ((float)area(b) / (float)(cols * rows) > kLargeAreaRatio) rec[f].bad = 1;
        if (rec[f].n < kFewPoints)
            rec[f].bad = 1;
        else if (rec[f].n >= kFewPoints && rec[f].n < kFewPointsOnEdge) {
            if (b[0] < kFewPointsEdgePixels || b[1] < kFewPointsEdgePixels || b[0] + b[2] > cols - kFewPointsEdgePixels || b[1] + b[3] > rows - kFewPointsEdgePixels)
                rec[f].bad = 1;
        }
        if (b[0] < kOnEdgePixels || b[1] < kOnEdgePixels || b[0] + b[2] > cols - kOnEdgePixels || b[1] + b[3] > rows - kOnEdgePixels) rec[f].on_edge = 1;
        for (int32_t l = 0; l < n_box; l++) {
            if (rec[l].bad) continue;
            if (f == l) continue;
            const int32_t* c = boxes + 4 * l;
            if (overlap_ratio(b, c) > kSameObjectIou) {
                if (score[f] < score[l]) rec[f].bad = 1;
                else if (score[f] >= score[l]) rec[l].bad = 1;
            }
            if (overlap_ratio(b, c) > kSurroundIou) {
                if (overlap_ratio_former(b, c) > kSurroundRatio) rec[f].bad = 1;
                if (overlap_ratio_latter(b, c) > kSurroundRatio) rec[l].bad = 1;
            }
        }
    }
}

// next[i]: the next keypoint after i that holds the same map point, or -1.  k_frame_features follows these links to the LAST keypoint of a map point that lies
// in any box: that keypoint's coordinates are the map point's `feature` after step 2 (:3053).  Ids below kDirectIds (an adapter numbers a frame's map points
// from zero) index a table that is all -1 between calls; larger ones go through a hash map.
constexpr int32_t kDirectIds = 1 << 20;
inline void same_id_links(int32_t n_kp, const int32_t* mp_id, int32_t* next) {
    int32_t top = -1;
    for (int32_t i = 0; i < n_kp; i++) top = mp_id[i] > top ? mp_id[i] : top;
    if (top < kDirectIds) {
        static thread_local std::vector<int32_t> later;
        if ((int64_t)later.size() <= (int64_t)top) later.resize((size_t)top + 1, -1);
        for (int32_t i = n_kp - 1; i >= 0; i--) {
            next[i] = -1;
            if (mp_id[i] < 0) continue;
            next[i] = later[(size_t)mp_id[i]];
            later[(size_t)mp_id[i]] = i;
        }
        for (int32_t i = 0; i < n_kp; i++)
            if (mp_id[i] >= 0) later[(size_t)mp_id[i]] = -1;
        return;
    }
    std::unordered_map<int32_t, int32_t> later;
    for (int32_t i = n_kp - 1; i >= 0; i--) {
        next[i] = -1;
        if (mp_id[i] < 0) continue;
        auto it = later.find(mp_id[i]);
        if (it != later.end()) { next[i] = it->second; it->second = i; }
        else later.emplace(mp_id[i], i);
    }
}

// ---- what the entry points refuse (include/eao_fusion.h); nullptr = accepted
inline const char* frame_refusal(const eao_frame_objects_desc& F) {
    if (F.n_kp < 0 || F.n_kp > kMaxKeypoints) return "n_kp outside 0 .. 4096";
    if (F.n_box < 0 || F.n_box > kMaxBoxes) return "n_box outside 0 .. 256";
    if (F.cols < 0 || F.rows < 0 || F.cols > kMaxBoxField || F.rows > kMaxBoxField) return "cols or rows outside 0 .. 2^15";
    if (F.n_kp > 0 && !(F.kp_x && F.kp_y && F.mp_id && F.mp_xyz)) return "a keypoint array is NULL";
    if (F.n_box > 0 && !(F.boxes && F.score)) return "boxes or score is NULL";
    for (int k = 0; k < 16; k++)
        if (!std::isfinite(F.Tcw[k])) return "a non-finite pose";
    if (!(std::isfinite(F.fx) && std::isfinite(F.fy) && std::isfinite(F.cx) && std::isfinite(F.cy))) return "a non-finite intrinsic";
    for (int32_t i = 0; i < F.n_kp; i++) {
        if (!(std::isfinite(F.kp_x[i]) && std::isfinite(F.kp_y[i]))) return "a non-finite keypoint";
        if (!(std::fabs(F.kp_x[i]) < kMaxKeypoint && std::fabs(F.kp_y[i]) < kMaxKeypoint)) return "a keypoint at or beyond 2^30";
        if (F.mp_id[i] < -1) return "mp_id below -1";
        if (F.mp_id[i] >= 0 && !(std::isfinite(F.mp_xyz[3 * i]) && std::isfinite(F.mp_xyz[3 * i + 1]) && std::isfinite(F.mp_xyz[3 * i + 2]))) return "a non-finite position";
    }
    for (int32_t k = 0; k < 4 * F.n_box; k++) {
        const int32_t v = F.boxes[k];
        if ((k & 3) >= 2 && v < 0) return "a negative box width or height";
        if (v > kMaxBoxField || v < -kMaxBoxField) return "a box field beyond 2^15";
    }
    return nullptr;
}

// ---- upstream's form, literally: the fallback no entry point takes, the sanitizer target and the -O3 baseline of tools/bench_frame_objects.py
struct Walk {
    std::vector<eao_frame_object_record> rec;
    std::vector<std::vector<int32_t>> assigned, kept;      // keypoint indices per box: Obj_c_MapPonits after step 2 and after the boxplot
};

// Object_2D::ComputeMeanAndStandardFrame (src/Object.cc:61-100) without the isBad() re-reads (one snapshot, include/eaofusion/FrameObjects.h)
inline void mean_and_standard(const eao_frame_objects_desc& F, const std::vector<int32_t>& list, const float* sum, float* pos, float* sd) {
    const int32_t n = (int32_t)list.size();
    for (int a = 0; a < 3; a++) pos[a] = mat_div(sum[a], n);
    float sum2[3] = {0, 0, 0};
    for (int32_t i : list)
        for (int a = 0; a < 3; a++) sum2[a] += (F.mp_xyz[3 * i + a] - pos[a]) * (F.mp_xyz[3 * i + a] - pos[a]);
    for (int a = 0; a < 3; a++) sd[a] = std::sqrt(sum2[a] / (float)n);
}

// the inner gate of RemoveOutliersByBoxPlot (:131): it cannot fire behind the `>= 8` gate of src/Tracking.cc:1782
inline bool boxplot_gate(size_t n) { return (n / 4 <= 0) || (n * 3 / 4 >= n - 1); }

// Object_2D::RemoveOutliersByBoxPlot (:104-157) up to its erase; false = the inner gate returned
inline bool boxplot(const eao_frame_objects_desc& F, std::vector<int32_t>& list, float* q1, float* q3, float* max_th) {
    std::vector<float> z_c;
    for (int32_t i : list) z_c.push_back(camera_row(F.Tcw, 2, F.mp_xyz + 3 * i));
    std::sort(z_c.begin(), z_c.end());
    if (boxplot_gate(z_c.size())) return false;
    const float Q1 = z_c[(int)(z_c.size() / kQuartileDivisor)], Q3 = z_c[(int)(z_c.size() * 3 / kQuartileDivisor)];
    const float IQR = Q3 - Q1;
    const float th = (float)((double)Q3 + kIqrFactor * (double)IQR);
    for (auto it = list.begin(); it != list.end();) {
        if (camera_row(F.Tcw, 2, F.mp_xyz + 3 * *it) > th) it = list.erase(it);
        else ++it;
    }
    *q1 = Q1; *q3 = Q3; *max_th = th;
    return true;
}

inline void walk_frame(const eao_frame_objects_desc& F, Walk& W) {
    const int32_t M = F.n_box;
    W.rec.assign((size_t)M, eao_frame_object_record{});
    W.assigned.assign((size_t)M, {});
    W.kept.assign((size_t)M, {});
    std::unordered_map<int32_t, int32_t> feature;      // map point -> the keypoint whose coordinates pMP->feature holds
    // step 2 (:3036-3064)
    for (int32_t i = 0; i < F.n_kp; i++) {
        if (F.mp_id[i] < 0) continue;
        for (int32_t k = 0; k < M; k++)
            if (contains(F.boxes + 4 * k, F.kp_x[i], F.kp_y[i])) {
                feature[F.mp_id[i]] = i;
                W.assigned[k].push_back(i);
                for (int a = 0; a < 3; a++) W.rec[k].sum_pos[a] = W.rec[k].sum_pos[a] + F.mp_xyz[3 * i + a];
            }
    }
    for (int32_t k = 0; k < M; k++) {
        eao_frame_object_record& r = W.rec[k];
        std::vector<int32_t>& list = W.kept[k] = W.assigned[k];
        r.n_assigned = (int32_t)list.size();
        // step 4 (:1776-1787)
        mean_and_standard(F, list, r.sum_pos, r.pos, r.std);
        if ((int32_t)list.size() >= kBoxplotMinPoints && boxplot(F, list, &r.q1, &r.q3, &r.max_th)) {
            r.boxplot_ran = 1;
            mean_and_standard(F, list, r.sum_pos, r.pos, r.std);      // about the OLD sum over the NEW count: the erase leaves sum_pos_3d alone
        }
        r.n = (int32_t)list.size();
        // step 5 (:1803-1854)
        for (int a = 0; a < 3; a++) r.pos[a] = mat_div(r.sum_pos[a], r.n);
        const float xc = camera_row(F.Tcw, 0, r.pos), yc = camera_row(F.Tcw, 1, r.pos), zc = camera_row(F.Tcw, 2, r.pos);
        const float invzc = (float)(1.0 / (double)zc);
        r.center_2d[0] = F.fx * xc * invzc + F.cx;
        r.center_2d[1] = F.fy * yc * invzc + F.cy;
        std::vector<float> x_pt, y_pt;
        for (int32_t i : list) {
            const int32_t j = feature[F.mp_id[i]];
            x_pt.push_back(F.kp_x[j]);
            y_pt.push_back(F.kp_y[j]);
        }
        if ((int32_t)x_pt.size() >= kFeatureRectMinPoints) {
            std::sort(x_pt.begin(), x_pt.end());
            std::sort(y_pt.begin(), y_pt.end());
            float x_min = x_pt[0], x_max = x_pt[x_pt.size() - 1], y_min = y_pt[0], y_max = y_pt[y_pt.size() - 1];
            if (x_min < 0) x_min = 0;
            if (y_min < 0) y_min = 0;
            if (x_max > F.cols) x_max = F.cols;
            if (y_max > F.rows) y_max = F.rows;
            r.has_feature_rect = 1;
            r.feature_rect[0] = (int32_t)x_min;
            r.feature_rect[1] = (int32_t)y_min;
            r.feature_rect[2] = (int32_t)(x_max - x_min);
            r.feature_rect[3] = (int32_t)(y_max - y_min);
        }
        r.num_overlaps = num_overlaps(M, F.boxes, k);
    }
    // step 6 (:1868-1945)
    remove_bad_boxes(M, F.boxes, F.score, F.cols, F.rows, W.rec.data());
}

}  // namespace frame_objects
}  // namespace eao
