// object_assoc_internal.h -- the host half of the object layer's per-frame data association: Object_2D::NoParaDataAssociation (reference src/Object.cc:728-962,
// the Wilcoxon rank-sum test of a detection's map points against a map object's) and Object_Map::ComputeProjectRectFrame (:1606-1651, the bounding box of an
// object's projected points).  HIP-free: csrc/object_assoc.hip includes it for the rules before and after its two kernels; tools/object_association_walk.cpp
// includes it alone, counts on the host in the kernel's form and runs under the sanitizers.
//
// Two facts the design rests on:
//   1. No sort is needed.  Upstream sorts each axis of the map object's good points separately and keeps elements 0, step, 2 step, ... (:798-807).  For a
//      detection value x let lb be the number of good map values < x and ub the number <= x, over ALL good points: the kept elements below x are ceil(lb / step),
//      those <= x are ceil(ub / step).  So w_12 += ceil(lb / step), w_00 += ceil(ub / step) - ceil(lb / step), w_21 += n - ceil(ub / step); ties and the order of
//      -0.0f / +0.0f inside std::sort cannot change a count.
//   2. The int product bounds everything.  m * n * (m + n + 1) is an int upstream (:942); above INT32_MAX it is signed overflow (undefined).  Below it, with
//      n < 6 m after the sampling, m * n < 2^24: upstream's float counters, incremented by one, never saturate and equal the integer counts kept here.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

// the projection and the rectangle compile for both sides: csrc/object_points.hip runs them inside its kernel
#if defined(__HIPCC__)
#define EAO_OA_HD __host__ __device__ inline
#else
#define EAO_OA_HD inline
#endif

namespace eao {
namespace object_assoc {

// ---- the literals of Object_2D::NoParaDataAssociation (tests/golden/object_association_constants.json holds them to the reference text)
constexpr int32_t kMinDetPoints = 20;       // src/Object.cc:760
constexpr int32_t kMinMapPoints = 20;       // :764
constexpr int32_t kSampleRatio = 3;         // :776 (and :778)
constexpr double kCritical = 1.282;         // :942
constexpr int32_t kVarianceDivisor = 12;    // :942
constexpr double kHalf = 0.5;               // :942

// the verdicts: upstream's return values, and 3 where its int product overflows
constexpr int32_t kSkip = 0, kAssociated = 1, kFailed = 2, kUndefined = 3, kPending = -1;

// What upstream knows before it compares a single coordinate (:732-828).  m: the detection's good points; nGood, S: the map object's good points and all of
// mvpMapObjectMappoints.  verdict: kSkip (:760), kFailed (:764), kUndefined, or kPending = the counts decide.  n and step are as far as upstream got:
//   kSkip, kFailed here     n = nGood, step = 0 (step is not declared yet)
//   kUndefined, kPending    n = the size of the sample (:808, :826), step = 1 without the sampling (:775)
struct Plan {
    int32_t m, n, step, verdict;
};
inline Plan plan_pair(int32_t m, int32_t nGood, int32_t S) {
    Plan p{m, nGood, 0, kPending};
    if (m < kMinDetPoints) { p.verdict = kSkip; return p; }
    if (nGood < kMinMapPoints) { p.verdict = kFailed; return p; }
    p.step = 1;
    const int64_t cap = (int64_t)kSampleRatio * m;
    if (cap > INT32_MAX) { p.verdict = kUndefined; return p; }      // `3 * m` itself overflows
    if ((int64_t)nGood > cap) {
        p.step = (int32_t)(S / (int32_t)cap);                       // S >= nGood > 3 m: step >= 1
        p.n = (int32_t)(((int64_t)nGood + p.step - 1) / p.step);    // elements 0, step, .. of nGood sorted values
    }
    if ((int64_t)p.m * p.n * ((int64_t)p.m + p.n + 1) > INT32_MAX) p.verdict = kUndefined;
    return p;
}

inline uint32_t ceil_div(uint32_t a, uint32_t step) { return (a + step - 1) / step; }

// :930-961 over the integer counts c = {x12 x21 x00 y12 y21 y00 z12 z21 z00}.  The expressions keep upstream's types: int terms, float sums, the critical values
// in double rounded to float once.  (csrc/ and the walk program are built with -ffp-contract=off: r1 and r2 are not fused.)
inline int32_t decide(int32_t m, int32_t n, const uint32_t* c, float* w, float* r) {
    for (int a = 0; a < 3; a++) {
        const float w12 = (float)c[3 * a], w21 = (float)c[3 * a + 1], w00 = (float)c[3 * a + 2];
        const float p = w12 + m * (m + 1) / 2, q = w21 + n * (n + 1) / 2;
        w[a] = (p < q ? p : q) + w00 / 2;      // std::min(p, q) returns q only when q < p; equal values are one value
    }
    const double root = std::sqrt((double)(m * n * (m + n + 1) / kVarianceDivisor));
    const double centre = kHalf * m * (m + n + 1), spread = kCritical * root;
    r[0] = (float)(centre - spread);
    r[1] = (float)(centre + spread);
    int add = 0;
    for (int a = 0; a < 3; a++)
        if (w[a] > r[0] && w[a] < r[1]) add++;
    return add == 3 ? kAssociated : kFailed;
}

// The counts of one pair on the host, in the kernel's form (the walk program; the timing tool's host baseline): per detection point lb and ub over all good map
// points, then the ceil rule.
inline void count_pair(const float* det, int32_t m, const float* map, int32_t nGood, int32_t step, int32_t n, uint32_t* c) {
    for (int k = 0; k < 9; k++) c[k] = 0;
    for (int32_t i = 0; i < m; i++)
        for (int a = 0; a < 3; a++) {
            const float x = det[3 * i + a];
            uint32_t lb = 0, ub = 0;
            for (int32_t j = 0; j < nGood; j++) {
                const float v = map[3 * j + a];
                lb += v < x ? 1u : 0u;
                ub += v <= x ? 1u : 0u;
            }
            const uint32_t kl = ceil_div(lb, (uint32_t)step), ku = ceil_div(ub, (uint32_t)step);
            c[3 * a] += kl;
            c[3 * a + 1] += (uint32_t)n - ku;
            c[3 * a + 2] += ku - kl;
        }
}

inline bool any_nan(const float* xyz, size_t nPoints) {
    for (size_t i = 0; i < 3 * nPoints; i++)
        if (std::isnan(xyz[i])) return true;
    return false;
}

// ---- Object_Map::ComputeProjectRectFrame
// :1617-1624 for one point.  Rcw * X + tcw is a cv::Mat product: accumulated in double, rounded to float once; 1.0 / z is a double
// division rounded to float; u and v are float expressions rounded operation by operation.  The kernel runs the same statements.
EAO_OA_HD void project_point(const float* Tcw, float fx, float fy, float cx, float cy, const float* X, float* u, float* v) {
    float Pc[3];
    for (int r = 0; r < 3; r++) {
        const double acc = (double)Tcw[4 * r] * (double)X[0] + (double)Tcw[4 * r + 1] * (double)X[1] + (double)Tcw[4 * r + 2] * (double)X[2];
        Pc[r] = (float)(acc + (double)Tcw[4 * r + 3]);
    }
    const float invzc = (float)(1.0 / (double)Pc[2]);
    *u = fx * Pc[0] * invzc + cx;
    *v = fy * Pc[1] * invzc + cy;
}

constexpr uint8_t kRectEmpty = 0, kRectOk = 1, kRectUndefined = 2;

// x_pt[0], x_pt[last], y_pt[0], y_pt[last] of the sorted lists (:1634-1639) as a min / max over the points, and whether any projection is a NaN
struct Extent {
    float uMin, uMax, vMin, vMax;
    uint32_t anyNan;
};
EAO_OA_HD void extent_init(Extent& e) { e.uMin = e.vMin = INFINITY; e.uMax = e.vMax = -INFINITY; e.anyNan = 0; }
EAO_OA_HD void extent_add(Extent& e, float u, float v) {
    if (std::isnan(u) || std::isnan(v)) e.anyNan = 1;
    e.uMin = u < e.uMin ? u : e.uMin;
    e.uMax = u > e.uMax ? u : e.uMax;
    e.vMin = v < e.vMin ? v : e.vMin;
    e.vMax = v > e.vMax ? v : e.vMax;
}

// float -> int as cv::Rect_<int>'s constructor converts: defined when the truncated value is an int
EAO_OA_HD bool fits_int(float v) { return v >= -2147483648.0f && v < 2147483648.0f; }

// :1641-1650.  rect = {x, y, width, height}; written only with kRectOk.
EAO_OA_HD uint8_t finish_rect(const Extent& e, int32_t cols, int32_t rows, int32_t* rect) {
    if (e.anyNan) return kRectUndefined;      // std::sort over a NaN (:1634)
    float x_min = e.uMin, x_max = e.uMax, y_min = e.vMin, y_max = e.vMax;
    if (x_min < 0) x_min = 0;
    if (y_min < 0) y_min = 0;
    if (x_max > cols) x_max = cols;
    if (y_max > rows) y_max = rows;
    const float width = x_max - x_min, height = y_max - y_min;
    if (!(fits_int(x_min) && fits_int(y_min) && fits_int(width) && fits_int(height))) return kRectUndefined;
    rect[0] = (int32_t)x_min;
    rect[1] = (int32_t)y_min;
    rect[2] = (int32_t)width;
    rect[3] = (int32_t)height;
    return kRectOk;
}

// ---- what the entry points check of the lists (include/eao_fusion.h); nullptr = accepted
inline const char* starts_refusal(int32_t n, const int32_t* start) {
    if (start[0] < 0) return "start[0] < 0";
    for (int32_t j = 0; j < n; j++)
        if (start[j] > start[j + 1]) return "starts do not ascend";
    return nullptr;
}

}  // namespace object_assoc
}  // namespace eao
