// yolox_internal.h -- what YOLOX::Detect does around the network (reference src/YOLOX.cc:51-62, :85-274, :369-410; the grey image of src/Tracking.cc:324-330),
// stated once for the host and, where marked, for the kernels of yolox.hip.  Plain C++17, no HIP: tools/yolox_walk.cpp runs it under AddressSanitizer on a
// machine without a GPU, and include/eaofusion/YOLOX.h takes its literal decode when the library reports a tie or an overflow.
//
//   geometry        r = min(S / (cols * 1.0), S / (rows * 1.0)) evaluated in double and stored as float; unpad = (int)(r * cols): a FLOAT product truncated, so a
//                   1064-wide frame gives 639 columns and one column of padding (:53-56).  `scale` of the decode is the same float (:390).
//   letterbox       cv::resize's 11-bit fixed-point bilinear form per channel (orb_resize_tables.h: resize_coef_host, columns clamped with their weight
//                   zeroed, rows clamped at the load with their weights kept), the rest of the S x S canvas 114.
//   blob            BlobFromImage swaps B and R in place first (:213), so blob channel c reads byte 2 - c; (((float)v) / 255.0f - mean[c]) / std[c] with mean
//                   and std held as float (:219-220) is a table of 3 x 256 floats.
//   grey            OpenCV 3.x 8-bit RGB2GRAY: (R 4899 + G 9617 + B 1868 + 8192) >> 14.
//   yolox_exp_f32   stands in for exp(feat_blob[..]) (:183-184), which resolves to glibc's expf: not correctly rounded and dispatched by CPU at run time, so the
//                   reference itself is unpinned there.  Here: the double-precision exponential rounded once to float, the same source on both sides.
//   the decode      GenerateYoloxProposals, the Hoare quicksort, NmsSortedBboxes, the rescale and clip, over PODs; std::max / std::min in their
//                   (a < b) ? b : a forms, so that NaN and infinities flow as they do upstream.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "orb_resize_tables.h"

#if defined(__HIPCC__)
#define EAO_YOLOX_HD __host__ __device__
#else
#define EAO_YOLOX_HD
#endif

namespace eao {
namespace yolox {

constexpr int kInputSize = 640;          // include/YOLOX.h:71-72
constexpr int kNumClasses = 80;          // src/YOLOX.cc:168
constexpr int kPad = 114;                // :59
constexpr int kStrides[3] = {8, 16, 32}; // :238
constexpr float kConfThresh = (float)0.3;   // BBOX_CONF_THRESH, a double literal passed on as a float (:241)
constexpr float kNmsThresh = (float)0.65;   // NMS_THRESH (:247)
constexpr float kMean[3] = {(float)0.485, (float)0.456, (float)0.406};   // :219
constexpr float kStd[3] = {(float)0.229, (float)0.224, (float)0.225};    // :220
constexpr double kTrackingMinProb = 0.5;    // src/Tracking.cc:434 (a float compared with a double literal)
constexpr int kTrackingClasses[14] = {0, 24, 28, 39, 56, 57, 58, 59, 60, 62, 63, 66, 67, 73};   // src/Tracking.cc:439
constexpr int kGrayR = 4899, kGrayG = 9617, kGrayB = 1868, kGrayShift = 14;

struct Object { float x, y, w, h, prob; int32_t label; };      // the layout of eao_yolox_object

// ---------------------------------------------------------------- geometry
struct Geometry { float r; int unpadW, unpadH; };
inline bool geometry(int cols, int rows, int S, Geometry* g) {
    if (cols < 1 || rows < 1 || S < 1) return false;
    const float r = (float)std::min(S / (cols * 1.0), S / (rows * 1.0));
    const int uw = (int)(r * (float)cols), uh = (int)(r * (float)rows);
    if (uw < 1 || uh < 1 || uw > S || uh > S) return false;      // (cv::resize asserts on an empty size)
    g->r = r; g->unpadW = uw; g->unpadH = uh;
    return true;
}

inline int num_anchors(int S) {
    int n = 0;
    for (int s : kStrides) n += (S / s) * (S / s);
    return n;
}

// ---------------------------------------------------------------- blob table, grey
inline void blob_table(float* table /* 3 x 256 */) {
    for (int c = 0; c < 3; c++)
        for (int v = 0; v < 256; v++) table[c * 256 + v] = (((float)v) / 255.0f - kMean[c]) / kStd[c];
}

EAO_YOLOX_HD inline unsigned gray_of(unsigned b0, unsigned b1, unsigned b2, bool rgb) {
    const unsigned r = rgb ? b0 : b2, b = rgb ? b2 : b0;
    return (r * (unsigned)kGrayR + b1 * (unsigned)kGrayG + b * (unsigned)kGrayB + (1u << (kGrayShift - 1))) >> kGrayShift;
}

// ---------------------------------------------------------------- letterbox
struct Tap { int32_t ofs; uint32_t wpair; };      // resize_coef_host's pair: w0 in the low half, w1 in the high one
// the S column taps and the S row taps of a geometry; entries past the unpadded size are zero and never read
inline void resize_taps(int cols, int rows, const Geometry& g, int S, Tap* xt, Tap* yt) {
    const double invX = 1. / ((double)g.unpadW / cols), invY = 1. / ((double)g.unpadH / rows);
    std::memset(xt, 0, sizeof(Tap) * (size_t)S);
    std::memset(yt, 0, sizeof(Tap) * (size_t)S);
    for (int x = 0; x < g.unpadW; x++) {
        int o; unsigned w;
        eao::orb::resize_coef_host(x, invX, cols, true, &o, &w);
        xt[x] = Tap{o, w};
    }
    for (int y = 0; y < g.unpadH; y++) {
        int o; unsigned w;
        eao::orb::resize_coef_host(y, invY, rows, false, &o, &w);
        yt[y] = Tap{o, w};
    }
}

// one channel of one canvas pixel inside the unpadded area: p00 .. p11 = the bytes at (row sy0 / sy1, column sx / sx1)
EAO_YOLOX_HD inline int bilinear_u8(int p00, int p01, int p10, int p11, unsigned aw, unsigned bw) {
    const int a0 = (short)(aw & 0xFFFFu), a1 = (short)(aw >> 16), b0 = (short)(bw & 0xFFFFu), b1 = (short)(bw >> 16);
    const int h0 = p00 * a0 + p01 * a1, h1 = p10 * a0 + p11 * a1;
    const int v = (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// StaticResize + BlobFromImage of one frame, and the grey image where wanted (gray: rows x grayStride bytes)
inline bool preprocess_literal(const uint8_t* img, int cols, int rows, int stride, int S, bool rgb, float* blob /* 3 x S x S */, uint8_t* gray, int grayStride) {
    Geometry g;
    if (!geometry(cols, rows, S, &g)) return false;
    std::vector<Tap> xt((size_t)S), yt((size_t)S);
    resize_taps(cols, rows, g, S, xt.data(), yt.data());
    std::vector<float> table(3 * 256);
    blob_table(table.data());
    for (int y = 0; y < S; y++)
        for (int x = 0; x < S; x++)
            for (int c = 0; c < 3; c++) {
                int v = kPad;
                if (x < g.unpadW && y < g.unpadH) {
                    const int sx = xt[x].ofs, sx1 = std::min(sx + 1, cols - 1);
                    const int sy0 = std::min(std::max(yt[y].ofs, 0), rows - 1), sy1 = std::min(std::max(yt[y].ofs + 1, 0), rows - 1);
                    const uint8_t *r0 = img + (size_t)sy0 * stride, *r1 = img + (size_t)sy1 * stride;
                    const int ch = 2 - c;
                    v = bilinear_u8(r0[3 * sx + ch], r0[3 * sx1 + ch], r1[3 * sx + ch], r1[3 * sx1 + ch], xt[x].wpair, yt[y].wpair);
                }
                blob[((size_t)c * S + y) * S + x] = table[c * 256 + v];
            }
    if (gray)
        for (int y = 0; y < rows; y++)
            for (int x = 0; x < cols; x++) {
                const uint8_t* p = img + (size_t)y * stride + 3 * x;
                gray[(size_t)y * grayStride + x] = (uint8_t)gray_of(p[0], p[1], p[2], rgb);
            }
    return true;
}

// ---------------------------------------------------------------- the exponential
// exp(x) in double arithmetic, rounded once to float: x = k ln2 + r with |r| <= ln2 / 2 (Cody-Waite, k ln2_hi exact), the Taylor polynomial of degree 14 in
// Horner form (its remainder is below 2^-57), 2^k from its bit pattern.  No libm call, no contraction: the same bits from g++ and from hipcc for gfx950.
// Beyond 89 the double result exceeds FLT_MAX (infinity); below -104 it is under half the smallest float denormal (zero).
EAO_YOLOX_HD inline float yolox_exp_f32(float xf) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double x = (double)xf;
    if (!(x == x)) return xf;
    if (x > 89.0) return __builtin_huge_valf();
    if (x < -104.0) return 0.0f;
    const double t = x * 1.4426950408889634074;
    const int k = (int)(t < 0.0 ? t - 0.5 : t + 0.5);
    const double kd = (double)k;
    const double r = (x - kd * 6.93147180369123816490e-01) - kd * 1.90821492927058770002e-10;
    double p = 1.1470745597729725e-11;      // 1 / 14!
    p = p * r + 1.6059043836821613e-10;     // 1 / 13!
    p = p * r + 2.08767569878681e-09;
    p = p * r + 2.505210838544172e-08;
    p = p * r + 2.755731922398589e-07;
    p = p * r + 2.7557319223985893e-06;
    p = p * r + 2.48015873015873e-05;
    p = p * r + 1.984126984126984e-04;
    p = p * r + 1.388888888888889e-03;
    p = p * r + 8.333333333333333e-03;
    p = p * r + 4.1666666666666664e-02;
    p = p * r + 1.6666666666666666e-01;
    p = p * r + 0.5;
    p = p * r + 1.0;
    p = p * r + 1.0;
    const uint64_t bits = (uint64_t)(k + 1023) << 52;      // k in -151 .. 129: a normal double
    double s;
    __builtin_memcpy(&s, &bits, 8);
    return (float)(p * s);
}

// ---------------------------------------------------------------- proposals
EAO_YOLOX_HD inline float rmax(float a, float b) { return (a < b) ? b : a; }      // std::max
EAO_YOLOX_HD inline float rmin(float a, float b) { return (b < a) ? b : a; }      // std::min

// anchor -> (grid0, grid1, stride) of GenerateGridsAndStride (:64-77): strides in order, g1 outer, g0 inner
EAO_YOLOX_HD inline void anchor_of(int anchor, int S, int* g0, int* g1, int* stride) {
    int a = anchor;
    for (int l = 0; l < 3; l++) {
        const int s = 8 << l, n = S / s;
        if (a < n * n || l == 2) {
            *g1 = a / n; *g0 = a - (a / n) * n; *stride = s;
            return;
        }
        a -= n * n;
    }
}

struct Box { float x, y, w, h; };
// :181-186 with the exponential as a parameter
template <typename Exp>
EAO_YOLOX_HD inline Box decode_box(const float* f, int g0, int g1, int stride, Exp ex) {
    const float xc = (f[0] + (float)g0) * (float)stride;
    const float yc = (f[1] + (float)g1) * (float)stride;
    const float w = ex(f[2]) * (float)stride;
    const float h = ex(f[3]) * (float)stride;
    return Box{xc - w * 0.5f, yc - h * 0.5f, w, h};
}
struct OurExp { EAO_YOLOX_HD float operator()(float v) const { return yolox_exp_f32(v); } };

template <typename Exp>
inline void generate_proposals(const float* feat, int S, int numClasses, float conf, Exp ex, std::vector<Object>& out) {
    const int A = num_anchors(S), row = 5 + numClasses;
    for (int a = 0; a < A; a++) {
        int g0, g1, stride;
        anchor_of(a, S, &g0, &g1, &stride);
        const float* f = feat + (size_t)a * row;
        const Box b = decode_box(f, g0, g1, stride, ex);
        const float objectness = f[4];
        for (int c = 0; c < numClasses; c++) {
            const float prob = objectness * f[5 + c];
            if (prob > conf) out.push_back(Object{b.x, b.y, b.w, b.h, prob, c});
        }
    }
}

// the sort key of the device path: ascending keys are descending probs (prob > conf >= 0: the bit patterns order like the values), equal probs in proposal order
EAO_YOLOX_HD inline uint64_t sort_key(uint32_t probBits, uint32_t proposalIndex) { return ((uint64_t)(~probBits) << 32) | proposalIndex; }

// ---------------------------------------------------------------- the two orders
inline void qsort_descent(std::vector<Object>& v, int left, int right) {      // :85-122; without OpenMP the two sections run one after the other
    int i = left, j = right;
    const float p = v[(size_t)((left + right) / 2)].prob;
    while (i <= j) {
        while (v[(size_t)i].prob > p) i++;
        while (v[(size_t)j].prob < p) j--;
        if (i <= j) {
            std::swap(v[(size_t)i], v[(size_t)j]);
            i++;
            j--;
        }
    }
    if (left < j) qsort_descent(v, left, j);
    if (i < right) qsort_descent(v, i, right);
}
inline void sort_literal(std::vector<Object>& v) { if (!v.empty()) qsort_descent(v, 0, (int)v.size() - 1); }
inline void sort_stable(std::vector<Object>& v) {
    std::stable_sort(v.begin(), v.end(), [](const Object& a, const Object& b) { return a.prob > b.prob; });
}
// the number of proposals that share their prob with another one
inline int count_tied(const std::vector<Object>& v) {
    std::vector<uint32_t> bits(v.size());
    for (size_t i = 0; i < v.size(); i++) std::memcpy(&bits[i], &v[i].prob, 4);
    std::sort(bits.begin(), bits.end());
    int tied = 0;
    for (size_t i = 0; i < bits.size(); i++)
        if ((i > 0 && bits[i - 1] == bits[i]) || (i + 1 < bits.size() && bits[i + 1] == bits[i])) tied++;
    return tied;
}

// ---------------------------------------------------------------- suppression
// `a` is the later box of the loop of :144-163, `b` an earlier, picked one: a.rect & b.rect (cv::Rect_<float>::operator&=), areas[i] + areas[picked[j]] - inter,
// one division, one comparison.  A NaN on either side compares false: the box is kept.
EAO_YOLOX_HD inline bool suppresses(const Box& a, const Box& b, float nms) {
    const float x1 = rmax(a.x, b.x), y1 = rmax(a.y, b.y);
    float w = rmin(a.x + a.w, b.x + b.w) - x1;
    float h = rmin(a.y + a.h, b.y + b.h) - y1;
    if (w <= 0 || h <= 0) { w = 0; h = 0; }
    const float inter = w * h;
    const float uni = a.w * a.h + b.w * b.h - inter;
    return inter / uni > nms;
}

inline void nms_sorted(const std::vector<Object>& v, float nms, std::vector<int>& picked) {
    picked.clear();
    for (int i = 0; i < (int)v.size(); i++) {
        const Box a{v[(size_t)i].x, v[(size_t)i].y, v[(size_t)i].w, v[(size_t)i].h};
        int keep = 1;
        for (int j : picked) {
            const Box b{v[(size_t)j].x, v[(size_t)j].y, v[(size_t)j].w, v[(size_t)j].h};
            if (suppresses(a, b, nms)) keep = 0;
        }
        if (keep) picked.push_back(i);
    }
}

// :258-272
EAO_YOLOX_HD inline Object rescale_clip(const Object& o, float scale, int imgW, int imgH) {
    float x0 = o.x / scale, y0 = o.y / scale, x1 = (o.x + o.w) / scale, y1 = (o.y + o.h) / scale;
    x0 = rmax(rmin(x0, (float)(imgW - 1)), 0.f);
    y0 = rmax(rmin(y0, (float)(imgH - 1)), 0.f);
    x1 = rmax(rmin(x1, (float)(imgW - 1)), 0.f);
    y1 = rmax(rmin(y1, (float)(imgH - 1)), 0.f);
    return Object{x0, y0, x1 - x0, y1 - y0, o.prob, o.label};
}

// DecodeOutputs (:235-274) of one head output.  stable = false: the reference's own order (the quicksort); true: the device's tie rule.
// proposals (optional) receives the sorted proposals.
template <typename Exp>
inline void decode_literal(const float* feat, int S, int numClasses, float conf, float nms, float scale, int imgW, int imgH, bool stable, Exp ex,
                           std::vector<Object>& objects, std::vector<Object>* proposals = nullptr) {
    std::vector<Object> prop;
    generate_proposals(feat, S, numClasses, conf, ex, prop);
    if (stable) sort_stable(prop); else sort_literal(prop);
    std::vector<int> picked;
    nms_sorted(prop, nms, picked);
    objects.resize(picked.size());
    for (size_t i = 0; i < picked.size(); i++) objects[i] = rescale_clip(prop[(size_t)picked[i]], scale, imgW, imgH);
    if (proposals) proposals->swap(prop);
}

// the rows of src/Tracking.cc:431-452: prob >= 0.5 (the float promoted to double), the class list, std::sort by score descending.  std::sort is not stable;
// rows of equal score keep their order here (any order of them is one std::sort may give).
inline bool tracking_keeps(const Object& o) {
    if ((double)o.prob < kTrackingMinProb) return false;
    for (int c : kTrackingClasses)
        if (o.label == c) return true;
    return false;
}

}  // namespace yolox
}  // namespace eao
