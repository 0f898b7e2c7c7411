// frame_objects.hip -- a frame's 2D objects on the device: steps 2, 4, 5 and 6 of the object layer (reference src/Tracking.cc:1768-1973; Tracking::AssociateObjAndPoints
// :3031-3065; Object_2D::ComputeMeanAndStandardFrame and RemoveOutliersByBoxPlot, src/Object.cc:61-157).  Bit for bit what upstream's loops compute
// (csrc/frame_objects_internal.h holds the literal form).
//
//   k_frame_features  one thread per keypoint that holds a map point: follows the host's same-id links to the LAST keypoint of that map point that lies in any
//                     box and stores its coordinates: pMP->feature after step 2 (:3053).  The links are built by the host before the upload (one pass over the ids);
//                     the any-box test and the choice are the device's.
//   k_frame_objects   one workgroup per (frame, box).
//                       1. membership in passes of kBlock keypoints: a wave ballot and a prefix count give each hit its place in the pass, a running base over
//                          the waves and the passes the place in the list: Obj_c_MapPonits in keypoint order, in LDS and in the box's slice of the scratch lists
//                       2. the positions of a chunk of the list go to LDS in parallel; lanes 0, 1 and 2 add them in list order, one coordinate each (:3059).  A
//                          dependent chain of at most 4096 float adds: the price of bit-for-bit parity, paid by three lanes while the rest of the group waits.
//                       3. z per entry in parallel; Q1 and Q3 by counting ranks: an entry is the k-th of the sorted list when #(< v) <= k < #(<= v); of the
//                          candidates (ties) the one with the smallest list position, which pins the sign of a zero
//                       4. the erase as a second ordered compaction; _Pos from the untouched sum over the new count; the squares summed like the positions; the
//                          projection of _Pos; the feature box as a min / max reduction
//                       5. num_overlaps from the integer intersection areas
//                     One lane stores the record.  No atomics: two calls return the same bytes.
//   k_frame_pack      one workgroup per box: its offset is the sum of the counts of the boxes before it; it moves its two lists from the scratch slices to
//                     their places in the packed lists and stores its starts.
//
// The host checks the frames first, and behind the download runs the sequential second loop of step 6 (remove_bad_boxes of the internal header).
#include <cstring>
#include <vector>

#include "common.h"
#include "frame_objects_internal.h"

namespace {

using namespace eao::frame_objects;

constexpr int kBlock = 256;                  // four wavefronts
constexpr int kWaves = kBlock / 64;
constexpr int kCap = kMaxKeypoints;          // a list holds at most every keypoint of its frame
constexpr int kChunk = 1024;                 // list entries whose three coordinates wait in LDS for the ordered adds

struct FrameDev {
    int32_t kpStart, nKp, boxStart, nBox;
    float T[12];      // rows 0..2 of Tcw
    float fx, fy, cx, cy;
    int32_t cols, rows, pad[2];
};
static_assert(sizeof(FrameDev) == 96, "FrameDev layout");
struct BoxDev {
    int32_t frame, x, y, w, h;
    int32_t scratch;      // the first entry of the box's slice of the scratch lists; the slice holds as many entries as the frame has keypoints with a map point
    int32_t pad[2];
};
static_assert(sizeof(BoxDev) == 32, "BoxDev layout");
static_assert(sizeof(eao_frame_object_record) == 100, "record layout");
static_assert(EAO_FRAME_OBJECTS_MAX_FRAMES <= 65535, "a frame is a y index of k_frame_features' grid");

// cv::Rect_<int>::contains(Point2f): cvRound (nearest, ties to even; |v| < 2^30 is checked by the host), then the half-open test
__device__ __forceinline__ bool box_contains(int x, int y, int w, int h, float px, float py) {
    const int ix = __float2int_rn(px), iy = __float2int_rn(py);
    return x <= ix && ix < x + w && y <= iy && iy < y + h;
}

__device__ __forceinline__ float dev_camera_row(const float* T, int r, float X0, float X1, float X2) {
    const double acc = (double)T[4 * r] * (double)X0 + (double)T[4 * r + 1] * (double)X1 + (double)T[4 * r + 2] * (double)X2;
    return (float)(acc + (double)T[4 * r + 3]);
}

__global__ __launch_bounds__(kBlock) void k_frame_features(const FrameDev* __restrict__ frames, const BoxDev* __restrict__ boxes, const float* __restrict__ kpx,
                                                           const float* __restrict__ kpy, const int32_t* __restrict__ mpid, const int32_t* __restrict__ next,
                                                           float* __restrict__ feat) {
    const FrameDev& F = frames[blockIdx.y];
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= F.nKp) return;
    const int g = F.kpStart + i;
    if (mpid[g] < 0) return;      // (never in a list: its slot is not read)
    int last = g, prev = i;
    for (int j = next[g]; j > prev && j < F.nKp; j = next[F.kpStart + j]) {      // the links ascend: the walk ends
        const int gj = F.kpStart + j;
        const float px = kpx[gj], py = kpy[gj];
        bool hit = false;
        for (int k = 0; k < F.nBox && !hit; k++) {
            const BoxDev& B = boxes[F.boxStart + k];
            hit = box_contains(B.x, B.y, B.w, B.h, px, py);
        }
        if (hit) last = gj;
        prev = j;
    }
    feat[2 * (size_t)g] = kpx[last];
    feat[2 * (size_t)g + 1] = kpy[last];
}

// One pass of an ordered compaction: the threads whose `keep` is set receive consecutive places from `base` on, in thread order; returns the new base.  Every
// thread of the workgroup calls it (two barriers).
__device__ __forceinline__ int compact_pass(bool keep, int base, int* sWave, int& place) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long m = __ballot(keep);
    if (lane == 0) sWave[wave] = __popcll(m);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kWaves; w++) {
        const int c = sWave[w];
        before += w < wave ? c : 0;
        total += c;
    }
    place = base + before + __popcll(m & ((1ull << lane) - 1ull));
    __syncthreads();      // sWave is free again
    return base + total;
}

// The three coordinates of the list's points -- or, with `squares`, (p - mean) * (p - mean) per coordinate -- summed in list order, one lane per coordinate
// (src/Tracking.cc:3059; src/Object.cc:93-95).  out[0..2] is valid for every thread after the call.
__device__ __forceinline__ void ordered_sums(const int* list, int count, int kpStart, const float* __restrict__ xyz, bool squares, const float* mean,
                                             float (*sVal)[kChunk], float* out) {
    const int t = threadIdx.x;
    float acc = 0.0f;
    for (int c0 = 0; c0 < count; c0 += kChunk) {      // (uniform)
        const int len = count - c0 < kChunk ? count - c0 : kChunk;
        for (int j = t; j < len; j += kBlock) {
            const float* p = xyz + 3 * (size_t)(kpStart + list[c0 + j]);
#pragma unroll
            for (int a = 0; a < 3; a++) {
                float v = p[a];
                if (squares) {
                    const float d = v - mean[a];
                    v = d * d;
                }
                sVal[a][j] = v;
            }
        }
        __syncthreads();
        if (t < 3)
            for (int j = 0; j < len; j++) acc = acc + sVal[t][j];
        __syncthreads();
    }
    if (t < 3) out[t] = acc;
    __syncthreads();
}

__global__ __launch_bounds__(kBlock) void k_frame_objects(const FrameDev* __restrict__ frames, const BoxDev* __restrict__ boxes, const float* __restrict__ kpx,
                                                          const float* __restrict__ kpy, const int32_t* __restrict__ mpid, const float* __restrict__ xyz,
                                                          const float* __restrict__ feat, eao_frame_object_record* __restrict__ records,
                                                          int32_t* __restrict__ scrAssigned, int32_t* __restrict__ scrKept) {
    __shared__ int sIdx[kCap];
    __shared__ int sKept[kCap];
    __shared__ float sZ[kCap];
    __shared__ float sVal[3][kChunk];
    __shared__ int sWave[kWaves];
    __shared__ int sPick[kWaves][2];
    __shared__ float sExt[kWaves][4];
    __shared__ float sSum[3], sSum2[3];
    const BoxDev B = boxes[blockIdx.x];
    const FrameDev& F = frames[B.frame];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int kpStart = F.kpStart, nKp = F.nKp;

    // 1. Obj_c_MapPonits after step 2, in keypoint order
    int nA = 0;
    for (int p0 = 0; p0 < nKp; p0 += kBlock) {      // (uniform)
        const int i = p0 + t;
        bool hit = false;
        if (i < nKp && mpid[kpStart + i] >= 0) hit = box_contains(B.x, B.y, B.w, B.h, kpx[kpStart + i], kpy[kpStart + i]);
        int place;
        nA = compact_pass(hit, nA, sWave, place);
        if (hit) {      // place < the frame's keypoints with a map point <= kCap: inside the LDS list and inside the box's scratch slice
            sIdx[place] = i;
            scrAssigned[(size_t)B.scratch + place] = i;
        }
    }
    __syncthreads();

    // 2. sum_pos_3d
    ordered_sums(sIdx, nA, kpStart, xyz, false, nullptr, sVal, sSum);

    // 3. the boxplot's thresholds
    const bool ran = nA >= kBoxplotMinPoints;
    float q1 = 0.0f, q3 = 0.0f, maxTh = 0.0f;
    for (int p = t; p < nA; p += kBlock) {
        const float* X = xyz + 3 * (size_t)(kpStart + sIdx[p]);
        sZ[p] = dev_camera_row(F.T, 2, X[0], X[1], X[2]);
    }
    __syncthreads();
    if (ran) {      // (uniform)
        const int k1 = nA / kQuartileDivisor, k3 = nA * 3 / kQuartileDivisor;
        int c1 = kCap, c3 = kCap;
        for (int p = t; p < nA; p += kBlock) {
            const float v = sZ[p];
            int lt = 0, le = 0;
            for (int q = 0; q < nA; q++) {
                const float z = sZ[q];
                lt += z < v ? 1 : 0;
                le += z <= v ? 1 : 0;
            }
            if (lt <= k1 && k1 < le && p < c1) c1 = p;
            if (lt <= k3 && k3 < le && p < c3) c3 = p;
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const int a = __shfl_xor(c1, d, 64), b = __shfl_xor(c3, d, 64);
            c1 = a < c1 ? a : c1;
            c3 = b < c3 ? b : c3;
        }
        if (lane == 0) { sPick[wave][0] = c1; sPick[wave][1] = c3; }
        __syncthreads();
        c1 = c3 = kCap;
#pragma unroll
        for (int w = 0; w < kWaves; w++) {
            c1 = sPick[w][0] < c1 ? sPick[w][0] : c1;
            c3 = sPick[w][1] < c3 ? sPick[w][1] : c3;
        }
        // (z has no NaN -- the host refuses non-finite input and the double products cannot overflow --, so both ranks are found: c1, c3 < nA)
        q1 = sZ[c1 < nA ? c1 : 0];
        q3 = sZ[c3 < nA ? c3 : 0];
        const float iqr = q3 - q1;
        maxTh = (float)((double)q3 + kIqrFactor * (double)iqr);
    }

    // 4. the erase, in list order
    int n = 0;
    for (int p0 = 0; p0 < nA; p0 += kBlock) {      // (uniform)
        const int p = p0 + t;
        const bool keep = p < nA && !(ran && sZ[p] > maxTh);
        int place;
        n = compact_pass(keep, n, sWave, place);
        if (keep) {      // place <= p
            const int i = sIdx[p];
            sKept[place] = i;
            scrKept[(size_t)B.scratch + place] = i;
        }
    }
    __syncthreads();

    float pos[3];
    {
        const float alpha = (float)(1.0 / (double)n);      // cv::Mat / n: convertTo with alpha = 1.0 / n (n == 0: 0 * inf = NaN, as upstream)
#pragma unroll
        for (int a = 0; a < 3; a++) pos[a] = sSum[a] * alpha + 0.0f;
    }
    ordered_sums(sKept, n, kpStart, xyz, true, pos, sVal, sSum2);

    // the feature box: min / max of pMP->feature over the list
    float xMin = INFINITY, xMax = -INFINITY, yMin = INFINITY, yMax = -INFINITY;
    for (int p = t; p < n; p += kBlock) {
        const size_t g = (size_t)(kpStart + sKept[p]);
        const float u = feat[2 * g], v = feat[2 * g + 1];
        xMin = u < xMin ? u : xMin;
        xMax = u > xMax ? u : xMax;
        yMin = v < yMin ? v : yMin;
        yMax = v > yMax ? v : yMax;
    }
    // 5. the first loop of step 6
    int num = 0;
    for (int l = t; l < F.nBox; l += kBlock) {
        const BoxDev& C = boxes[F.boxStart + l];
        if (F.boxStart + l == (int)blockIdx.x) continue;
        const int x1 = B.x > C.x ? B.x : C.x, y1 = B.y > C.y ? B.y : C.y;
        const int x2 = B.x + B.w < C.x + C.w ? B.x + B.w : C.x + C.w, y2 = B.y + B.h < C.y + C.h ? B.y + B.h : C.y + C.h;
        const int w = x2 - x1, h = y2 - y1;
        const int overlap = (w <= 0 || h <= 0) ? 0 : w * h;
        const float ratio = (float)overlap / ((float)(C.w * C.h));
        num += (double)ratio > kCrowdRatio ? 1 : 0;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const float a = __shfl_xor(xMin, d, 64), b = __shfl_xor(xMax, d, 64), c = __shfl_xor(yMin, d, 64), e = __shfl_xor(yMax, d, 64);
        xMin = a < xMin ? a : xMin;
        xMax = b > xMax ? b : xMax;
        yMin = c < yMin ? c : yMin;
        yMax = e > yMax ? e : yMax;
        num += __shfl_xor(num, d, 64);
    }
    if (lane == 0) {
        sExt[wave][0] = xMin; sExt[wave][1] = xMax; sExt[wave][2] = yMin; sExt[wave][3] = yMax;
        sPick[wave][0] = num;
    }
    __syncthreads();
    if (t == 0) {
        num = 0;
#pragma unroll
        for (int w = 0; w < kWaves; w++) {
            xMin = w == 0 || sExt[w][0] < xMin ? sExt[w][0] : xMin;
            xMax = w == 0 || sExt[w][1] > xMax ? sExt[w][1] : xMax;
            yMin = w == 0 || sExt[w][2] < yMin ? sExt[w][2] : yMin;
            yMax = w == 0 || sExt[w][3] > yMax ? sExt[w][3] : yMax;
            num += sPick[w][0];
        }
        eao_frame_object_record r;
        r.n_assigned = nA;
        r.n = n;
#pragma unroll
        for (int a = 0; a < 3; a++) {
            r.sum_pos[a] = sSum[a];
            r.pos[a] = pos[a];
            const float q = sSum2[a] / (float)n;
            r.std[a] = (float)sqrt((double)q);      // (sqrt through double is the same float)
        }
        r.q1 = q1; r.q3 = q3; r.max_th = maxTh;
        r.boxplot_ran = ran ? 1 : 0;
        const float xc = dev_camera_row(F.T, 0, pos[0], pos[1], pos[2]), yc = dev_camera_row(F.T, 1, pos[0], pos[1], pos[2]);
        const float zc = dev_camera_row(F.T, 2, pos[0], pos[1], pos[2]);
        const float invzc = (float)(1.0 / (double)zc);
        r.center_2d[0] = F.fx * xc * invzc + F.cx;
        r.center_2d[1] = F.fy * yc * invzc + F.cy;
        r.has_feature_rect = 0;
        r.feature_rect[0] = r.feature_rect[1] = r.feature_rect[2] = r.feature_rect[3] = 0;
        if (n >= kFeatureRectMinPoints) {
            if (xMin < 0) xMin = 0;
            if (yMin < 0) yMin = 0;
            if (xMax > (float)F.cols) xMax = (float)F.cols;
            if (yMax > (float)F.rows) yMax = (float)F.rows;
            r.has_feature_rect = 1;
            r.feature_rect[0] = (int)xMin;      // (|kp| < 2^30: the truncations are defined)
            r.feature_rect[1] = (int)yMin;
            r.feature_rect[2] = (int)(xMax - xMin);
            r.feature_rect[3] = (int)(yMax - yMin);
        }
        r.num_overlaps = num;
        r.bad = 0;
        r.on_edge = 0;
        records[blockIdx.x] = r;
    }
}

__global__ __launch_bounds__(kBlock) void k_frame_pack(int nBoxes, const BoxDev* __restrict__ boxes, const eao_frame_object_record* __restrict__ records,
                                                       const int32_t* __restrict__ scrAssigned, const int32_t* __restrict__ scrKept, int32_t* __restrict__ startA,
                                                       int32_t* __restrict__ startK, int32_t* __restrict__ outA, int32_t* __restrict__ outK) {
    __shared__ int sPart[kWaves][2];
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    int offA = 0, offK = 0;
    for (int j = t; j < b; j += kBlock) {
        offA += records[j].n_assigned;
        offK += records[j].n;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        offA += __shfl_xor(offA, d, 64);
        offK += __shfl_xor(offK, d, 64);
    }
    if (lane == 0) { sPart[wave][0] = offA; sPart[wave][1] = offK; }
    __syncthreads();
    offA = offK = 0;
#pragma unroll
    for (int w = 0; w < kWaves; w++) {
        offA += sPart[w][0];
        offK += sPart[w][1];
    }
    const int nA = records[b].n_assigned, n = records[b].n;
    const size_t from = (size_t)boxes[b].scratch;
    // (the packed lists are as long as the scratch lists, and every box's counts fit its slice: offA + nA <= the sum of the slices up to this box's)
    for (int p = t; p < nA; p += kBlock) outA[(size_t)offA + p] = scrAssigned[from + p];
    for (int p = t; p < n; p += kBlock) outK[(size_t)offK + p] = scrKept[from + p];
    if (t == 0) {
        startA[b] = offA;
        startK[b] = offK;
        if (b == nBoxes - 1) {
            startA[nBoxes] = offA + nA;
            startK[nBoxes] = offK + n;
        }
    }
}

struct FrameObjectsCtx : eao::ThreadStream {
    eao::DevBuf<unsigned char> dev;
    eao::PinBuf<hipHostMallocDefault> host;
    eao::KernelClock<3> clock;      // k_frame_features, k_frame_objects, k_frame_pack of the last call that reached the device
};
thread_local FrameObjectsCtx g_fo;

constexpr int64_t kMaxScratch = (int64_t)1 << 30;      // entries of one scratch list: the offsets are int32
constexpr size_t kOneDownloadBytes = 512 * 1024;       // a frame of 1500 keypoints and 16 boxes: 2 x 16 x 1350 entries, 173 KB

}  // namespace

extern "C" {

eao_status eao_frame_objects_batch(int32_t n_frames, const eao_frame_objects_desc* frames, const eao_frame_objects_out* out) {
    EAO_REQUIRE(n_frames >= 0 && n_frames <= EAO_FRAME_OBJECTS_MAX_FRAMES, "n_frames outside 0 .. %d", EAO_FRAME_OBJECTS_MAX_FRAMES);
    EAO_REQUIRE(out, "null argument");
    EAO_REQUIRE(n_frames == 0 || frames, "null argument");
    EAO_REQUIRE(out->assigned_start && out->kept_start, "assigned_start or kept_start is NULL");
    EAO_REQUIRE(out->assigned_cap >= 0 && out->kept_cap >= 0, "a negative capacity");
    EAO_REQUIRE((out->assigned_cap == 0 || out->assigned) && (out->kept_cap == 0 || out->kept), "a list buffer is NULL");
    int64_t nBoxes = 0, nKps = 0, nScratch = 0;
    int32_t maxKp = 0;
    std::vector<int32_t> valid((size_t)n_frames, 0);
    for (int32_t f = 0; f < n_frames; f++) {
        const char* why = frame_refusal(frames[f]);
        EAO_REQUIRE(!why, "frame %d: %s", f, why);
        for (int32_t i = 0; i < frames[f].n_kp; i++) valid[f] += frames[f].mp_id[i] >= 0 ? 1 : 0;
        nBoxes += frames[f].n_box;
        nKps += frames[f].n_kp;
        nScratch += (int64_t)frames[f].n_box * valid[f];
        maxKp = frames[f].n_kp > maxKp ? frames[f].n_kp : maxKp;
        EAO_REQUIRE(nScratch <= kMaxScratch && nKps <= kMaxScratch, "the batch's lists could exceed 2^30 entries: split the call");
    }
    EAO_REQUIRE(nBoxes == 0 || out->records, "records is NULL");
    if (nBoxes == 0) {
        out->assigned_start[0] = 0;
        out->kept_start[0] = 0;
        return EAO_OK;
    }

    FrameObjectsCtx& ctx = g_fo;
    eao_status st = ctx.ready(eao::StreamClass::Latency);
    if (st) return st;
    const size_t nK = (size_t)nKps, nB = (size_t)nBoxes, nS = (size_t)nScratch;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t at = off; off = eao::align256(off + bytes); return at; };
    const size_t oFrames = take((size_t)n_frames * sizeof(FrameDev)), oBoxes = take(nB * sizeof(BoxDev)), oKpx = take(nK * 4), oKpy = take(nK * 4), oId = take(nK * 4);
    const size_t oNext = take(nK * 4), oXyz = take(nK * 12), inEnd = off;
    const size_t oFeat = take(nK * 8), oScrA = take(nS * 4), oScrK = take(nS * 4);
    const size_t oRec = take(nB * sizeof(eao_frame_object_record)), oStartA = take((nB + 1) * 4), oStartK = take((nB + 1) * 4), smallEnd = off;
    const size_t oOutA = take(nS * 4), oOutK = take(nS * 4), end = off;
    if ((st = ctx.dev.reserve(end))) return st;
    if ((st = ctx.host.reserve(end))) return st;
    unsigned char *d = ctx.dev.p, *h = ctx.host.p;
    FrameDev* hf = (FrameDev*)(h + oFrames);
    BoxDev* hb = (BoxDev*)(h + oBoxes);
    int32_t kp = 0, box = 0, scratch = 0;
    for (int32_t f = 0; f < n_frames; f++) {
        const eao_frame_objects_desc& F = frames[f];
        FrameDev D{};
        D.kpStart = kp; D.nKp = F.n_kp; D.boxStart = box; D.nBox = F.n_box;
        std::memcpy(D.T, F.Tcw, sizeof(D.T));
        D.fx = F.fx; D.fy = F.fy; D.cx = F.cx; D.cy = F.cy;
        D.cols = F.cols; D.rows = F.rows;
        hf[f] = D;
        if (F.n_kp > 0) {
            std::memcpy(h + oKpx + (size_t)kp * 4, F.kp_x, (size_t)F.n_kp * 4);
            std::memcpy(h + oKpy + (size_t)kp * 4, F.kp_y, (size_t)F.n_kp * 4);
            std::memcpy(h + oId + (size_t)kp * 4, F.mp_id, (size_t)F.n_kp * 4);
            std::memcpy(h + oXyz + (size_t)kp * 12, F.mp_xyz, (size_t)F.n_kp * 12);
            same_id_links(F.n_kp, F.mp_id, (int32_t*)(h + oNext) + kp);
        }
        for (int32_t k = 0; k < F.n_box; k++) {
            BoxDev B{};
            B.frame = f;
            B.x = F.boxes[4 * k]; B.y = F.boxes[4 * k + 1]; B.w = F.boxes[4 * k + 2]; B.h = F.boxes[4 * k + 3];
            B.scratch = scratch;
            hb[box + k] = B;
            scratch += valid[f];
        }
        kp += F.n_kp;
        box += F.n_box;
    }
    eao::Drain drain(ctx.stream);
    EAO_HIP(hipMemcpyAsync(d, h, inEnd, hipMemcpyHostToDevice, ctx.stream));
    ctx.clock.mark(0, ctx.stream);
    if (maxKp > 0)
        hipLaunchKernelGGL(k_frame_features, dim3((unsigned)eao::cdiv(maxKp, kBlock), (unsigned)n_frames), dim3(kBlock), 0, ctx.stream, (const FrameDev*)(d + oFrames),
                           (const BoxDev*)(d + oBoxes), (const float*)(d + oKpx), (const float*)(d + oKpy), (const int32_t*)(d + oId), (const int32_t*)(d + oNext),
                           (float*)(d + oFeat));
    EAO_HIP(hipGetLastError());
    ctx.clock.mark(1, ctx.stream);
    hipLaunchKernelGGL(k_frame_objects, dim3((unsigned)nB), dim3(kBlock), 0, ctx.stream, (const FrameDev*)(d + oFrames), (const BoxDev*)(d + oBoxes),
                       (const float*)(d + oKpx), (const float*)(d + oKpy), (const int32_t*)(d + oId), (const float*)(d + oXyz), (const float*)(d + oFeat),
                       (eao_frame_object_record*)(d + oRec), (int32_t*)(d + oScrA), (int32_t*)(d + oScrK));
    EAO_HIP(hipGetLastError());
    ctx.clock.mark(2, ctx.stream);
    hipLaunchKernelGGL(k_frame_pack, dim3((unsigned)nB), dim3(kBlock), 0, ctx.stream, (int)nB, (const BoxDev*)(d + oBoxes), (const eao_frame_object_record*)(d + oRec),
                       (const int32_t*)(d + oScrA), (const int32_t*)(d + oScrK), (int32_t*)(d + oStartA), (int32_t*)(d + oStartK), (int32_t*)(d + oOutA),
                       (int32_t*)(d + oOutK));
    EAO_HIP(hipGetLastError());
    ctx.clock.mark(3, ctx.stream);
    // records, starts and packed lists lie back to back: a call whose lists are short takes them in ONE download and one wait; otherwise the starts come first
    // and say how much of the lists to fetch
    const bool oneDownload = end - oRec <= kOneDownloadBytes;
    EAO_HIP(hipMemcpyAsync(h + oRec, d + oRec, (oneDownload ? end : smallEnd) - oRec, hipMemcpyDeviceToHost, ctx.stream));
    EAO_HIP(drain.wait_more(eao::Drain::Latency));
    ctx.clock.collect();
    const int32_t *sa = (const int32_t*)(h + oStartA), *sk = (const int32_t*)(h + oStartK);
    const size_t totalA = (size_t)sa[nB], totalK = (size_t)sk[nB];
    if (totalA > nS || totalK > totalA) {
        drain.disarm();
        eao::set_error("the device's list lengths are inconsistent");
        return EAO_ERR_INTERNAL;
    }
    if ((int64_t)totalA > out->assigned_cap || (int64_t)totalK > out->kept_cap) {
        drain.disarm();      // (the stream is empty)
        std::memcpy(out->assigned_start, sa, (nB + 1) * 4);
        std::memcpy(out->kept_start, sk, (nB + 1) * 4);
        eao::set_error("the lists need %zu and %zu entries, the buffers hold %lld and %lld", totalA, totalK, (long long)out->assigned_cap, (long long)out->kept_cap);
        return EAO_ERR_CAPACITY;
    }
    if (oneDownload) {
        drain.disarm();      // (the stream is empty)
    } else {
        if (totalA > 0) EAO_HIP(hipMemcpyAsync(h + oOutA, d + oOutA, totalA * 4, hipMemcpyDeviceToHost, ctx.stream));
        if (totalK > 0) EAO_HIP(hipMemcpyAsync(h + oOutK, d + oOutK, totalK * 4, hipMemcpyDeviceToHost, ctx.stream));
        EAO_HIP(drain.wait(eao::Drain::Latency));
    }
    // the sequential loops of step 6, per frame (src/Tracking.cc:1879-1945)
    eao_frame_object_record* rec = (eao_frame_object_record*)(h + oRec);
    box = 0;
    for (int32_t f = 0; f < n_frames; f++) {
        remove_bad_boxes(frames[f].n_box, frames[f].boxes, frames[f].score, frames[f].cols, frames[f].rows, rec + box);
        box += frames[f].n_box;
    }
    std::memcpy(out->records, rec, nB * sizeof(eao_frame_object_record));
    std::memcpy(out->assigned_start, sa, (nB + 1) * 4);
    std::memcpy(out->kept_start, sk, (nB + 1) * 4);
    if (totalA > 0) std::memcpy(out->assigned, h + oOutA, totalA * 4);
    if (totalK > 0) std::memcpy(out->kept, h + oOutK, totalK * 4);
    return EAO_OK;
}

eao_status eao_frame_objects(const eao_frame_objects_desc* frame, const eao_frame_objects_out* out) {
    EAO_REQUIRE(frame, "null argument");
    return eao_frame_objects_batch(1, frame, out);
}

eao_status eao_frame_objects_set_profiling(int32_t on) {
    g_fo.clock.arm(on != 0);
    return EAO_OK;
}

eao_status eao_frame_objects_last_kernel_ms(float* kernel_ms) {
    EAO_REQUIRE(kernel_ms, "null argument");
    return g_fo.clock.read(kernel_ms, "no measurement on this thread: eao_frame_objects_set_profiling(1) and a call with at least one box come first");
}

}  // extern "C"
