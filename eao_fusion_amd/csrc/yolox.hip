// yolox.hip -- what YOLOX::Detect does around the network, on the device (reference src/YOLOX.cc:51-62 StaticResize, :211-233 BlobFromImage, :235-274 DecodeOutputs;
// the grey image of src/Tracking.cc:324-330).  The arithmetic is stated once in csrc/yolox_internal.h and shared with the host's literal form.
//
//   k_yolox_pre        one pass over the S x S canvas, four pixels per lane: three bilinear taps from the interleaved source (the 11-bit fixed-point form of
//                      resize_item in orb.hip, per channel; the taps come from the host, per geometry) or the pad value, three planar float4 stores through the
//                      3 x 256 table (in LDS).  Behind the canvas items, where a grey image is wanted: four source pixels per lane, one 4-byte store into a
//                      pitched buffer that eao_orb_extract_batch_device reads directly.
//   k_yolox_proposals  one wavefront per anchor, a lane per class: box_prob = objectness * cls, kept when > conf; the survivors of a wave take their slots with
//                      one atomic add (ballot + prefix count) and store (key, box), key = (~bits(prob) << 32) | (anchor * classes + class).  Slots past the
//                      capacity are counted and not stored.
//   k_yolox_rank       the sort: keys are distinct, so the rank of a key is the number of smaller ones -- every lane counts them over LDS tiles and scatters its
//                      record.  The same pass counts the proposals whose prob another one shares.
//   k_yolox_mask       the n x ceil(n / 64) suppression bit matrix of the sorted boxes: bit (i, j), j > i, is suppresses(box j, box i).
//   k_yolox_scan       one wavefront replays the greedy loop: the rows are fetched eight ahead whatever the verdicts, only the OR depends on them; the picked boxes
//                      are rescaled and clipped by all lanes.
// The batch is a grid dimension of every kernel.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "common.h"
#include "yolox_internal.h"

namespace {

using namespace eao::yolox;

static_assert(sizeof(Object) == sizeof(eao_yolox_object) && sizeof(Object) == 24, "eao_yolox_object and yolox_internal.h state the same record");
static_assert(kInputSize == EAO_YOLOX_INPUT_SIZE && kNumClasses == EAO_YOLOX_NUM_CLASSES && kPad == EAO_YOLOX_PAD, "include/eao_fusion.h and yolox_internal.h agree");

constexpr int kMaxProposals = EAO_YOLOX_MAX_PROPOSALS;      // 16384: 256 words per matrix row, four per lane of the scan
constexpr int kWordsPerLane = kMaxProposals / 64 / 64;
constexpr int kScanAhead = 8;
constexpr int kCounts = 4;      // per frame: proposals, objects, tied, unused

struct FrameInfo { float scale; int imgW, imgH, pad; };

struct PreArgs {
    const uint8_t* src; int cols, rows, stride; long long frameStride;
    float* blob; uint8_t* gray; int grayStride; long long grayFrameStride;
    int S, unpadW, unpadH, rgb;
    const Tap* xt; const Tap* yt; const float* lut;
    int canvasItems, grayGroups, grayG4;
};

__global__ __launch_bounds__(256) void k_yolox_pre(PreArgs A) {
    __shared__ float lut[3 * 256];
    for (int k = threadIdx.x; k < 3 * 256; k += 256) lut[k] = A.lut[k];
    __syncthreads();
    const int f = blockIdx.y;
    const int item = blockIdx.x * 256 + threadIdx.x;
    const uint8_t* src = A.src + (long long)f * A.frameStride;
    if (item < A.canvasItems) {
        const int S4 = A.S >> 2;
        const int y = item / S4, x0 = (item - y * S4) * 4;
        float out[3][4];
        const bool rowIn = y < A.unpadH;
        const uint8_t *r0 = src, *r1 = src;
        unsigned bw = 0;
        if (rowIn) {
            const Tap ty = A.yt[y];
            r0 = src + (long long)min(max(ty.ofs, 0), A.rows - 1) * A.stride;
            r1 = src + (long long)min(max(ty.ofs + 1, 0), A.rows - 1) * A.stride;
            bw = ty.wpair;
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int x = x0 + i;
            if (rowIn && x < A.unpadW) {
                const Tap tx = A.xt[x];
                const int o0 = 3 * tx.ofs, o1 = 3 * min(tx.ofs + 1, A.cols - 1);
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    const int ch = 2 - c;      // BlobFromImage swaps B and R first
                    out[c][i] = lut[c * 256 + bilinear_u8(r0[o0 + ch], r0[o1 + ch], r1[o0 + ch], r1[o1 + ch], tx.wpair, bw)];
                }
            } else {
#pragma unroll
                for (int c = 0; c < 3; c++) out[c][i] = lut[c * 256 + kPad];
            }
        }
        float* b = A.blob + (size_t)f * 3 * A.S * A.S + (size_t)y * A.S + x0;
#pragma unroll
        for (int c = 0; c < 3; c++) *reinterpret_cast<float4*>(b + (size_t)c * A.S * A.S) = make_float4(out[c][0], out[c][1], out[c][2], out[c][3]);
    } else if (A.gray) {
        const int g = item - A.canvasItems;
        if (g >= A.grayGroups) return;
        const int y = g / A.grayG4, x0 = (g - y * A.grayG4) * 4;
        const uint8_t* p = src + (long long)y * A.stride + 3 * x0;
        unsigned packed = 0;
#pragma unroll
        for (int i = 0; i < 4; i++)
            if (x0 + i < A.cols) packed |= gray_of(p[3 * i], p[3 * i + 1], p[3 * i + 2], A.rgb != 0) << (8 * i);
        // (the pitch is a multiple of 64: the tail of a row's last word lands in its padding)
        *reinterpret_cast<unsigned*>(A.gray + (long long)f * A.grayFrameStride + (long long)y * A.grayStride + x0) = packed;
    }
}

__device__ __forceinline__ unsigned below(unsigned long long mask, int lane) { return __popcll(mask & ((1ull << lane) - 1ull)); }

__global__ __launch_bounds__(256) void k_yolox_proposals(const float* __restrict__ prob, int S, int nAnchors, int nc, float conf, unsigned cap,
                                                         unsigned* __restrict__ counts, unsigned long long* __restrict__ keys, float4* __restrict__ boxes) {
    const int f = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int a = blockIdx.x * 4 + wave;
    if (a >= nAnchors) return;      // (per wavefront: nothing below waits for another one)
    const float* fp = prob + ((size_t)f * nAnchors + a) * (size_t)(5 + nc);
    int g0, g1, stride;
    anchor_of(a, S, &g0, &g1, &stride);
    const Box b = decode_box(fp, g0, g1, stride, OurExp{});
    const float objectness = fp[4];
    for (int c0 = 0; c0 < nc; c0 += 64) {
        const int c = c0 + lane;
        const bool on = c < nc;
        const float p = on ? objectness * fp[5 + c] : 0.f;
        const bool keep = on && p > conf;
        const unsigned long long m = __ballot(keep);
        if (!m) continue;
        unsigned base = 0;
        if (lane == 0) base = atomicAdd(&counts[f * kCounts], (unsigned)__popcll(m));
        base = __shfl(base, 0, 64);
        const unsigned pos = base + below(m, lane);
        if (keep && pos < cap) {
            keys[(size_t)f * cap + pos] = sort_key(__float_as_uint(p), (unsigned)(a * nc + c));
            boxes[(size_t)f * cap + pos] = make_float4(b.x, b.y, b.w, b.h);
        }
    }
}

__global__ __launch_bounds__(256) void k_yolox_rank(unsigned cap, unsigned* __restrict__ counts, const unsigned long long* __restrict__ keys,
                                                    const float4* __restrict__ boxes, unsigned long long* __restrict__ skeys, float4* __restrict__ sboxes) {
    __shared__ unsigned long long sh[256];
    const int f = blockIdx.y, tid = threadIdx.x;
    const unsigned n = counts[f * kCounts];
    if (n > cap || blockIdx.x * 256u >= n) return;      // (per block)
    const unsigned i = blockIdx.x * 256u + tid;
    const unsigned long long* K = keys + (size_t)f * cap;
    // the filler is above every key and shares its upper half with none: a kept prob is > 0, so the upper half of its key is not all ones
    const unsigned long long my = i < n ? K[i] : ~0ull;
    unsigned rank = 0;
    bool tied = false;
    for (unsigned t = 0; t < n; t += 256) {
        sh[tid] = t + tid < n ? K[t + tid] : ~0ull;
        __syncthreads();
#pragma unroll 8
        for (int q = 0; q < 256; q++) {
            const unsigned long long k = sh[q];
            rank += k < my ? 1u : 0u;
            tied = tied || ((unsigned)(k >> 32) == (unsigned)(my >> 32) && k != my);
        }
        __syncthreads();
    }
    if (i < n) {
        skeys[(size_t)f * cap + rank] = my;
        sboxes[(size_t)f * cap + rank] = boxes[(size_t)f * cap + i];
    }
    const unsigned long long tm = __ballot(tied && i < n);
    if ((tid & 63) == 0 && tm) atomicAdd(&counts[f * kCounts + 2], (unsigned)__popcll(tm));
}

__global__ __launch_bounds__(64) void k_yolox_mask(unsigned cap, unsigned wstride, float nms, const unsigned* __restrict__ counts, const float4* __restrict__ sboxes,
                                                   unsigned long long* __restrict__ mask) {
    __shared__ float4 cb[64];
    const int f = blockIdx.y, lane = threadIdx.x;
    const unsigned n = counts[f * kCounts];
    const unsigned rb = blockIdx.x;
    if (n > cap || rb * 64u >= n) return;
    const unsigned W = (n + 63u) >> 6;
    const float4* B = sboxes + (size_t)f * cap;
    const unsigned i = rb * 64u + lane;
    const bool on = i < n;
    const float4 mine = on ? B[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    const Box earlier{mine.x, mine.y, mine.z, mine.w};
    for (unsigned c = 0; c < W; c++) {
        unsigned long long word = 0;
        if (c >= rb) {
            const unsigned j0 = c * 64u;
            cb[lane] = j0 + lane < n ? B[j0 + lane] : make_float4(0.f, 0.f, 0.f, 0.f);
            eao::wave_sync();
            if (on)
                for (unsigned q = 0; q < 64; q++) {
                    const unsigned j = j0 + q;
                    if (j > i && j < n) {
                        const float4 v = cb[q];
                        if (suppresses(Box{v.x, v.y, v.z, v.w}, earlier, nms)) word |= 1ull << q;
                    }
                }
            eao::wave_sync();
        }
        if (on) mask[((size_t)f * cap + i) * wstride + c] = word;
    }
}

__global__ __launch_bounds__(64) void k_yolox_scan(unsigned cap, unsigned wstride, int nc, unsigned* __restrict__ counts, const unsigned long long* __restrict__ skeys,
                                                   const float4* __restrict__ sboxes, const unsigned long long* __restrict__ mask, int* __restrict__ picked,
                                                   const FrameInfo* __restrict__ info, Object* __restrict__ objs) {
    const int f = blockIdx.x, lane = threadIdx.x;
    const unsigned n = counts[f * kCounts];
    if (n > cap) return;
    const unsigned W = (n + 63u) >> 6;
    const unsigned long long* M = mask + (size_t)f * cap * wstride;
    int* P = picked + (size_t)f * cap;
    unsigned long long rem[kWordsPerLane];
#pragma unroll
    for (int k = 0; k < kWordsPerLane; k++) rem[k] = 0;
    unsigned np = 0;
    for (unsigned i0 = 0; i0 < n; i0 += kScanAhead) {
        unsigned long long row[kScanAhead][kWordsPerLane];
#pragma unroll
        for (int r = 0; r < kScanAhead; r++)
#pragma unroll
            for (int k = 0; k < kWordsPerLane; k++) {
                const unsigned w = (unsigned)lane + 64u * k;
                row[r][k] = (i0 + r < n && w < W) ? M[(size_t)(i0 + r) * wstride + w] : 0ull;
            }
#pragma unroll
        for (int r = 0; r < kScanAhead; r++) {
            const unsigned i = i0 + r;
            if (i < n) {      // (wave-uniform)
                const unsigned wi = i >> 6, slot = wi >> 6;
                unsigned long long v = rem[0];
#pragma unroll
                for (int k = 1; k < kWordsPerLane; k++) v = slot == (unsigned)k ? rem[k] : v;
                const unsigned long long word = __shfl(v, (int)(wi & 63u), 64);
                if (!((word >> (i & 63u)) & 1ull)) {
                    if (lane == 0) P[np] = (int)i;
                    np++;
#pragma unroll
                    for (int k = 0; k < kWordsPerLane; k++) rem[k] |= row[r][k];
                }
            }
        }
    }
    eao::wave_sync();
    const FrameInfo I = info[f];
    for (unsigned p = lane; p < np; p += 64) {
        const int idx = P[p];
        const unsigned long long key = skeys[(size_t)f * cap + idx];
        const float4 b = sboxes[(size_t)f * cap + idx];
        const Object o{b.x, b.y, b.z, b.w, __uint_as_float(~(unsigned)(key >> 32)), (int)((unsigned)key % (unsigned)nc)};
        objs[(size_t)f * cap + p] = rescale_clip(o, I.scale, I.imgW, I.imgH);
    }
    if (lane == 0) counts[f * kCounts + 1] = np;
}

}  // namespace

struct eao_yolox {
    std::mutex mutex;
    eao_yolox_cfg cfg;
    int S = 0, A = 0, row = 0, cap = 0, wstride = 0;
    hipStream_t stream = nullptr;
    eao::DevBuf<float> lut, blob, prob;
    eao::DevBuf<Tap> taps;                      // S column taps, then S row taps, of the geometry below
    eao::DevBuf<unsigned char> frames, gray;
    eao::DevBuf<unsigned> counts;
    eao::DevBuf<unsigned long long> keys, skeys, mask;
    eao::DevBuf<float4> boxes, sboxes;
    eao::DevBuf<int> picked;
    eao::DevBuf<Object> objs;
    eao::DevBuf<FrameInfo> info;
    int geoCols = 0, geoRows = 0;
    Geometry geo{};
    int blobFrames = 0, decoded = 0;            // frames of the last host pre-processing / of the last decode that did not overflow
    std::vector<unsigned> lastCounts;
    eao::KernelClock<5> clock;
    ~eao_yolox() { if (stream) (void)hipStreamDestroy(stream); }
};

namespace {

// the taps of (cols, rows) on the device; a change of geometry waits for whatever still reads the old ones
eao_status set_geometry(eao_yolox* h, int cols, int rows) {
    if (h->geoCols == cols && h->geoRows == rows) return EAO_OK;
    Geometry g;
    EAO_REQUIRE(geometry(cols, rows, h->S, &g), "a %d x %d frame has no letterbox in %d x %d (an empty resize)", cols, rows, h->S, h->S);
    std::vector<Tap> t((size_t)2 * h->S);
    resize_taps(cols, rows, g, h->S, t.data(), t.data() + h->S);
    EAO_HIP(hipDeviceSynchronize());
    EAO_HIP(hipMemcpy(h->taps.p, t.data(), t.size() * sizeof(Tap), hipMemcpyHostToDevice));
    h->geo = g; h->geoCols = cols; h->geoRows = rows;
    return EAO_OK;
}

eao_status launch_pre(eao_yolox* h, const uint8_t* dSrc, int cols, int rows, int stride, long long frameStride, int batch, int rgb, float* dBlob, uint8_t* dGray,
                      int grayStride, hipStream_t s) {
    PreArgs a{};
    a.src = dSrc; a.cols = cols; a.rows = rows; a.stride = stride; a.frameStride = frameStride;
    a.blob = dBlob; a.gray = dGray; a.grayStride = grayStride; a.grayFrameStride = (long long)grayStride * rows;
    a.S = h->S; a.unpadW = h->geo.unpadW; a.unpadH = h->geo.unpadH; a.rgb = rgb;
    a.xt = h->taps.p; a.yt = h->taps.p + h->S; a.lut = h->lut.p;
    a.canvasItems = h->S * h->S / 4;
    a.grayG4 = eao::cdiv(cols, 4);
    a.grayGroups = dGray ? a.grayG4 * rows : 0;
    h->clock.mark(0, s);
    hipLaunchKernelGGL(k_yolox_pre, dim3((unsigned)eao::cdiv(a.canvasItems + a.grayGroups, 256), (unsigned)batch), dim3(256), 0, s, a);
    EAO_HIP(hipGetLastError());
    h->clock.mark(1, s);
    return EAO_OK;
}

eao_status check_frames(const eao_yolox* h, const void* frames, int width, int height, int stride, int64_t frameStride, int batch) {
    EAO_REQUIRE(h && frames, "null argument");
    EAO_REQUIRE(batch >= 1 && batch <= h->cfg.max_batch, "batch = %d is outside 1 .. max_batch = %d", batch, h->cfg.max_batch);
    EAO_REQUIRE(width >= 1 && height >= 1 && width <= EAO_YOLOX_MAX_IMAGE && height <= EAO_YOLOX_MAX_IMAGE, "width x height = %d x %d is outside 1 .. %d", width, height,
                EAO_YOLOX_MAX_IMAGE);
    EAO_REQUIRE(stride >= 3 * width, "stride = %d is below 3 * width = %d", stride, 3 * width);
    EAO_REQUIRE(batch == 1 || frameStride >= (int64_t)stride * height, "frame_stride = %lld is below stride * height", (long long)frameStride);
    Geometry g;
    EAO_REQUIRE(geometry(width, height, h->S, &g), "a %d x %d frame has no letterbox in %d x %d (an empty resize)", width, height, h->S, h->S);
    return EAO_OK;
}

// the decode of `batch` head outputs at dProb on stream s; waits, and copies the results out unless a frame overflowed
eao_status run_decode(eao_yolox* h, const float* dProb, int batch, const int32_t* imgW, const int32_t* imgH, eao_yolox_object* objects, int32_t cap, int32_t* n,
                      int32_t* nProposals, int32_t* nTied, hipStream_t s) {
    std::vector<FrameInfo> info((size_t)batch);
    for (int f = 0; f < batch; f++) {
        Geometry g;
        EAO_REQUIRE(imgW[f] >= 1 && imgH[f] >= 1 && imgW[f] <= EAO_YOLOX_MAX_IMAGE && imgH[f] <= EAO_YOLOX_MAX_IMAGE && geometry(imgW[f], imgH[f], h->S, &g),
                    "frame %d: a %d x %d image has no letterbox in %d x %d", f, imgW[f], imgH[f], h->S, h->S);
        info[(size_t)f] = FrameInfo{g.r, imgW[f], imgH[f], 0};
    }
    const unsigned ucap = (unsigned)h->cap, ws = (unsigned)h->wstride;
    h->decoded = 0;
    eao::Drain drain(s);
    EAO_HIP(hipMemcpyAsync(h->info.p, info.data(), info.size() * sizeof(FrameInfo), hipMemcpyHostToDevice, s));
    EAO_HIP(hipMemsetAsync(h->counts.p, 0, (size_t)batch * kCounts * 4, s));
    h->clock.mark(1, s);
    hipLaunchKernelGGL(k_yolox_proposals, dim3((unsigned)eao::cdiv(h->A, 4), (unsigned)batch), dim3(256), 0, s, dProb, h->S, h->A, h->cfg.num_classes,
                       h->cfg.conf_thresh, ucap, h->counts.p, h->keys.p, h->boxes.p);
    EAO_HIP(hipGetLastError());
    h->clock.mark(2, s);
    hipLaunchKernelGGL(k_yolox_rank, dim3((unsigned)eao::cdiv(h->cap, 256), (unsigned)batch), dim3(256), 0, s, ucap, h->counts.p, h->keys.p, h->boxes.p, h->skeys.p,
                       h->sboxes.p);
    EAO_HIP(hipGetLastError());
    h->clock.mark(3, s);
    hipLaunchKernelGGL(k_yolox_mask, dim3(ws, (unsigned)batch), dim3(64), 0, s, ucap, ws, h->cfg.nms_thresh, h->counts.p, h->sboxes.p, h->mask.p);
    EAO_HIP(hipGetLastError());
    h->clock.mark(4, s);
    hipLaunchKernelGGL(k_yolox_scan, dim3((unsigned)batch), dim3(64), 0, s, ucap, ws, h->cfg.num_classes, h->counts.p, h->skeys.p, h->sboxes.p, h->mask.p, h->picked.p,
                       h->info.p, h->objs.p);
    EAO_HIP(hipGetLastError());
    h->clock.mark(5, s);
    std::vector<unsigned>& c = h->lastCounts;
    c.assign((size_t)batch * kCounts, 0u);
    EAO_HIP(hipMemcpyAsync(c.data(), h->counts.p, c.size() * 4, hipMemcpyDeviceToHost, s));
    EAO_HIP(drain.wait_more(eao::Drain::Latency));
    h->clock.collect();
    bool overflow = false, small = false;
    for (int f = 0; f < batch; f++) {
        overflow = overflow || c[(size_t)f * kCounts] > ucap;
        small = small || (int64_t)c[(size_t)f * kCounts + 1] > cap;
    }
    if (overflow) {
        drain.disarm();
        for (int f = 0; f < batch; f++) nProposals[f] = (int32_t)c[(size_t)f * kCounts];
        eao::set_error("a frame has more proposals than max_proposals = %d (n_proposals holds the counts); no object is written", h->cap);
        return EAO_ERR_CAPACITY;
    }
    h->decoded = batch;
    if (small) {
        drain.disarm();
        for (int f = 0; f < batch; f++) { nProposals[f] = (int32_t)c[(size_t)f * kCounts]; n[f] = (int32_t)c[(size_t)f * kCounts + 1]; }
        eao::set_error("a frame has more objects than cap = %d (n holds the counts); no object is written", cap);
        return EAO_ERR_CAPACITY;
    }
    for (int f = 0; f < batch; f++)
        if (c[(size_t)f * kCounts + 1])
            EAO_HIP(hipMemcpyAsync(objects + (size_t)f * cap, h->objs.p + (size_t)f * h->cap, (size_t)c[(size_t)f * kCounts + 1] * sizeof(Object), hipMemcpyDeviceToHost, s));
    EAO_HIP(drain.wait(eao::Drain::Latency));
    for (int f = 0; f < batch; f++) {
        nProposals[f] = (int32_t)c[(size_t)f * kCounts];
        n[f] = (int32_t)c[(size_t)f * kCounts + 1];
        nTied[f] = (int32_t)c[(size_t)f * kCounts + 2];
    }
    return EAO_OK;
}

eao_status check_decode(const eao_yolox* h, const void* prob, int batch, const int32_t* imgW, const int32_t* imgH, const void* objects, int32_t cap, const void* n,
                        const void* nProposals, const void* nTied) {
    EAO_REQUIRE(h && prob && imgW && imgH && objects && n && nProposals && nTied, "null argument");
    EAO_REQUIRE(batch >= 1 && batch <= h->cfg.max_batch, "batch = %d is outside 1 .. max_batch = %d", batch, h->cfg.max_batch);
    EAO_REQUIRE(cap >= 1, "cap = %d", cap);
    return EAO_OK;
}

}  // namespace

extern "C" {

void eao_yolox_cfg_default(eao_yolox_cfg* cfg) {
    if (!cfg) return;
    cfg->input_size = kInputSize;
    cfg->num_classes = kNumClasses;
    cfg->conf_thresh = kConfThresh;
    cfg->nms_thresh = kNmsThresh;
    cfg->max_proposals = EAO_YOLOX_DEFAULT_PROPOSALS;
    cfg->max_batch = 1;
}

eao_status eao_yolox_create(const eao_yolox_cfg* cfg, eao_yolox** out) {
    EAO_REQUIRE(cfg && out, "null argument");
    const eao_yolox_cfg& c = *cfg;
    EAO_REQUIRE(c.input_size >= 32 && c.input_size <= EAO_YOLOX_MAX_INPUT_SIZE && c.input_size % 32 == 0, "input_size = %d is not a multiple of 32 in 32 .. %d", c.input_size,
                EAO_YOLOX_MAX_INPUT_SIZE);
    EAO_REQUIRE(c.num_classes >= 1 && c.num_classes <= EAO_YOLOX_MAX_CLASSES, "num_classes = %d is outside 1 .. %d", c.num_classes, EAO_YOLOX_MAX_CLASSES);
    EAO_REQUIRE(c.conf_thresh >= 0.f && std::isfinite(c.conf_thresh), "conf_thresh is negative or not finite (the sort key orders positive probs)");
    EAO_REQUIRE(!std::isnan(c.nms_thresh), "nms_thresh is a NaN");
    EAO_REQUIRE(c.max_proposals >= 1 && c.max_proposals <= kMaxProposals, "max_proposals = %d is outside 1 .. %d", c.max_proposals, kMaxProposals);
    EAO_REQUIRE(c.max_batch >= 1 && c.max_batch <= EAO_YOLOX_MAX_BATCH, "max_batch = %d is outside 1 .. %d", c.max_batch, EAO_YOLOX_MAX_BATCH);
    const int wstride = eao::cdiv(c.max_proposals, 64);
    EAO_REQUIRE((int64_t)c.max_batch * c.max_proposals * wstride * 8 <= ((int64_t)1 << 31), "max_batch x max_proposals^2 / 8 exceeds 2 GiB of suppression matrix");
    eao_status st = eao::require_device();
    if (st) return st;
    eao_yolox* h = new (std::nothrow) eao_yolox;
    if (!h) { eao::set_error("out of memory"); return EAO_ERR_INTERNAL; }
    h->cfg = c; h->S = c.input_size; h->A = num_anchors(c.input_size); h->row = 5 + c.num_classes; h->cap = c.max_proposals; h->wstride = wstride;
    const size_t B = (size_t)c.max_batch, cap = (size_t)h->cap;
    auto fail = [&](eao_status s) { delete h; return s; };
    if (hipError_t e = eao::create_stream(&h->stream, eao::StreamClass::Latency); e != hipSuccess) {
        eao::set_error("hipStreamCreate failed: %s", hipGetErrorString(e));
        return fail(EAO_ERR_NO_DEVICE);
    }
    if ((st = h->lut.reserve(3 * 256)) || (st = h->taps.reserve((size_t)2 * h->S)) || (st = h->blob.reserve(B * 3 * h->S * h->S)) ||
        (st = h->prob.reserve(B * h->A * h->row)) || (st = h->counts.reserve(B * kCounts)) || (st = h->keys.reserve(B * cap)) || (st = h->skeys.reserve(B * cap)) ||
        (st = h->boxes.reserve(B * cap)) || (st = h->sboxes.reserve(B * cap)) || (st = h->mask.reserve(B * cap * wstride)) || (st = h->picked.reserve(B * cap)) ||
        (st = h->objs.reserve(B * cap)) || (st = h->info.reserve(B)))
        return fail(st);
    float table[3 * 256];
    blob_table(table);
    if (hipMemcpy(h->lut.p, table, sizeof(table), hipMemcpyHostToDevice) != hipSuccess) { eao::set_error("the table upload failed"); return fail(EAO_ERR_NO_DEVICE); }
    *out = h;
    return EAO_OK;
}

void eao_yolox_destroy(eao_yolox* h) { delete h; }

eao_status eao_yolox_preprocess(eao_yolox* h, const uint8_t* frames, int32_t width, int32_t height, int32_t stride, int64_t frame_stride, int32_t batch, int32_t rgb,
                                uint8_t* gray, int32_t gray_stride) {
    eao_status st = check_frames(h, frames, width, height, stride, frame_stride, batch);
    if (st) return st;
    EAO_REQUIRE(!gray || gray_stride >= width, "gray_stride = %d is below width = %d", gray_stride, width);
    std::lock_guard<std::mutex> lock(h->mutex);
    if (batch == 1) frame_stride = (int64_t)stride * height;
    const size_t bytes = (size_t)frame_stride * (batch - 1) + (size_t)stride * height;
    const int pitch = eao::cdiv(width, 64) * 64;
    if ((st = h->frames.reserve(bytes))) return st;
    if (gray && (st = h->gray.reserve((size_t)pitch * height * batch))) return st;
    if ((st = set_geometry(h, width, height))) return st;
    h->blobFrames = 0;
    eao::Drain drain(h->stream);
    EAO_HIP(hipMemcpyAsync(h->frames.p, frames, bytes, hipMemcpyHostToDevice, h->stream));
    if ((st = launch_pre(h, h->frames.p, width, height, stride, frame_stride, batch, rgb, h->blob.p, gray ? h->gray.p : nullptr, pitch, h->stream))) return st;
    if (gray)
        EAO_HIP(hipMemcpy2DAsync(gray, (size_t)gray_stride, h->gray.p, (size_t)pitch, (size_t)width, (size_t)height * batch, hipMemcpyDeviceToHost, h->stream));
    EAO_HIP(drain.wait(eao::Drain::Latency));
    h->clock.collect();
    h->blobFrames = batch;
    return EAO_OK;
}

eao_status eao_yolox_preprocess_device(eao_yolox* h, const uint8_t* d_frames, int32_t width, int32_t height, int32_t stride, int64_t frame_stride, int32_t batch,
                                       int32_t rgb, float* d_blob, uint8_t* d_gray, int32_t gray_stride, void* stream) {
    eao_status st = check_frames(h, d_frames, width, height, stride, frame_stride, batch);
    if (st) return st;
    EAO_REQUIRE(d_blob && ((uintptr_t)d_blob & 15) == 0, "d_blob is NULL or not 16-byte aligned");
    EAO_REQUIRE(!d_gray || (gray_stride >= width && gray_stride % 64 == 0 && ((uintptr_t)d_gray & 3) == 0), "gray_stride = %d is below width or no multiple of 64, or d_gray is not 4-byte aligned",
                gray_stride);
    std::lock_guard<std::mutex> lock(h->mutex);
    if (batch == 1) frame_stride = (int64_t)stride * height;
    if ((st = set_geometry(h, width, height))) return st;
    hipStream_t s = (hipStream_t)stream;
    if ((st = launch_pre(h, d_frames, width, height, stride, frame_stride, batch, rgb, d_blob, d_gray, gray_stride, s))) return st;
    if (h->clock.armed()) {      // (a measurement reads its events: the call waits for them)
        EAO_HIP(hipStreamSynchronize(s));
        h->clock.collect();
    }
    return EAO_OK;
}

eao_status eao_yolox_decode(eao_yolox* h, const float* prob, int32_t batch, const int32_t* img_w, const int32_t* img_h, eao_yolox_object* objects, int32_t cap,
                            int32_t* n, int32_t* n_proposals, int32_t* n_tied) {
    eao_status st = check_decode(h, prob, batch, img_w, img_h, objects, cap, n, n_proposals, n_tied);
    if (st) return st;
    std::lock_guard<std::mutex> lock(h->mutex);
    {
        eao::Drain drain(h->stream);
        EAO_HIP(hipMemcpyAsync(h->prob.p, prob, (size_t)batch * h->A * h->row * 4, hipMemcpyHostToDevice, h->stream));
        EAO_HIP(drain.wait(eao::Drain::Block));      // (the caller's array may be pageable: it is read before the call goes on)
    }
    return run_decode(h, h->prob.p, batch, img_w, img_h, objects, cap, n, n_proposals, n_tied, h->stream);
}

eao_status eao_yolox_decode_device(eao_yolox* h, const float* d_prob, int32_t batch, const int32_t* img_w, const int32_t* img_h, eao_yolox_object* objects, int32_t cap,
                                   int32_t* n, int32_t* n_proposals, int32_t* n_tied, void* stream) {
    eao_status st = check_decode(h, d_prob, batch, img_w, img_h, objects, cap, n, n_proposals, n_tied);
    if (st) return st;
    std::lock_guard<std::mutex> lock(h->mutex);
    return run_decode(h, d_prob, batch, img_w, img_h, objects, cap, n, n_proposals, n_tied, (hipStream_t)stream);
}

eao_status eao_yolox_buffers(eao_yolox* h, float** d_blob, float** d_prob, void** stream) {
    EAO_REQUIRE(h, "null argument");
    if (d_blob) *d_blob = h->blob.p;
    if (d_prob) *d_prob = h->prob.p;
    if (stream) *stream = (void*)h->stream;
    return EAO_OK;
}

eao_status eao_yolox_head(eao_yolox* h, const float* d_prob, int32_t batch, float* prob, void* stream) {
    EAO_REQUIRE(h && d_prob && prob, "null argument");
    EAO_REQUIRE(batch >= 1 && batch <= h->cfg.max_batch, "batch = %d is outside 1 .. max_batch = %d", batch, h->cfg.max_batch);
    std::lock_guard<std::mutex> lock(h->mutex);
    eao::Drain drain((hipStream_t)stream);
    EAO_HIP(hipMemcpyAsync(prob, d_prob, (size_t)batch * h->A * h->row * 4, hipMemcpyDeviceToHost, (hipStream_t)stream));
    EAO_HIP(drain.wait(eao::Drain::Block));
    return EAO_OK;
}

eao_status eao_yolox_blob(eao_yolox* h, int32_t frame, float* blob) {
    EAO_REQUIRE(h && blob, "null argument");
    std::lock_guard<std::mutex> lock(h->mutex);
    EAO_REQUIRE(frame >= 0 && frame < h->blobFrames, "frame = %d: the last eao_yolox_preprocess left %d frames", frame, h->blobFrames);
    const size_t one = (size_t)3 * h->S * h->S;
    EAO_HIP(hipMemcpy(blob, h->blob.p + (size_t)frame * one, one * 4, hipMemcpyDeviceToHost));
    return EAO_OK;
}

eao_status eao_yolox_proposals(eao_yolox* h, int32_t frame, eao_yolox_object* proposals, int32_t cap, int32_t* n) {
    EAO_REQUIRE(h && n, "null argument");
    std::lock_guard<std::mutex> lock(h->mutex);
    EAO_REQUIRE(frame >= 0 && frame < h->decoded, "frame = %d: the last decode left %d frames", frame, h->decoded);
    const int32_t cnt = (int32_t)h->lastCounts[(size_t)frame * kCounts];
    if (proposals) {
        EAO_REQUIRE(cap >= cnt, "cap = %d is below the %d proposals", cap, cnt);
        std::vector<unsigned long long> k((size_t)cnt);
        std::vector<float4> b((size_t)cnt);
        if (cnt) {
            EAO_HIP(hipMemcpy(k.data(), h->skeys.p + (size_t)frame * h->cap, (size_t)cnt * 8, hipMemcpyDeviceToHost));
            EAO_HIP(hipMemcpy(b.data(), h->sboxes.p + (size_t)frame * h->cap, (size_t)cnt * 16, hipMemcpyDeviceToHost));
        }
        for (int32_t i = 0; i < cnt; i++) {
            const uint32_t bits = ~(uint32_t)(k[(size_t)i] >> 32);
            float p;
            std::memcpy(&p, &bits, 4);
            proposals[i] = eao_yolox_object{b[(size_t)i].x, b[(size_t)i].y, b[(size_t)i].z, b[(size_t)i].w, p, (int32_t)((uint32_t)k[(size_t)i] % (uint32_t)h->cfg.num_classes)};
        }
    }
    *n = cnt;
    return EAO_OK;
}

eao_status eao_yolox_set_profiling(eao_yolox* h, int32_t on) {
    EAO_REQUIRE(h, "null argument");
    std::lock_guard<std::mutex> lock(h->mutex);
    h->clock.arm(on != 0);
    return EAO_OK;
}

eao_status eao_yolox_last_kernel_ms(eao_yolox* h, float* kernel_ms) {
    EAO_REQUIRE(h && kernel_ms, "null argument");
    std::lock_guard<std::mutex> lock(h->mutex);
    return h->clock.read(kernel_ms, "no measurement on this handle: eao_yolox_set_profiling(h, 1) and a call come first");
}

}  // extern "C"
