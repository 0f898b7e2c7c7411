// detnet_internal.h -- the detector network (the engine the reference deserialises in src/YOLOX.cc:7-48 and runs in DoInference, :331-367) as a graph of
// convolutions read from a model file, stated once for the host and, where marked, for the kernels of detnet.hip.  Plain C++17, no HIP: tools/detnet_walk.cpp
// runs it under AddressSanitizer on a machine without a GPU and is the -O3 host baseline.
//
//   the file        little-endian.  Header (40 bytes): magic "EAODNET\0", u32 version (1), u32 classes, u32 tensors, u32 ops, u64 weights_offset (a multiple of
//                   16), u64 weights_count (floats).  Then `tensors` records of 16 bytes, `ops` records of 64 bytes, and at weights_offset one block of float32.
//   tensors         {u32 channels, u32 kind, u32 a, u32 b}.  SCALED: an NHWC map of H = W = S / a (a = the downscale, a power of two up to 32; S is the
//                   handle's input size, a multiple of 32, so one file serves every S).  FIXED and FIXED_INPUT: an NHWC map of a x b pixels whatever S is (the
//                   single-op graphs of the tests); FIXED_INPUT is filled by the caller (eao_detnet_set_tensor) and counts as written.  BLOB: the 3 x S x S CHW
//                   input of DoInference, tensor 0 and only there.  HEAD: the output, anchors x (5 + classes) floats, strides 8, 16 and 32 in that order,
//                   row-major inside a level -- what GenerateYoloxProposals reads (src/YOLOX.cc:64-77, :166-209); at most one.
//   ops             read a channel range of a tensor and write a channel range of a tensor, so a concatenation costs nothing.
//                   FOCUS      the blob -> 12 channels at half size, YOLOX's order: top-left, bottom-left, top-right, bottom-right, three channels each
//                   CONV       k in {1, 3}, stride in {1, 2}, pad (k - 1) / 2, a bias always (batch norm is folded by the exporter), activation none / SiLU /
//                              sigmoid, an optional residual range added after the activation; weights [Cout][ky][kx][Cin].  Into the HEAD: the level is the one
//                              whose map the source has.
//                   MAXPOOL    odd k <= 13, stride 1, pad k / 2
//                   UPSAMPLE2  nearest neighbour
//   the loader      checks, before anything is computed: sizes and offsets inside the file, channel ranges inside their tensors, every range written before it
//                   is read, no channel written twice, the head covered exactly once, shapes consistent under the strides; grouped and depthwise convolutions
//                   (YOLOX-nano, YOLOX-tiny) are refused by name.
//   the arithmetic  conv       acc = bias; over the taps in the order ky, kx, ci ascending acc = fmaf(x, w, acc); a position outside the map reads +0.0f.  One
//                              accumulator per output element: no split of K, no atomics.  (+0.0f is not neutral: fmaf(0, 0, -0.0f) is +0.0f.  A kernel that pads
//                              K therefore pads with the product (+0.0f) * (-0.0f) = -0.0f, which is.)
//                   sigmoid    1.0f / (1.0f + yolox_exp_f32(-x)) in float operations; SiLU x * sigmoid(x); the residual one float add behind the activation
//                   maxpool    the maximum under the order -0 < +0; any NaN in the window gives 0x7fc00000; the padding is -inf.  Independent of the scan order, so
//                              9 x 9 and 13 x 13 may be repeated 5 x 5.
#pragma once

#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "yolox_internal.h"

namespace eao {
namespace detnet {

using eao::yolox::yolox_exp_f32;

constexpr char kMagic[8] = {'E', 'A', 'O', 'D', 'N', 'E', 'T', '\0'};
constexpr uint32_t kVersion = 1;
constexpr size_t kHeaderBytes = 40, kTensorBytes = 16, kOpBytes = 64;
constexpr uint32_t kMaxTensors = 4096, kMaxOps = 4096, kMaxChannels = 65536, kMaxClasses = 1024, kMaxFixed = 4096;
constexpr int kMaxInput = 2048;      // EAO_YOLOX_MAX_INPUT_SIZE

enum TensorKind : uint32_t { SCALED = 0, FIXED = 1, BLOB = 2, HEAD = 3, FIXED_INPUT = 4 };
enum OpKind : uint32_t { FOCUS = 0, CONV = 1, MAXPOOL = 2, UPSAMPLE2 = 3 };
enum Act : uint32_t { ACT_NONE = 0, ACT_SILU = 1, ACT_SIGMOID = 2 };

struct TensorRec { uint32_t channels, kind, a, b; };
struct OpRec {
    uint32_t kind, src, src_c0, src_c, dst, dst_c0, dst_c, k, stride, act, groups;
    int32_t res;
    uint32_t res_c0, w_off, b_off, reserved;
};
static_assert(sizeof(TensorRec) == kTensorBytes && sizeof(OpRec) == kOpBytes, "the records of the file");

struct Tensor { int C = 0, H = 0, W = 0; uint32_t kind = SCALED; size_t offset = 0; };      // offset: floats into the activation block (frame 0)
struct Op {
    OpRec r;
    int level = -1;            // into the HEAD: 0, 1, 2
    int anchor0 = 0;           // ... and the first anchor of that level
    double flops = 0;          // of one frame
};
struct Net {
    int S = 0, classes = 0, row = 0, anchors = 0, head = -1;
    std::vector<Tensor> tensors;
    std::vector<Op> ops;
    const float* weights = nullptr;      // into the caller's file, or into `own`
    size_t weightCount = 0;
    std::vector<float> own;
    size_t actFloats = 0;                // of one frame: the tensors' maps one after the other, each from a multiple of 64 floats
    double flops = 0;
};

// ---------------------------------------------------------------- the arithmetic
EAO_YOLOX_HD inline float sigmoid_f32(float x) { return 1.0f / (1.0f + yolox_exp_f32(-x)); }
EAO_YOLOX_HD inline float activate(float v, uint32_t act) {
    if (act == ACT_SILU) return v * sigmoid_f32(v);
    if (act == ACT_SIGMOID) return sigmoid_f32(v);
    return v;
}
// the order of maxpool: NaN above everything (and canonical), -0 below +0
EAO_YOLOX_HD inline uint32_t f32_bits(float f) { uint32_t b; __builtin_memcpy(&b, &f, 4); return b; }
EAO_YOLOX_HD inline float bits_f32(uint32_t b) { float f; __builtin_memcpy(&f, &b, 4); return f; }
EAO_YOLOX_HD inline float pool_max(float a, float b) {
    if (a != a || b != b) return bits_f32(0x7fc00000u);
    if (a == b) return (f32_bits(a) >> 31) ? b : a;      // +-0: the one without a sign where there is one
    return a < b ? b : a;
}
constexpr uint32_t kNegInfBits = 0xff800000u;

// ---------------------------------------------------------------- the tile form of a convolution (which instantiation of k_detnet_conv launch_op takes)
// All three give the same bits; the rule is stated here so that the host (tools/detnet_walk.cpp `forms`) can say which kernel a test ran.
enum ConvForm : int { FORM_16x16x4_ONE = 0, FORM_16x16x4_TWO = 1, FORM_32x32x2 = 2 };      // 64 x 16, 64 x 32 and 128 x 64 outputs per block
constexpr int kFillBlocks = 256;      // a 32 x 32 x 2 grid below one block per compute unit leaves units idle: the 16 x 16 x 4 tiles are a quarter of the size
inline const char* conv_form_name(ConvForm f) { return f == FORM_32x32x2 ? "32x32x2" : f == FORM_16x16x4_TWO ? "16x16x4x2" : "16x16x4x1"; }
// M: the output pixels over the batch
inline ConvForm conv_form(long long M, int Cout) {
    if (Cout <= 16) return FORM_16x16x4_ONE;
    if (((M + 127) / 128) * ((Cout + 63) / 64) >= kFillBlocks) return FORM_32x32x2;
    return FORM_16x16x4_TWO;
}

// ---------------------------------------------------------------- the loader
struct Fail {
    std::string msg;
    bool operator()(const char* fmt, ...) __attribute__((format(printf, 2, 3))) {
        char buf[320];
        va_list ap;
        va_start(ap, fmt);
        std::vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        msg = buf;
        return false;
    }
};

inline int level_of(int S, int H, int W) {
    for (int l = 0; l < 3; l++)
        if (H == S / (8 << l) && W == H) return l;
    return -1;
}

// parses and checks `bytes` bytes at `file` for an input of S x S; copy: keep the weights in net->own (the file may go away).  false: *why says what is wrong.
inline bool load(const void* file, uint64_t bytes, int S, bool copy, Net* net, std::string* why) {
    Fail fail;
    auto bad = [&]() { *why = fail.msg; return false; };
    const unsigned char* f = (const unsigned char*)file;
    if (!f) { fail("the model is NULL"); return bad(); }
    if (S < 32 || S > kMaxInput || S % 32) { fail("input_size = %d is not a multiple of 32 in 32 .. %d", S, kMaxInput); return bad(); }
    if (bytes < kHeaderBytes) { fail("the file has %llu bytes, the header has %zu (truncated)", (unsigned long long)bytes, kHeaderBytes); return bad(); }
    if (std::memcmp(f, kMagic, 8) != 0) { fail("the magic is not EAODNET"); return bad(); }
    uint32_t h32[4];
    uint64_t h64[2];
    std::memcpy(h32, f + 8, 16);
    std::memcpy(h64, f + 24, 16);
    const uint32_t version = h32[0], classes = h32[1], nT = h32[2], nO = h32[3];
    const uint64_t wOff = h64[0], wCount = h64[1];
    if (version != kVersion) { fail("version %u, this library reads %u", version, kVersion); return bad(); }
    if (classes < 1 || classes > kMaxClasses) { fail("classes = %u is outside 1 .. %u", classes, kMaxClasses); return bad(); }
    if (nT < 2 || nT > kMaxTensors || nO < 1 || nO > kMaxOps) { fail("%u tensors and %u ops are outside 2 .. %u and 1 .. %u", nT, nO, kMaxTensors, kMaxOps); return bad(); }
    const uint64_t tablesEnd = kHeaderBytes + (uint64_t)nT * kTensorBytes + (uint64_t)nO * kOpBytes;
    if (tablesEnd > bytes) { fail("the tables end at byte %llu of %llu (truncated)", (unsigned long long)tablesEnd, (unsigned long long)bytes); return bad(); }
    if (wOff % 16 || wOff < tablesEnd || wOff > bytes || wCount > (bytes - wOff) / 4) {
        fail("the weights (offset %llu, %llu floats) are misaligned, overlap the tables or pass the end of the %llu bytes", (unsigned long long)wOff,
             (unsigned long long)wCount, (unsigned long long)bytes);
        return bad();
    }
    net->S = S; net->classes = (int)classes; net->row = 5 + (int)classes; net->anchors = 0; net->head = -1;
    net->tensors.assign(nT, Tensor{});
    net->ops.assign(nO, Op{});
    net->flops = 0;
    // tensors
    size_t act = 0;
    for (uint32_t t = 0; t < nT; t++) {
        TensorRec r;
        std::memcpy(&r, f + kHeaderBytes + (size_t)t * kTensorBytes, kTensorBytes);
        Tensor& T = net->tensors[t];
        T.kind = r.kind;
        if (r.channels < 1 || r.channels > kMaxChannels) { fail("tensor %u: %u channels are outside 1 .. %u", t, r.channels, kMaxChannels); return bad(); }
        T.C = (int)r.channels;
        if ((r.kind == BLOB) != (t == 0)) { fail("tensor %u: the blob is tensor 0 and only tensor 0", t); return bad(); }
        switch (r.kind) {
        case BLOB:
            if (r.channels != 3) { fail("tensor 0: the blob has 3 channels, not %u", r.channels); return bad(); }
            T.H = T.W = S;
            break;
        case SCALED:
            if (r.a < 1 || r.a > 32 || (r.a & (r.a - 1)) || r.b != 0) { fail("tensor %u: downscale %u is no power of two up to 32", t, r.a); return bad(); }
            T.H = T.W = S / (int)r.a;
            break;
        case FIXED: case FIXED_INPUT:
            if (r.a < 1 || r.a > kMaxFixed || r.b < 1 || r.b > kMaxFixed) { fail("tensor %u: a map of %u x %u is outside 1 .. %u", t, r.a, r.b, kMaxFixed); return bad(); }
            T.H = (int)r.a; T.W = (int)r.b;
            break;
        case HEAD:
            if (net->head >= 0) { fail("tensor %u: a second head (tensor %d is one)", t, net->head); return bad(); }
            if (r.channels != 5 + classes) { fail("tensor %u: the head has %u channels, 5 + classes = %u", t, r.channels, 5 + classes); return bad(); }
            net->head = (int)t;
            net->anchors = eao::yolox::num_anchors(S);
            break;
        default:
            fail("tensor %u: kind %u", t, r.kind);
            return bad();
        }
        if (r.kind == SCALED || r.kind == FIXED || r.kind == FIXED_INPUT) {
            T.offset = act;
            act += ((size_t)T.H * T.W * T.C + 63) & ~(size_t)63;
        }
    }
    net->actFloats = act;
    // ops: written[t][level * C + c] for the head, [c] elsewhere
    std::vector<std::vector<uint8_t>> written(nT);
    for (uint32_t t = 0; t < nT; t++) {
        const Tensor& T = net->tensors[t];
        written[t].assign((size_t)T.C * (T.kind == HEAD ? 3 : 1), (T.kind == BLOB || T.kind == FIXED_INPUT) ? 1 : 0);
    }
    auto inside = [&](uint32_t t, uint32_t c0, uint32_t c) { return t < nT && c >= 1 && c0 <= (uint32_t)net->tensors[t].C && c <= (uint32_t)net->tensors[t].C - c0; };
    for (uint32_t i = 0; i < nO; i++) {
        Op& op = net->ops[i];
        OpRec& r = op.r;
        std::memcpy(&r, f + kHeaderBytes + (size_t)nT * kTensorBytes + (size_t)i * kOpBytes, kOpBytes);
        if (r.kind > UPSAMPLE2) { fail("op %u: kind %u", i, r.kind); return bad(); }
        if (!inside(r.src, r.src_c0, r.src_c)) { fail("op %u: the source channels %u + %u lie outside tensor %u", i, r.src_c0, r.src_c, r.src); return bad(); }
        if (!inside(r.dst, r.dst_c0, r.dst_c)) { fail("op %u: the destination channels %u + %u lie outside tensor %u", i, r.dst_c0, r.dst_c, r.dst); return bad(); }
        const Tensor &Ts = net->tensors[r.src], &Td = net->tensors[r.dst];
        if (Td.kind == BLOB || Td.kind == FIXED_INPUT) { fail("op %u: writes an input (tensor %u)", i, r.dst); return bad(); }
        if (Ts.kind == HEAD) { fail("op %u: reads the head", i); return bad(); }
        if ((Ts.kind == BLOB) != (r.kind == FOCUS)) { fail("op %u: the blob is read by FOCUS and FOCUS reads the blob", i); return bad(); }
        if (Td.kind == HEAD && r.kind != CONV) { fail("op %u: only a convolution writes the head", i); return bad(); }
        int Ho = 0, Wo = 0;
        switch (r.kind) {
        case FOCUS:
            if (r.src_c0 != 0 || r.src_c != 3 || r.dst_c != 12) { fail("op %u: FOCUS reads 3 channels and writes 12", i); return bad(); }
            Ho = Ts.H / 2; Wo = Ts.W / 2;
            break;
        case CONV: {
            if (r.groups != 1) { fail("op %u: a grouped or depthwise convolution (groups = %u; YOLOX-nano and YOLOX-tiny) is not supported", i, r.groups); return bad(); }
            if ((r.k != 1 && r.k != 3) || (r.stride != 1 && r.stride != 2) || r.act > ACT_SIGMOID) {
                fail("op %u: k = %u, stride = %u, activation %u are outside {1, 3}, {1, 2}, 0 .. 2", i, r.k, r.stride, r.act);
                return bad();
            }
            const int p = ((int)r.k - 1) / 2;
            Ho = (Ts.H + 2 * p - (int)r.k) / (int)r.stride + 1;
            Wo = (Ts.W + 2 * p - (int)r.k) / (int)r.stride + 1;
            const uint64_t nW = (uint64_t)r.dst_c * r.k * r.k * r.src_c;
            if (r.w_off > wCount || nW > wCount - r.w_off || r.b_off > wCount || r.dst_c > wCount - r.b_off) {
                fail("op %u: its weights (%u + %llu) or its bias (%u + %u) pass the end of the %llu floats", i, r.w_off, (unsigned long long)nW, r.b_off, r.dst_c,
                     (unsigned long long)wCount);
                return bad();
            }
            op.flops = 2.0 * (double)nW * Ho * Wo;
            break;
        }
        case MAXPOOL:
            if (r.k < 1 || r.k > 13 || !(r.k & 1) || r.src_c != r.dst_c) { fail("op %u: MAXPOOL with k = %u (odd, up to 13) over %u -> %u channels", i, r.k, r.src_c, r.dst_c); return bad(); }
            Ho = Ts.H; Wo = Ts.W;
            break;
        case UPSAMPLE2:
            if (r.src_c != r.dst_c) { fail("op %u: UPSAMPLE2 over %u -> %u channels", i, r.src_c, r.dst_c); return bad(); }
            Ho = 2 * Ts.H; Wo = 2 * Ts.W;
            break;
        }
        size_t wbase = 0;
        if (Td.kind == HEAD) {
            if (r.stride != 1 || (op.level = level_of(S, Ts.H, Ts.W)) < 0) { fail("op %u: a %d x %d map at stride %u is no level of the head", i, Ts.H, Ts.W, r.stride); return bad(); }
            op.anchor0 = 0;
            for (int l = 0; l < op.level; l++) op.anchor0 += (S / (8 << l)) * (S / (8 << l));
            wbase = (size_t)op.level * Td.C;
        } else if (Ho != Td.H || Wo != Td.W) {
            fail("op %u: it makes a %d x %d map and tensor %u is %d x %d", i, Ho, Wo, r.dst, Td.H, Td.W);
            return bad();
        }
        for (uint32_t c = 0; c < r.src_c; c++)
            if (!written[r.src][r.src_c0 + c]) { fail("op %u: reads channel %u of tensor %u before it is written", i, r.src_c0 + c, r.src); return bad(); }
        if (r.kind == CONV && r.res >= 0) {
            if (!inside((uint32_t)r.res, r.res_c0, r.dst_c)) { fail("op %u: the residual channels %u + %u lie outside tensor %d", i, r.res_c0, r.dst_c, r.res); return bad(); }
            const Tensor& Tr = net->tensors[(size_t)r.res];
            if (Tr.kind == BLOB || Tr.kind == HEAD || Tr.H != Ho || Tr.W != Wo) { fail("op %u: the residual tensor %d has another shape", i, r.res); return bad(); }
            for (uint32_t c = 0; c < r.dst_c; c++)
                if (!written[(size_t)r.res][r.res_c0 + c]) { fail("op %u: reads channel %u of tensor %d before it is written", i, r.res_c0 + c, r.res); return bad(); }
        } else if (r.kind != CONV || r.res < -1) {
            r.res = -1;
        }
        for (uint32_t c = 0; c < r.dst_c; c++) {
            uint8_t& w = written[r.dst][wbase + r.dst_c0 + c];
            if (w) { fail("op %u: writes channel %u of tensor %u a second time", i, r.dst_c0 + c, r.dst); return bad(); }
            w = 1;
        }
        net->flops += op.flops;
    }
    if (net->head >= 0)
        for (size_t k = 0; k < written[(size_t)net->head].size(); k++)
            if (!written[(size_t)net->head][k]) {
                fail("the head is not covered: level %zu, channel %zu is never written", k / (size_t)net->row, k % (size_t)net->row);
                return bad();
            }
    const float* w = (const float*)(f + wOff);
    net->weightCount = (size_t)wCount;
    if (copy) {
        net->own.resize((size_t)wCount);
        if (wCount) std::memcpy(net->own.data(), w, (size_t)wCount * 4);
        net->weights = net->own.data();
    } else {
        if ((uintptr_t)w & 3) { fail("the model is not 4-byte aligned in memory"); return bad(); }
        net->weights = w;
    }
    return true;
}

// ---------------------------------------------------------------- the walk: one frame on the host
// act: actFloats floats (FIXED_INPUT tensors filled by the caller); prob: anchors x row floats (may be null without a head)
inline void forward_host(const Net& net, const float* blob, float* act, float* prob) {
    for (const Op& op : net.ops) {
        const OpRec& r = op.r;
        const Tensor &Ts = net.tensors[r.src], &Td = net.tensors[r.dst];
        const float* src = Ts.kind == BLOB ? blob : act + Ts.offset;
        const bool head = Td.kind == HEAD;
        float* dst = head ? prob + (size_t)op.anchor0 * net.row : act + Td.offset;
        const int Cs = Ts.C, Cd = Td.C;
        const int Ho = head ? Ts.H : Td.H, Wo = head ? Ts.W : Td.W;
        switch (r.kind) {
        case FOCUS:
            for (int y = 0; y < Ho; y++)
                for (int x = 0; x < Wo; x++)
                    for (int c = 0; c < 12; c++) {
                        const int q = c / 3, ch = c % 3, dy = q & 1, dx = q >> 1;      // top-left, bottom-left, top-right, bottom-right
                        dst[((size_t)y * Wo + x) * Cd + r.dst_c0 + c] = src[((size_t)ch * Ts.H + 2 * y + dy) * Ts.W + 2 * x + dx];
                    }
            break;
        case CONV: {
            const int k = (int)r.k, s = (int)r.stride, p = (k - 1) / 2, Ci = (int)r.src_c, Co = (int)r.dst_c;
            const size_t K = (size_t)k * k * Ci;
            const float *W = net.weights + r.w_off, *B = net.weights + r.b_off;
            const float* res = r.res >= 0 ? act + net.tensors[(size_t)r.res].offset : nullptr;
            const int Cr = r.res >= 0 ? net.tensors[(size_t)r.res].C : 0;
            std::vector<float> patch(K);
            for (int y = 0; y < Ho; y++)
                for (int x = 0; x < Wo; x++) {
                    for (int ky = 0; ky < k; ky++)
                        for (int kx = 0; kx < k; kx++) {
                            const int iy = y * s - p + ky, ix = x * s - p + kx;
                            float* pp = patch.data() + ((size_t)ky * k + kx) * Ci;
                            if (iy < 0 || iy >= Ts.H || ix < 0 || ix >= Ts.W) for (int c = 0; c < Ci; c++) pp[c] = 0.0f;
                            else std::memcpy(pp, src + ((size_t)iy * Ts.W + ix) * Cs + r.src_c0, (size_t)Ci * 4);
                        }
                    const size_t pix = (size_t)y * Wo + x;
                    int co = 0;
                    for (; co + 8 <= Co; co += 8) {      // eight chains side by side: each one is still a single accumulator in k order
                        float a[8];
                        for (int j = 0; j < 8; j++) a[j] = B[co + j];
                        for (size_t kk = 0; kk < K; kk++)
                            for (int j = 0; j < 8; j++) a[j] = std::fmaf(patch[kk], W[(size_t)(co + j) * K + kk], a[j]);
                        for (int j = 0; j < 8; j++) {
                            float v = activate(a[j], r.act);
                            if (res) v = v + res[pix * Cr + r.res_c0 + co + j];
                            dst[pix * Cd + r.dst_c0 + co + j] = v;
                        }
                    }
                    for (; co < Co; co++) {
                        float a = B[co];
                        for (size_t kk = 0; kk < K; kk++) a = std::fmaf(patch[kk], W[(size_t)co * K + kk], a);
                        float v = activate(a, r.act);
                        if (res) v = v + res[pix * Cr + r.res_c0 + co];
                        dst[pix * Cd + r.dst_c0 + co] = v;
                    }
                }
            break;
        }
        case MAXPOOL: {
            const int p = (int)r.k / 2;
            for (int y = 0; y < Ho; y++)
                for (int x = 0; x < Wo; x++)
                    for (int c = 0; c < (int)r.src_c; c++) {
                        float m = bits_f32(kNegInfBits);
                        for (int iy = y - p; iy <= y + p; iy++)
                            for (int ix = x - p; ix <= x + p; ix++)
                                if (iy >= 0 && iy < Ts.H && ix >= 0 && ix < Ts.W) m = pool_max(m, src[((size_t)iy * Ts.W + ix) * Cs + r.src_c0 + c]);
                        dst[((size_t)y * Wo + x) * Cd + r.dst_c0 + c] = m;
                    }
            break;
        }
        case UPSAMPLE2:
            for (int y = 0; y < Ho; y++)
                for (int x = 0; x < Wo; x++)
                    for (int c = 0; c < (int)r.src_c; c++)
                        dst[((size_t)y * Wo + x) * Cd + r.dst_c0 + c] = src[((size_t)(y / 2) * Ts.W + x / 2) * Cs + r.src_c0 + c];
            break;
        }
    }
}

}  // namespace detnet
}  // namespace eao
