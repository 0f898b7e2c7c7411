// detnet.hip -- the detector network on the device: what the reference hands to a TensorRT engine (src/YOLOX.cc:7-48 the deserialisation, :331-367 DoInference)
// as a sequence of launches over a graph read from a model file.  The file, its checks and the arithmetic are stated once in csrc/detnet_internal.h.
//
//   k_detnet_conv<T, NT>  an implicit GEMM on the f32-input MFMA: M = the output pixels over the batch, N = Cout, K = k * k * Cin in the order ky, kx, ci (NHWC keeps
//                         ci contiguous).  T = 32 is v_mfma_f32_32x32x2_f32, T = 16 is v_mfma_f32_16x16x4_f32; lane l holds A[l % T][l / T] and B[l / T][l % T].
//                         A block of four waves makes (4 T) x (NT T) outputs: wave w the rows w T .. w T + T - 1, NT accumulator tiles side by side.  K goes through
//                         LDS in stages of 64 or 128, both operands k-major with an odd row pitch.  The accumulator starts as the bias and one accumulator carries the
//                         whole chain of an output element, so the result is the fmaf chain of detnet_internal.h bit for bit.  Behind K (and only there) A is padded
//                         with +0.0f and B with -0.0f: their product -0.0f changes no accumulator, not even -0.0f.  Bias, activation, residual and the strided
//                         store are the epilogue.  Which form an op takes is conv_form() of detnet_internal.h.
//   k_detnet_focus, k_detnet_maxpool, k_detnet_upsample2   one lane per output element.
// A forward pass is a sequence of launches on the caller's stream: no capture, no stream of its own, no host hop.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <mutex>
#include <new>
#include <vector>

#include "common.h"
#include "detnet_internal.h"

namespace {

using namespace eao::detnet;

static_assert(kMaxInput == EAO_YOLOX_MAX_INPUT_SIZE && kMaxClasses == EAO_YOLOX_MAX_CLASSES, "include/eao_fusion.h and detnet_internal.h agree");

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

struct ConvArgs {
    const float* src; const float* w; const float* bias; const float* res; float* dst;
    long long srcFrame, dstFrame, resFrame;      // floats between the frames of a batch
    int srcC, srcC0, dstC, dstC0, resC, resC0;
    int Hi, Wi, Ho, Wo, Ci, Co, k, stride, act, M, K;
};

template <int T> struct Mfma;
template <> struct Mfma<32> {
    typedef f32x16 Acc;
    static constexpr int kRegs = 16;
    static __device__ __forceinline__ Acc run(float a, float b, Acc c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ int row(int reg, int lane) { return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5); }
};
template <> struct Mfma<16> {
    typedef f32x4 Acc;
    static constexpr int kRegs = 4;
    static __device__ __forceinline__ Acc run(float a, float b, Acc c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ int row(int reg, int lane) { return 4 * (lane >> 4) + reg; }
};

// K per LDS stage.  A stage costs one round trip to memory whatever its depth (all of a lane's loads are issued before the first is used), and the chain of a
// deep layer is a sequence of such round trips: the small-tile forms, which the deep layers take, stage 128 deep, the large one 64.
template <int T> struct Stage { static constexpr int kDepth = T == 16 ? 128 : 64; };

template <int T, int NT>
__global__ __launch_bounds__(256) void k_detnet_conv(ConvArgs A) {
    typedef Mfma<T> MF;
    constexpr int BM = 4 * T, BN = NT * T, KS = 64 / T, KC = Stage<T>::kDepth, RS = 256 / KC, NA = BM / RS, NB = BN / RS;
    __shared__ float As[KC][BM + 1];
    __shared__ float Bs[KC][BN + 1];
    __shared__ int rowY[BM], rowX[BM], rowN[BM];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
    const int HoWo = A.Ho * A.Wo, pad = (A.k - 1) >> 1;
    for (int r = tid; r < BM; r += 256) {
        const int m = m0 + r;
        if (m < A.M) {
            const int n = m / HoWo, p = m - n * HoWo, oy = p / A.Wo, ox = p - oy * A.Wo;
            rowN[r] = n; rowY[r] = oy * A.stride - pad; rowX[r] = ox * A.stride - pad;
        } else {
            rowN[r] = 0; rowY[r] = -(1 << 20); rowX[r] = -(1 << 20);      // (every tap outside the map)
        }
    }
    const int lr = lane % T, lk = lane / T;
    typename MF::Acc acc[NT];
#pragma unroll
    for (int t = 0; t < NT; t++) {
        const int col = n0 + t * T + lr;
        const float b = col < A.Co ? A.bias[col] : 0.f;
#pragma unroll
        for (int r = 0; r < MF::kRegs; r++) acc[t][r] = b;
    }
    __syncthreads();
    const int kk = tid & (KC - 1), r0 = tid / KC;
    for (int k0 = 0; k0 < A.K; k0 += KC) {
        const int left = A.K - k0;
        const int kEnd = left >= KC ? KC : ((left + KS - 1) / KS) * KS;      // the stage's depth: the last one ends at K rounded up to the instruction's
        if (kk < kEnd) {
            const int k = k0 + kk;
            const bool kIn = k < A.K;
            const int tap = k / A.Ci, ci = k - tap * A.Ci;
            const int ky = A.k == 3 ? tap / 3 : 0, kx = tap - ky * A.k;
            float va[NA], vb[NB];
#pragma unroll
            for (int i = 0; i < NA; i++) {
                const int r = r0 + RS * i;
                const int iy = rowY[r] + ky, ix = rowX[r] + kx;
                va[i] = 0.0f;
                if (kIn && iy >= 0 && iy < A.Hi && ix >= 0 && ix < A.Wi) va[i] = A.src[(long long)rowN[r] * A.srcFrame + ((long long)iy * A.Wi + ix) * A.srcC + A.srcC0 + ci];
            }
#pragma unroll
            for (int i = 0; i < NB; i++) {
                const int col = n0 + r0 + RS * i;
                vb[i] = -0.0f;      // behind K: (+0.0f) * (-0.0f) leaves every accumulator as it is
                if (kIn && col < A.Co) vb[i] = A.w[(long long)col * A.K + k];
            }
#pragma unroll
            for (int i = 0; i < NA; i++) As[kk][r0 + RS * i] = va[i];
#pragma unroll
            for (int i = 0; i < NB; i++) Bs[kk][r0 + RS * i] = vb[i];
        }
        __syncthreads();
        for (int s = 0; s < kEnd; s += KS) {
            const float a = As[s + lk][wave * T + lr];
#pragma unroll
            for (int t = 0; t < NT; t++) acc[t] = MF::run(a, Bs[s + lk][t * T + lr], acc[t]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int t = 0; t < NT; t++) {
        const int col = n0 + t * T + lr;
#pragma unroll
        for (int r = 0; r < MF::kRegs; r++) {
            const int m = m0 + wave * T + MF::row(r, lane);
            if (m < A.M && col < A.Co) {
                const int n = m / HoWo, p = m - n * HoWo;
                float v = activate(acc[t][r], (uint32_t)A.act);
                if (A.res) v = v + A.res[(long long)n * A.resFrame + (long long)p * A.resC + A.resC0 + col];
                A.dst[(long long)n * A.dstFrame + (long long)p * A.dstC + A.dstC0 + col] = v;
            }
        }
    }
}

struct MapArgs {
    const float* src; float* dst;
    long long srcFrame, dstFrame;
    int srcC, srcC0, dstC, dstC0, C, Hi, Wi, Ho, Wo, k;
    long long total;      // batch * Ho * Wo * C
};

__device__ __forceinline__ bool map_item(const MapArgs& A, int* n, int* y, int* x, int* c) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.total) return false;
    *c = (int)(i % A.C);
    long long p = i / A.C;
    *x = (int)(p % A.Wo); p /= A.Wo;
    *y = (int)(p % A.Ho);
    *n = (int)(p / A.Ho);
    return true;
}

// the blob is CHW (3 x S x S); the 12 channels are top-left, bottom-left, top-right, bottom-right, three each
__global__ __launch_bounds__(256) void k_detnet_focus(MapArgs A) {
    int n, y, x, c;
    if (!map_item(A, &n, &y, &x, &c)) return;
    const int q = c / 3, ch = c - 3 * q, dy = q & 1, dx = q >> 1;
    A.dst[n * A.dstFrame + ((long long)y * A.Wo + x) * A.dstC + A.dstC0 + c] = A.src[n * A.srcFrame + ((long long)ch * A.Hi + 2 * y + dy) * A.Wi + 2 * x + dx];
}

__global__ __launch_bounds__(256) void k_detnet_maxpool(MapArgs A) {
    int n, y, x, c;
    if (!map_item(A, &n, &y, &x, &c)) return;
    const int p = A.k >> 1;
    const float* s = A.src + n * A.srcFrame + A.srcC0 + c;
    float m = bits_f32(kNegInfBits);
    for (int iy = max(y - p, 0); iy <= min(y + p, A.Hi - 1); iy++)
        for (int ix = max(x - p, 0); ix <= min(x + p, A.Wi - 1); ix++) m = pool_max(m, s[((long long)iy * A.Wi + ix) * A.srcC]);
    A.dst[n * A.dstFrame + ((long long)y * A.Wo + x) * A.dstC + A.dstC0 + c] = m;
}

__global__ __launch_bounds__(256) void k_detnet_upsample2(MapArgs A) {
    int n, y, x, c;
    if (!map_item(A, &n, &y, &x, &c)) return;
    A.dst[n * A.dstFrame + ((long long)y * A.Wo + x) * A.dstC + A.dstC0 + c] = A.src[n * A.srcFrame + ((long long)(y >> 1) * A.Wi + (x >> 1)) * A.srcC + A.srcC0 + c];
}

}  // namespace

struct eao_detnet {
    Net net;
    int maxBatch = 0;
    eao::DevBuf<float> weights, act;
    std::mutex mutex;
    bool profiling = false;
    std::vector<hipEvent_t> ev;      // ops + 1
    std::vector<float> ms;           // per op, -1: not measured
    ~eao_detnet() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
};

namespace {

eao_status launch_op(eao_detnet* h, const Op& op, const float* dBlob, float* dProb, int batch, hipStream_t s) {
    const Net& net = h->net;
    const OpRec& r = op.r;
    const Tensor &Ts = net.tensors[r.src], &Td = net.tensors[r.dst];
    const bool head = Td.kind == HEAD;
    const long long actFrame = (long long)net.actFloats;
    const float* src = Ts.kind == BLOB ? dBlob : h->act.p + Ts.offset;
    const long long srcFrame = Ts.kind == BLOB ? 3ll * net.S * net.S : actFrame;
    float* dst = head ? dProb + (size_t)op.anchor0 * net.row : h->act.p + Td.offset;
    const long long dstFrame = head ? (long long)net.anchors * net.row : actFrame;
    const int Ho = head ? Ts.H : Td.H, Wo = head ? Ts.W : Td.W;
    if (r.kind == CONV) {
        ConvArgs A;
        A.src = src; A.w = h->weights.p + r.w_off; A.bias = h->weights.p + r.b_off; A.dst = dst;
        A.res = r.res >= 0 ? h->act.p + net.tensors[(size_t)r.res].offset : nullptr;
        A.srcFrame = srcFrame; A.dstFrame = dstFrame; A.resFrame = actFrame;
        A.srcC = Ts.C; A.srcC0 = (int)r.src_c0; A.dstC = Td.C; A.dstC0 = (int)r.dst_c0;
        A.resC = r.res >= 0 ? net.tensors[(size_t)r.res].C : 0; A.resC0 = (int)r.res_c0;
        A.Hi = Ts.H; A.Wi = Ts.W; A.Ho = Ho; A.Wo = Wo; A.Ci = (int)r.src_c; A.Co = (int)r.dst_c; A.k = (int)r.k; A.stride = (int)r.stride; A.act = (int)r.act;
        A.M = batch * Ho * Wo; A.K = (int)(r.k * r.k * r.src_c);
        switch (conv_form(A.M, A.Co)) {
        case FORM_16x16x4_ONE:
            hipLaunchKernelGGL((k_detnet_conv<16, 1>), dim3((unsigned)eao::cdiv(A.M, 64), 1), dim3(256), 0, s, A);
            break;
        case FORM_32x32x2:
            hipLaunchKernelGGL((k_detnet_conv<32, 2>), dim3((unsigned)eao::cdiv(A.M, 128), (unsigned)eao::cdiv(A.Co, 64)), dim3(256), 0, s, A);
            break;
        case FORM_16x16x4_TWO:
            hipLaunchKernelGGL((k_detnet_conv<16, 2>), dim3((unsigned)eao::cdiv(A.M, 64), (unsigned)eao::cdiv(A.Co, 32)), dim3(256), 0, s, A);
            break;
        }
    } else {
        MapArgs A;
        A.src = src; A.dst = dst; A.srcFrame = srcFrame; A.dstFrame = dstFrame;
        A.srcC = Ts.C; A.srcC0 = (int)r.src_c0; A.dstC = Td.C; A.dstC0 = (int)r.dst_c0; A.C = (int)r.dst_c;
        A.Hi = Ts.H; A.Wi = Ts.W; A.Ho = Ho; A.Wo = Wo; A.k = (int)r.k;
        A.total = (long long)batch * Ho * Wo * A.C;
        const dim3 grid((unsigned)((A.total + 255) / 256));
        if (r.kind == FOCUS) hipLaunchKernelGGL(k_detnet_focus, grid, dim3(256), 0, s, A);
        else if (r.kind == MAXPOOL) hipLaunchKernelGGL(k_detnet_maxpool, grid, dim3(256), 0, s, A);
        else hipLaunchKernelGGL(k_detnet_upsample2, grid, dim3(256), 0, s, A);
    }
    EAO_HIP(hipGetLastError());
    return EAO_OK;
}

// a diagnostic cannot fail a product call: a failed event call costs the measurement and clears the sticky error
bool mark(eao_detnet* h, size_t k, hipStream_t s) {
    if ((h->ev[k] || hipEventCreate(&h->ev[k]) == hipSuccess) && hipEventRecord(h->ev[k], s) == hipSuccess) return true;
    (void)hipGetLastError();
    return false;
}

eao_status check_tensor(const eao_detnet* h, int32_t tensor, int32_t frame, const void* p) {
    EAO_REQUIRE(h && p, "null argument");
    EAO_REQUIRE(tensor >= 1 && (size_t)tensor < h->net.tensors.size() && h->net.tensors[(size_t)tensor].kind != HEAD,
                "tensor = %d is not an activation map of this model (1 .. %zu, the head excepted)", tensor, h->net.tensors.size() - 1);
    EAO_REQUIRE(frame >= 0 && frame < h->maxBatch, "frame = %d is outside 0 .. max_batch - 1 = %d", frame, h->maxBatch - 1);
    return EAO_OK;
}

}  // namespace

extern "C" {

eao_status eao_detnet_create(const void* model, int64_t bytes, int32_t input_size, int32_t max_batch, eao_detnet** out) {
    EAO_REQUIRE(model && out, "null argument");
    EAO_REQUIRE(bytes >= 0, "bytes = %lld", (long long)bytes);
    EAO_REQUIRE(max_batch >= 1 && max_batch <= EAO_YOLOX_MAX_BATCH, "max_batch = %d is outside 1 .. %d", max_batch, EAO_YOLOX_MAX_BATCH);
    eao_detnet* h = new (std::nothrow) eao_detnet;
    if (!h) { eao::set_error("out of memory"); return EAO_ERR_INTERNAL; }
    auto fail = [&](eao_status s) { delete h; return s; };
    std::string why;
    if (!load(model, (uint64_t)bytes, input_size, true, &h->net, &why)) {
        eao::set_error("the model is refused: %s", why.c_str());
        return fail(EAO_ERR_INVALID);
    }
    const Net& net = h->net;
    if ((double)net.actFloats * max_batch * 4.0 > 32.0 * 1073741824.0 || (double)net.anchors * net.row * max_batch > 2147483647.0) {
        eao::set_error("max_batch = %d frames of %zu activation floats exceed 32 GiB, or the head exceeds 2^31 floats", max_batch, net.actFloats);
        return fail(EAO_ERR_INVALID);
    }
    eao_status st = eao::require_device();
    if (st) return fail(st);
    h->maxBatch = max_batch;
    if ((st = h->weights.reserve(net.weightCount ? net.weightCount : 1)) || (st = h->act.reserve(net.actFloats * (size_t)max_batch + 64))) return fail(st);
    if (net.weightCount && hipMemcpy(h->weights.p, net.weights, net.weightCount * 4, hipMemcpyHostToDevice) != hipSuccess) {
        eao::set_error("the weight upload failed");
        return fail(EAO_ERR_NO_DEVICE);
    }
    if (hipMemset(h->act.p, 0, h->act.n * 4) != hipSuccess) { eao::set_error("clearing the activations failed"); return fail(EAO_ERR_NO_DEVICE); }
    h->net.own.clear(); h->net.own.shrink_to_fit(); h->net.weights = nullptr;      // (the weights live on the device from here)
    h->ev.assign(net.ops.size() + 1, nullptr);
    h->ms.assign(net.ops.size(), -1.f);
    *out = h;
    return EAO_OK;
}

eao_status eao_detnet_create_from_file(const char* path, int32_t input_size, int32_t max_batch, eao_detnet** out) {
    EAO_REQUIRE(path && out, "null argument");
    std::ifstream in(path, std::ios::binary | std::ios::ate);
    EAO_REQUIRE(in.good(), "cannot open %s", path);
    const std::streamoff size = in.tellg();
    EAO_REQUIRE(size >= 0, "cannot size %s", path);
    std::vector<char> buf((size_t)size);
    in.seekg(0);
    if (size) in.read(buf.data(), size);
    EAO_REQUIRE(in.good(), "cannot read %s", path);
    static const char none = 0;
    return eao_detnet_create(size ? buf.data() : &none, (int64_t)size, input_size, max_batch, out);
}

void eao_detnet_destroy(eao_detnet* h) { delete h; }

eao_status eao_detnet_info(const eao_detnet* h, eao_detnet_desc* info) {
    EAO_REQUIRE(h && info, "null argument");
    const Net& net = h->net;
    info->classes = net.classes; info->anchors = net.anchors; info->tensors = (int32_t)net.tensors.size(); info->ops = (int32_t)net.ops.size();
    info->input_size = net.S; info->max_batch = h->maxBatch;
    info->weight_bytes = (int64_t)net.weightCount * 4; info->activation_bytes = (int64_t)h->act.n * 4;
    info->flops = net.flops;
    return EAO_OK;
}

eao_status eao_detnet_forward(eao_detnet* h, const float* d_blob, float* d_prob, int32_t batch, void* stream) {
    EAO_REQUIRE(h && d_blob, "null argument");
    EAO_REQUIRE(d_prob || h->net.head < 0, "d_prob is NULL and the model has a head");
    EAO_REQUIRE(batch >= 1 && batch <= h->maxBatch, "batch = %d is outside 1 .. max_batch = %d", batch, h->maxBatch);
    std::lock_guard<std::mutex> lock(h->mutex);
    hipStream_t s = (hipStream_t)stream;
    const size_t n = h->net.ops.size();
    bool prev = h->profiling && mark(h, 0, s);
    std::vector<uint8_t> ok(h->profiling ? n : 0, 0);
    for (size_t i = 0; i < n; i++) {
        eao_status st = launch_op(h, h->net.ops[i], d_blob, d_prob, batch, s);
        if (st) return st;
        if (h->profiling) {
            const bool now = mark(h, i + 1, s);
            ok[i] = prev && now;
            prev = now;
        }
    }
    if (h->profiling) {      // (a measurement reads its events: the call waits for them)
        EAO_HIP(hipStreamSynchronize(s));
        for (size_t i = 0; i < n; i++) {
            h->ms[i] = -1.f;
            if (ok[i] && hipEventElapsedTime(&h->ms[i], h->ev[i], h->ev[i + 1]) != hipSuccess) { h->ms[i] = -1.f; (void)hipGetLastError(); }
        }
    }
    return EAO_OK;
}

eao_status eao_detnet_tensor(eao_detnet* h, int32_t tensor, int32_t frame, float* out) {
    eao_status st = check_tensor(h, tensor, frame, out);
    if (st) return st;
    std::lock_guard<std::mutex> lock(h->mutex);
    const Tensor& T = h->net.tensors[(size_t)tensor];
    EAO_HIP(hipDeviceSynchronize());      // (an inspection call: whatever stream the last forward ran on has finished)
    EAO_HIP(hipMemcpy(out, h->act.p + (size_t)frame * h->net.actFloats + T.offset, (size_t)T.H * T.W * T.C * 4, hipMemcpyDeviceToHost));
    return EAO_OK;
}

eao_status eao_detnet_set_tensor(eao_detnet* h, int32_t tensor, int32_t frame, const float* in) {
    eao_status st = check_tensor(h, tensor, frame, in);
    if (st) return st;
    std::lock_guard<std::mutex> lock(h->mutex);
    const Tensor& T = h->net.tensors[(size_t)tensor];
    EAO_HIP(hipDeviceSynchronize());
    EAO_HIP(hipMemcpy(h->act.p + (size_t)frame * h->net.actFloats + T.offset, in, (size_t)T.H * T.W * T.C * 4, hipMemcpyHostToDevice));
    return EAO_OK;
}

eao_status eao_detnet_set_profiling(eao_detnet* h, int32_t on) {
    EAO_REQUIRE(h, "null argument");
    std::lock_guard<std::mutex> lock(h->mutex);
    h->profiling = on != 0;
    for (float& m : h->ms) m = -1.f;
    return EAO_OK;
}

eao_status eao_detnet_last_op_ms(eao_detnet* h, float* op_ms, int32_t cap) {
    EAO_REQUIRE(h && op_ms, "null argument");
    std::lock_guard<std::mutex> lock(h->mutex);
    EAO_REQUIRE(cap >= (int32_t)h->ms.size(), "cap = %d is below the %zu ops", cap, h->ms.size());
    bool any = false;
    for (float m : h->ms) any = any || m >= 0.f;
    EAO_REQUIRE(any, "no measurement on this handle: eao_detnet_set_profiling(h, 1) and a forward come first");
    for (size_t i = 0; i < h->ms.size(); i++) op_ms[i] = h->ms[i];
    return EAO_OK;
}

}  // extern "C"
