// object_cuboid.hip -- a map object's cuboid on the device: Object_Map::ComputeMeanAndStandard (reference src/Object.cc:999-1235) with both of its calls of
// Object_Map::UpdateObjPose (:2243-2303), and the pairwise overlap test (Object_Map::WhetherOverlap, :1954-1970; src/LocalMapping.cc:858-877).  Bit for bit what
// upstream's loops compute (csrc/object_cuboid_internal.h holds the literal form and the scalar steps both sides share).
//
//   k_object_cuboids  one workgroup per object, whatever its size: the order-dependent sums are one lane's work however the object is spread, the passes around
//                     them (staging, squares, the change of frame, the extrema) use all 256 lanes, and a batch has far fewer objects (a frame's 8, a map's 64)
//                     than the device has compute units, so a wave per small object would free nothing anybody waits for.
//                       A. the points go to LDS in chunks of kChunk; lanes 0, 1 and 2 add them in list order, one coordinate each (:1020): a dependent chain of n
//                          float adds, the price of bit-for-bit parity.  Every lane keeps the world-frame extrema of the points it staged (:1073-1090; upstream
//                          sorts, the ends of a sorted list are its extrema).
//                       B. mCenter3D; the squares about it of a chunk of points AND of a chunk of centroids go to LDS in parallel, with each centroid's distance
//                          (one sqrt per centroid, :1232); lanes 0-2 of wave 0 add the points' squares (:1038-1040), lanes 0-3 of wave 1 the centroids' squares
//                          and distances (:1062-1064, :1232) at the same time
//                       C. one lane: the world box (n_centroids < 5) and the first UpdateObjPose; pose.inverse() goes to LDS
//                       D. every point into the object frame in double, narrowed to float (:1137-1140); the six extrema
//                       E. one lane: corners, scale, cuboidCenter, the second UpdateObjPose, mfRMax; the record is assembled in LDS and stored by all lanes as
//                          whole words
//                     Among equal extrema (-0.0f beside +0.0f) the smallest list position wins: a lane walks its points in ascending order with a strict
//                     comparison, and lanes are merged by (value, position).  No atomics: two calls return the same bytes.
//   k_object_overlaps one lane per ordered pair.
#include <cstring>
#include <vector>

#include "common.h"
#include "object_cuboid_internal.h"

namespace {

using namespace eao::object_cuboid;

constexpr int kBlock = 256;                  // four wavefronts
constexpr int kWaves = kBlock / 64;
constexpr int kChunk = 1024;                 // list entries whose terms wait in LDS for the ordered adds
constexpr int kNone = 0x7fffffff;            // the list position of a lane that has seen no point

static_assert(sizeof(eao_object_cuboid_rec) == 752, "record layout");
static_assert(sizeof(eao_object_overlap_row) == 40, "row layout");
constexpr int kRecWords = sizeof(eao_object_cuboid_rec) / 4;

struct Ext {      // the six extrema of a lane, each with the list position that holds it
    float v[6];
    int at[6];
};

__device__ __forceinline__ void ext_init(Ext& e) {
#pragma unroll
    for (int k = 0; k < 6; k++) {
        e.v[k] = (k & 1) ? -INFINITY : INFINITY;
        e.at[k] = kNone;
    }
}

// positions ascend within a lane: a strict comparison keeps the first of equal values
__device__ __forceinline__ void ext_take(Ext& e, const float* p, int at) {
#pragma unroll
    for (int a = 0; a < 3; a++) {
        if (p[a] < e.v[2 * a] || e.at[2 * a] == kNone) { e.v[2 * a] = p[a]; e.at[2 * a] = at; }
        if (p[a] > e.v[2 * a + 1] || e.at[2 * a + 1] == kNone) { e.v[2 * a + 1] = p[a]; e.at[2 * a + 1] = at; }
    }
}

__device__ __forceinline__ void ext_merge(float& v, int& at, float ov, int oat, bool isMax) {
    const bool better = oat != kNone && (at == kNone || (isMax ? ov > v : ov < v) || (ov == v && oat < at));
    if (better) { v = ov; at = oat; }
}

// the workgroup's extrema in out[0..5], valid for every thread after the call (two barriers)
__device__ __forceinline__ void ext_reduce(Ext& e, float (*sV)[6], int (*sAt)[6], float* out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 6; k++) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const float ov = __shfl_xor(e.v[k], d, 64);
            const int oat = __shfl_xor(e.at[k], d, 64);
            ext_merge(e.v[k], e.at[k], ov, oat, (k & 1) != 0);
        }
        if (lane == 0) { sV[wave][k] = e.v[k]; sAt[wave][k] = e.at[k]; }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 6; k++) {
        float v = sV[0][k];
        int at = sAt[0][k];
#pragma unroll
        for (int w = 1; w < kWaves; w++) ext_merge(v, at, sV[w][k], sAt[w][k], (k & 1) != 0);
        out[k] = v;
    }
    __syncthreads();      // sV, sAt are free again
}

__global__ __launch_bounds__(kBlock) void k_object_cuboids(const ObjDev* __restrict__ objs, const float* __restrict__ points, const float* __restrict__ centroids,
                                                           eao_object_cuboid_rec* __restrict__ records) {
    __shared__ float sP[3][kChunk];
    __shared__ float sC[4][kChunk];
    __shared__ float sV[kWaves][6];
    __shared__ int sAt[kWaves][6];
    __shared__ float sSum[3], sSum2[3], sCen[4];
    __shared__ Pose sInv;
    __shared__ eao_object_cuboid_rec sRec;
    __shared__ Pose sPose[2];
    const ObjDev& O = objs[blockIdx.x];
    if (O.skip) return;      // (uniform) an object of a chain whose point update did not finish
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int n = O.n, m = O.m;
    const float* P = points + 3 * (size_t)O.pointStart;
    const float* Cn = centroids + 3 * (size_t)O.centroidStart;

    for (int k = t; k < kRecWords; k += kBlock) ((uint32_t*)&sRec)[k] = 0u;      // fields upstream leaves untouched are zero

    // A. mSumPointsPos and the world-frame extrema
    Ext ew;
    ext_init(ew);
    float acc = 0.0f;
    for (int c0 = 0; c0 < n; c0 += kChunk) {      // (uniform)
        const int len = n - c0 < kChunk ? n - c0 : kChunk;
        for (int j = t; j < len; j += kBlock) {
            const float* p = P + 3 * (size_t)(c0 + j);
            const float v[3] = {p[0], p[1], p[2]};
            sP[0][j] = v[0]; sP[1][j] = v[1]; sP[2][j] = v[2];
            ext_take(ew, v, c0 + j);
        }
        __syncthreads();
        if (t < 3)
            for (int j = 0; j < len; j++) acc = acc + sP[t][j];
        __syncthreads();
    }
    if (t < 3) sSum[t] = acc;
    __syncthreads();
    float center[3];
#pragma unroll
    for (int a = 0; a < 3; a++) center[a] = mat_div(sSum[a], n);

    if (n == 0) {      // :1050 (uniform): the sums of step 1 are empty, 0 / 0
        if (t == 0) {
            for (int a = 0; a < 3; a++) {
                sRec.sum_pos[a] = sSum[a];
                sRec.center[a] = center[a];
                sRec.standar[a] = sqrt_f(0.0f / (float)n);
            }
            sRec.status = EAO_OBJECT_CUBOID_EMPTY;
        }
        __syncthreads();
        for (int k = t; k < kRecWords; k += kBlock) ((uint32_t*)(records + blockIdx.x))[k] = ((const uint32_t*)&sRec)[k];
        return;
    }

    // B. the squares about mCenter3D: the points' on wave 0, the centroids' (and their distances) on wave 1
    const int passes = ((n > m ? n : m) + kChunk - 1) / kChunk;
    acc = 0.0f;
    for (int ps = 0; ps < passes; ps++) {      // (uniform)
        const int c0 = ps * kChunk;      // (n, m <= 2^27: checked by the host)
        const int lenP = n - c0 < kChunk ? (n - c0 > 0 ? n - c0 : 0) : kChunk, lenC = m - c0 < kChunk ? (m - c0 > 0 ? m - c0 : 0) : kChunk;
        for (int j = t; j < lenP; j += kBlock) {
            const float* p = P + 3 * (size_t)(c0 + j);
#pragma unroll
            for (int a = 0; a < 3; a++) sP[a][j] = (p[a] - center[a]) * (p[a] - center[a]);
        }
        for (int j = t; j < lenC; j += kBlock) {
            const float* c = Cn + 3 * (size_t)(c0 + j);
            const float cv[3] = {c[0], c[1], c[2]};
            float sq[3], dis;
            centroid_terms(cv, center, sq, &dis);
            sC[0][j] = sq[0]; sC[1][j] = sq[1]; sC[2][j] = sq[2]; sC[3][j] = dis;
        }
        __syncthreads();
        if (wave == 0 && lane < 3)
            for (int j = 0; j < lenP; j++) acc = acc + sP[lane][j];
        if (wave == 1 && lane < 4)
            for (int j = 0; j < lenC; j++) acc = acc + sC[lane][j];
        __syncthreads();
    }
    if (wave == 0 && lane < 3) sSum2[lane] = acc;
    if (wave == 1 && lane < 4) sCen[lane] = acc;
    __syncthreads();

    // C. the world box and the first UpdateObjPose
    const bool few = m < kFewFrames;      // (uniform)
    float ext[6];
    if (few) ext_reduce(ew, sV, sAt, ext);
    if (t == 0) {
        eao_object_cuboid_rec& r = sRec;
        r.status = EAO_OBJECT_CUBOID_DONE;
        for (int a = 0; a < 3; a++) {
            r.sum_pos[a] = sSum[a];
            r.center[a] = center[a];
            r.standar[a] = sqrt_f(sSum2[a] / (float)n);
            r.center_standar[a] = sqrt_f(sCen[a] / (float)m);
            r.cuboid_center[a] = O.prev[a];
        }
        r.center_standar_dis = sqrt_f(sCen[3] / (float)m);
        if (few) world_box(ext, r);
        update_obj_pose(O.Ryaw, r, sPose[0], sPose[1]);
        pose_inverse(sPose[0], sInv);
    }
    __syncthreads();

    // D. world -> object frame, and the extrema there
    const Pose inv = sInv;
    Ext eo;
    ext_init(eo);
    for (int i = t; i < n; i += kBlock) {
        const float* p = P + 3 * (size_t)i;
        const float v[3] = {p[0], p[1], p[2]};
        float o[3];
        to_object_frame(inv, v, o);
        ext_take(eo, o, i);
    }
    ext_reduce(eo, sV, sAt, ext);

    // E. corners, scale, cuboidCenter, the second UpdateObjPose, mfRMax
    if (t == 0) object_box(O.Ryaw, ext, sPose[0], sPose[1], sRec);
    __syncthreads();
    for (int k = t; k < kRecWords; k += kBlock) ((uint32_t*)(records + blockIdx.x))[k] = ((const uint32_t*)&sRec)[k];
}

__global__ __launch_bounds__(kBlock) void k_object_overlaps(int m, const eao_object_overlap_row* __restrict__ rows, const uint8_t* __restrict__ eligible,
                                                            uint8_t* __restrict__ verdict, float* __restrict__ extents) {
    const int64_t pair = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (pair >= (int64_t)m * m) return;
    const int i = (int)(pair / m), j = (int)(pair % m);
    float e[3];
    const bool hit = overlap(rows[i], rows[j], e);
    const bool v = i != j && eligible[i] != 0 && eligible[j] != 0 && hit;
    verdict[pair] = v ? 1 : 0;
    extents[3 * pair] = e[0];
    extents[3 * pair + 1] = e[1];
    extents[3 * pair + 2] = e[2];
}

struct ObjectCuboidCtx : eao::ThreadStream {
    eao::DevBuf<unsigned char> dev;
    eao::PinBuf<hipHostMallocDefault> host;
    eao::KernelClock<2> clock;      // k_object_cuboids, k_object_overlaps of the last calls that reached the device
};
thread_local ObjectCuboidCtx g_oc;

}  // namespace

namespace eao {
namespace object_cuboid {

hipError_t enqueue_cuboids(hipStream_t stream, const ObjDev* objs, const float* points, const float* centroids, eao_object_cuboid_rec* records, unsigned n_obj) {
    hipLaunchKernelGGL(k_object_cuboids, dim3(n_obj), dim3(kBlock), 0, stream, objs, points, centroids, records);
    return hipGetLastError();
}

}  // namespace object_cuboid
}  // namespace eao

extern "C" {

eao_status eao_object_cuboids_batch(int32_t n_obj, const eao_object_cuboid_desc* objs, eao_object_cuboid_rec* recs) {
    EAO_REQUIRE(n_obj >= 0 && n_obj <= kMaxObjects, "n_obj outside 0 .. %d", kMaxObjects);
    EAO_REQUIRE(n_obj == 0 || (objs && recs), "null argument");
    int64_t nPts = 0, nCen = 0;
    for (int32_t k = 0; k < n_obj; k++) {
        EAO_REQUIRE(objs[k].n_points >= 0 && objs[k].n_centroids >= 0, "object %d: a negative count", k);
        nPts += objs[k].n_points;
        nCen += objs[k].n_centroids;
        EAO_REQUIRE(nPts + nCen <= kMaxBatchEntries, "more than 2^27 points and centroids in one call: split it");
    }
    for (int32_t k = 0; k < n_obj; k++) {
        const char* why = object_refusal(objs[k]);
        EAO_REQUIRE(!why, "object %d: %s", k, why);
    }
    if (n_obj == 0) return EAO_OK;

    ObjectCuboidCtx& ctx = g_oc;
    eao_status st = ctx.ready(eao::StreamClass::Latency);
    if (st) return st;
    const size_t nO = (size_t)n_obj;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t at = off; off = eao::align256(off + bytes); return at; };
    const size_t oObj = take(nO * sizeof(ObjDev)), oPts = take((size_t)nPts * 12), oCen = take((size_t)nCen * 12), inEnd = off;
    const size_t oRec = take(nO * sizeof(eao_object_cuboid_rec)), end = off;
    if ((st = ctx.dev.reserve(end))) return st;
    if ((st = ctx.host.reserve(end))) return st;
    unsigned char *d = ctx.dev.p, *h = ctx.host.p;
    ObjDev* ho = (ObjDev*)(h + oObj);
    int64_t p = 0, c = 0;
    for (int32_t k = 0; k < n_obj; k++) {
        const eao_object_cuboid_desc& D = objs[k];
        ObjDev O{};
        O.pointStart = p; O.centroidStart = c; O.n = D.n_points; O.m = D.n_centroids;
        std::memcpy(O.Ryaw, D.Ryaw, sizeof(O.Ryaw));
        std::memcpy(O.prev, D.prev_cuboid_center, sizeof(O.prev));
        ho[k] = O;
        if (D.n_points > 0) std::memcpy(h + oPts + (size_t)p * 12, D.points, (size_t)D.n_points * 12);
        if (D.n_centroids > 0) std::memcpy(h + oCen + (size_t)c * 12, D.centroids, (size_t)D.n_centroids * 12);
        p += D.n_points;
        c += D.n_centroids;
    }
    eao::Drain drain(ctx.stream);
    EAO_HIP(hipMemcpyAsync(d, h, inEnd, hipMemcpyHostToDevice, ctx.stream));
    ctx.clock.mark(0, ctx.stream);
    EAO_HIP(enqueue_cuboids(ctx.stream, (const ObjDev*)(d + oObj), (const float*)(d + oPts), (const float*)(d + oCen), (eao_object_cuboid_rec*)(d + oRec), (unsigned)nO));
    ctx.clock.mark(1, ctx.stream);
    EAO_HIP(hipMemcpyAsync(h + oRec, d + oRec, nO * sizeof(eao_object_cuboid_rec), hipMemcpyDeviceToHost, ctx.stream));
    EAO_HIP(drain.wait(eao::Drain::Latency));
    ctx.clock.collect();
    std::memcpy(recs, h + oRec, nO * sizeof(eao_object_cuboid_rec));
    return EAO_OK;
}

eao_status eao_object_cuboids(const eao_object_cuboid_desc* obj, eao_object_cuboid_rec* rec) {
    EAO_REQUIRE(obj && rec, "null argument");
    return eao_object_cuboids_batch(1, obj, rec);
}

eao_status eao_object_overlaps(int32_t m, const eao_object_overlap_row* rows, const uint8_t* eligible, uint8_t* verdict, float* extents) {
    const char* why = overlap_refusal(m, rows, eligible, verdict);
    EAO_REQUIRE(!why, "%s", why);
    if (m == 0) return EAO_OK;

    ObjectCuboidCtx& ctx = g_oc;
    eao_status st = ctx.ready(eao::StreamClass::Latency);
    if (st) return st;
    const size_t M = (size_t)m, pairs = M * M;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t at = off; off = eao::align256(off + bytes); return at; };
    const size_t oRows = take(M * sizeof(eao_object_overlap_row)), oEl = take(M), inEnd = off;
    const size_t oVer = take(pairs), oExt = take(pairs * 12), end = off;
    if ((st = ctx.dev.reserve(end))) return st;
    if ((st = ctx.host.reserve(end))) return st;
    unsigned char *d = ctx.dev.p, *h = ctx.host.p;
    std::memcpy(h + oRows, rows, M * sizeof(eao_object_overlap_row));
    std::memcpy(h + oEl, eligible, M);
    eao::Drain drain(ctx.stream);
    EAO_HIP(hipMemcpyAsync(d, h, inEnd, hipMemcpyHostToDevice, ctx.stream));
    ctx.clock.mark(1, ctx.stream);
    hipLaunchKernelGGL(k_object_overlaps, dim3((unsigned)((pairs + kBlock - 1) / kBlock)), dim3(kBlock), 0, ctx.stream, (int)m, (const eao_object_overlap_row*)(d + oRows),
                       (const uint8_t*)(d + oEl), (uint8_t*)(d + oVer), (float*)(d + oExt));
    EAO_HIP(hipGetLastError());
    ctx.clock.mark(2, ctx.stream);
    EAO_HIP(hipMemcpyAsync(h + oVer, d + oVer, (extents ? end : oExt) - oVer, hipMemcpyDeviceToHost, ctx.stream));
    EAO_HIP(drain.wait(eao::Drain::Latency));
    ctx.clock.collect();
    std::memcpy(verdict, h + oVer, pairs);
    if (extents) {
        const float* e = (const float*)(h + oExt);
        for (size_t k = 0; k < pairs; k++)
            if (verdict[k]) std::memcpy(extents + 3 * k, e + 3 * k, 12);
    }
    return EAO_OK;
}

eao_status eao_object_cuboid_set_profiling(int32_t on) {
    g_oc.clock.arm(on != 0);
    return EAO_OK;
}

eao_status eao_object_cuboid_last_kernel_ms(float* kernel_ms) {
    EAO_REQUIRE(kernel_ms, "null argument");
    return g_oc.clock.read(kernel_ms, "no measurement on this thread: eao_object_cuboid_set_profiling(1) and a call that reaches the device come first");
}

}  // extern "C"
