// object_assoc.hip -- the object layer's per-frame data association on the device (Tracking step 10, reference src/Tracking.cc:2036-2069): the rank-sum test of
// Object_2D::NoParaDataAssociation (src/Object.cc:728-962) for many (detection, map object) pairs in one call, and Object_Map::ComputeProjectRectFrame
// (:1606-1651) for many map objects.  Everything is integer or bit-exact (csrc/object_assoc_internal.h states why no sort is needed).
//
//   k_np_counts       one workgroup per pair.  A thread owns detection points; the map object's good points stream through LDS in tiles of kTile, one array per
//                     axis, so every lane reads the same address (a broadcast).  Per owned point and axis a thread counts the map values below it (lb) and not
//                     above it (ub); after the last tile the ceil(. / step) rule turns them into upstream's three counters over the strided sample.  A wave
//                     reduction and a cross-wave reduction through LDS give nine sums; one thread stores them.  No atomics: the result does not depend on timing.
//                     A pair's map points are not split across workgroups: ceil(lb / step) needs the complete lb.
//   k_project_rects   one wavefront per map object, lanes over its points: Rcw X + tcw accumulated in double and rounded once, an IEEE 1.0 / z, u and v in float
//                     operation by operation, then a wave min / max reduction and an any-NaN flag.
//
// The host does the early returns, step and n, the overflow bound, w, r1 / r2 and the verdict, the clamps and the float -> int conversion of cv::Rect.
#include <cstring>
#include <vector>

#include "common.h"
#include "object_assoc_internal.h"

namespace {

using namespace eao::object_assoc;

static_assert(kMinDetPoints == EAO_OBJECT_NP_MIN_DET_POINTS && kMinMapPoints == EAO_OBJECT_NP_MIN_MAP_POINTS && kSampleRatio == EAO_OBJECT_NP_SAMPLE_RATIO &&
                  kCritical == EAO_OBJECT_NP_CRITICAL && kVarianceDivisor == EAO_OBJECT_NP_VARIANCE_DIVISOR && kHalf == EAO_OBJECT_NP_HALF &&
                  kUndefined == EAO_OBJECT_NP_UNDEFINED,
              "include/eao_fusion.h and object_assoc_internal.h state the same rules");

constexpr int kBlock = 256;          // four wavefronts: a detection of 300 points takes one pass of two points per thread
constexpr int kOwned = 2;            // detection points per thread and pass: every LDS read serves both
constexpr int kTile = 1024;          // map points per LDS tile: 3 x 4 KB, so five workgroups fit a CU's 160 KB beside each other
static_assert(kTile % 4 == 0, "the tile is read four values at a time");

struct PairDev {
    uint32_t detStart, m, mapStart, nGood;      // in points
    uint32_t step, n, pad[2];
};
static_assert(sizeof(PairDev) == 32, "PairDev layout");

__device__ __forceinline__ void count4(const float4 v, const float x, unsigned& lb, unsigned& ub) {
    lb += (v.x < x ? 1u : 0u) + (v.y < x ? 1u : 0u) + (v.z < x ? 1u : 0u) + (v.w < x ? 1u : 0u);
    ub += (v.x <= x ? 1u : 0u) + (v.y <= x ? 1u : 0u) + (v.z <= x ? 1u : 0u) + (v.w <= x ? 1u : 0u);
}

__global__ __launch_bounds__(kBlock) void k_np_counts(const PairDev* __restrict__ pairs, const float* __restrict__ detXyz, const float* __restrict__ mapXyz,
                                                      unsigned* __restrict__ counts) {
    __shared__ __attribute__((aligned(16))) float tile[3][kTile];
    __shared__ unsigned part[kBlock / 64][9];
    const PairDev P = pairs[blockIdx.x];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const float* det = detXyz + (size_t)P.detStart * 3;
    const float* map = mapXyz + (size_t)P.mapStart * 3;
    const float quietNan = __builtin_nanf("");      // the tile's tail: a NaN is neither < nor <= anything
    unsigned sum[9];
#pragma unroll
    for (int k = 0; k < 9; k++) sum[k] = 0;

    for (unsigned base = 0; base < P.m; base += kBlock * kOwned) {      // (uniform: every thread of the workgroup reaches every barrier below)
        float x[kOwned][3];
        bool own[kOwned];
        unsigned lb[kOwned][3], ub[kOwned][3];
#pragma unroll
        for (int o = 0; o < kOwned; o++) {
            const unsigned i = base + o * kBlock + t;
            own[o] = i < P.m;
#pragma unroll
            for (int a = 0; a < 3; a++) {
                x[o][a] = own[o] ? det[(size_t)i * 3 + a] : 0.0f;
                lb[o][a] = ub[o][a] = 0;
            }
        }
        for (unsigned first = 0; first < P.nGood; first += kTile) {
            const unsigned have = P.nGood - first < (unsigned)kTile ? P.nGood - first : (unsigned)kTile;
            const unsigned padded = (have + 3u) & ~3u;      // <= kTile
            __syncthreads();      // the previous tile has been read
            for (unsigned j = t; j < padded; j += kBlock) {
                const bool in = j < have;
                const float* p = map + (size_t)(first + j) * 3;
                tile[0][j] = in ? p[0] : quietNan;
                tile[1][j] = in ? p[1] : quietNan;
                tile[2][j] = in ? p[2] : quietNan;
            }
            __syncthreads();
            for (unsigned j = 0; j < padded; j += 4) {
                const float4 vx = *reinterpret_cast<const float4*>(&tile[0][j]);
                const float4 vy = *reinterpret_cast<const float4*>(&tile[1][j]);
                const float4 vz = *reinterpret_cast<const float4*>(&tile[2][j]);
#pragma unroll
                for (int o = 0; o < kOwned; o++) {
                    count4(vx, x[o][0], lb[o][0], ub[o][0]);
                    count4(vy, x[o][1], lb[o][1], ub[o][1]);
                    count4(vz, x[o][2], lb[o][2], ub[o][2]);
                }
            }
        }
#pragma unroll
        for (int o = 0; o < kOwned; o++)
            if (own[o]) {
#pragma unroll
                for (int a = 0; a < 3; a++) {
                    const unsigned kl = (lb[o][a] + P.step - 1) / P.step, ku = (ub[o][a] + P.step - 1) / P.step;
                    sum[3 * a] += kl;
                    sum[3 * a + 1] += P.n - ku;
                    sum[3 * a + 2] += ku - kl;
                }
            }
    }
#pragma unroll
    for (int k = 0; k < 9; k++) {
        unsigned v = sum[k];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
        if (lane == 0) part[wave][k] = v;
    }
    __syncthreads();
    if (t == 0) {
        unsigned* out = counts + (size_t)blockIdx.x * 9;
#pragma unroll
        for (int k = 0; k < 9; k++) {
            unsigned v = 0;
#pragma unroll
            for (int w = 0; w < kBlock / 64; w++) v += part[w][k];
            out[k] = v;
        }
    }
}

struct RectDev {      // what lane 0 of an object's wavefront stores
    float uMin, uMax, vMin, vMax;
    unsigned anyNan, pad[3];
};
static_assert(sizeof(RectDev) == 32, "RectDev layout");
struct RectArgs {
    float T[12];      // rows 0..2 of Tcw
    float fx, fy, cx, cy;
};

constexpr int kRectWaves = 4;
__global__ __launch_bounds__(64 * kRectWaves) void k_project_rects(int nMap, const int* __restrict__ start, const float* __restrict__ xyz, const RectArgs A,
                                                                   RectDev* __restrict__ out, float* __restrict__ uv) {
    const int lane = threadIdx.x & 63;
    const int obj = blockIdx.x * kRectWaves + (threadIdx.x >> 6);
    if (obj >= nMap) return;      // (per wavefront: nothing below waits for another one)
    const int first = start[obj] - start[0], count = start[obj + 1] - start[obj];
    float uMin = INFINITY, uMax = -INFINITY, vMin = INFINITY, vMax = -INFINITY;
    unsigned anyNan = 0;
    for (int i = lane; i < count; i += 64) {
        const float* X = xyz + (size_t)(first + i) * 3;
        const float X0 = X[0], X1 = X[1], X2 = X[2];
        float Pc[3];
#pragma unroll
        for (int r = 0; r < 3; r++) {
            const double acc = (double)A.T[4 * r] * (double)X0 + (double)A.T[4 * r + 1] * (double)X1 + (double)A.T[4 * r + 2] * (double)X2;
            Pc[r] = (float)(acc + (double)A.T[4 * r + 3]);
        }
        const float invzc = (float)(1.0 / (double)Pc[2]);
        const float u = A.fx * Pc[0] * invzc + A.cx;
        const float v = A.fy * Pc[1] * invzc + A.cy;
        if (uv) {
            uv[(size_t)(first + i) * 2] = u;
            uv[(size_t)(first + i) * 2 + 1] = v;
        }
        anyNan |= (u != u || v != v) ? 1u : 0u;
        uMin = u < uMin ? u : uMin;
        uMax = u > uMax ? u : uMax;
        vMin = v < vMin ? v : vMin;
        vMax = v > vMax ? v : vMax;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const float a = __shfl_xor(uMin, d, 64), b = __shfl_xor(uMax, d, 64), c = __shfl_xor(vMin, d, 64), e = __shfl_xor(vMax, d, 64);
        anyNan |= __shfl_xor(anyNan, d, 64);
        uMin = a < uMin ? a : uMin;
        uMax = b > uMax ? b : uMax;
        vMin = c < vMin ? c : vMin;
        vMax = e > vMax ? e : vMax;
    }
    if (lane == 0) {
        RectDev r;
        r.uMin = uMin; r.uMax = uMax; r.vMin = vMin; r.vMax = vMax;
        r.anyNan = anyNan; r.pad[0] = r.pad[1] = r.pad[2] = 0;
        out[obj] = r;
    }
}

struct AssocCtx : eao::ThreadStream {
    eao::DevBuf<unsigned char> dev;
    eao::PinBuf<hipHostMallocDefault> host;
    eao::KernelClock<2> clock;      // k_np_counts between marks 0 and 1, k_project_rects between 1 and 2: each of its own last call
};
thread_local AssocCtx g_assoc;

struct Lists {
    int32_t n_det, n_map, n_pair;
    const int32_t *det_start, *map_start, *map_total, *pair_det, *pair_map;
    const float *det_xyz, *map_xyz;
};

// The checks of include/eao_fusion.h, the plan of every pair, and the device counts of the pairs the plans leave open.  Nothing of the caller's is written.
eao_status run_counts(const Lists& L, std::vector<Plan>& plans, std::vector<uint32_t>& counts) {
    EAO_REQUIRE(L.n_det >= 0 && L.n_map >= 0 && L.n_pair >= 0, "a negative count");
    plans.clear();
    counts.assign((size_t)L.n_pair * 9, 0u);
    if (L.n_pair == 0) return EAO_OK;
    EAO_REQUIRE(L.pair_det && L.pair_map, "null argument");
    EAO_REQUIRE(L.n_det == 0 || L.det_start, "det_start is NULL");
    EAO_REQUIRE(L.n_map == 0 || (L.map_start && L.map_total), "map_start or map_total is NULL");
    const char* why = L.n_det ? starts_refusal(L.n_det, L.det_start) : nullptr;
    EAO_REQUIRE(!why, "det_start: %s", why);
    why = L.n_map ? starts_refusal(L.n_map, L.map_start) : nullptr;
    EAO_REQUIRE(!why, "map_start: %s", why);
    for (int32_t j = 0; j < L.n_map; j++) {
        EAO_REQUIRE(L.map_total[j] >= 0, "map_total[%d] < 0", j);
        EAO_REQUIRE((int64_t)L.map_total[j] >= (int64_t)L.map_start[j + 1] - L.map_start[j], "map_total[%d] is below the number of good points", j);
    }
    plans.resize((size_t)L.n_pair);
    std::vector<PairDev> open;
    std::vector<int32_t> owner;
    std::vector<uint8_t> detRead((size_t)L.n_det, 0), mapRead((size_t)L.n_map, 0);
    for (int32_t p = 0; p < L.n_pair; p++) {
        const int32_t d = L.pair_det[p], j = L.pair_map[p];
        EAO_REQUIRE(d >= 0 && d < L.n_det && j >= 0 && j < L.n_map, "pair %d names detection %d / map object %d out of range", p, d, j);
        const int32_t m = L.det_start[d + 1] - L.det_start[d], nGood = L.map_start[j + 1] - L.map_start[j];
        plans[p] = plan_pair(m, nGood, L.map_total[j]);
        if (plans[p].verdict != kPending) continue;
        detRead[d] = mapRead[j] = 1;
        PairDev P{};
        P.detStart = (uint32_t)(L.det_start[d] - L.det_start[0]); P.m = (uint32_t)m;
        P.mapStart = (uint32_t)(L.map_start[j] - L.map_start[0]); P.nGood = (uint32_t)nGood;
        P.step = (uint32_t)plans[p].step; P.n = (uint32_t)plans[p].n;
        open.push_back(P);
        owner.push_back(p);
    }
    if (open.empty()) return EAO_OK;
    EAO_REQUIRE(L.det_xyz && L.map_xyz, "null argument");
    for (int32_t d = 0; d < L.n_det; d++)
        EAO_REQUIRE(!detRead[d] || !any_nan(L.det_xyz + (size_t)L.det_start[d] * 3, (size_t)(L.det_start[d + 1] - L.det_start[d])), "detection %d has a NaN coordinate", d);
    for (int32_t j = 0; j < L.n_map; j++)
        EAO_REQUIRE(!mapRead[j] || !any_nan(L.map_xyz + (size_t)L.map_start[j] * 3, (size_t)(L.map_start[j + 1] - L.map_start[j])), "map object %d has a NaN coordinate", j);

    AssocCtx& ctx = g_assoc;
    eao_status st = ctx.ready(eao::StreamClass::Latency);
    if (st) return st;
    const size_t nDetPts = (size_t)(L.det_start[L.n_det] - L.det_start[0]), nMapPts = (size_t)(L.map_start[L.n_map] - L.map_start[0]), nOpen = open.size();
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t at = off; off = eao::align256(off + bytes); return at; };
    const size_t oDet = take(nDetPts * 12), oMap = take(nMapPts * 12), oPair = take(nOpen * sizeof(PairDev)), inEnd = off;
    const size_t oCnt = take(nOpen * 36), end = off;
    if ((st = ctx.dev.reserve(end))) return st;
    if ((st = ctx.host.reserve(end))) return st;
    unsigned char *d = ctx.dev.p, *h = ctx.host.p;
    std::memcpy(h + oDet, L.det_xyz + (size_t)L.det_start[0] * 3, nDetPts * 12);
    std::memcpy(h + oMap, L.map_xyz + (size_t)L.map_start[0] * 3, nMapPts * 12);
    std::memcpy(h + oPair, open.data(), nOpen * sizeof(PairDev));
    eao::Drain drain(ctx.stream);
    EAO_HIP(hipMemcpyAsync(d, h, inEnd, hipMemcpyHostToDevice, ctx.stream));
    ctx.clock.mark(0, ctx.stream);
    hipLaunchKernelGGL(k_np_counts, dim3((unsigned)nOpen), dim3(kBlock), 0, ctx.stream, (const PairDev*)(d + oPair), (const float*)(d + oDet), (const float*)(d + oMap),
                       (unsigned*)(d + oCnt));
    EAO_HIP(hipGetLastError());
    ctx.clock.mark(1, ctx.stream);
    EAO_HIP(hipMemcpyAsync(h + oCnt, d + oCnt, nOpen * 36, hipMemcpyDeviceToHost, ctx.stream));
    EAO_HIP(drain.wait(eao::Drain::Latency));
    ctx.clock.collect();
    for (size_t q = 0; q < nOpen; q++) std::memcpy(counts.data() + (size_t)owner[q] * 9, h + oCnt + q * 36, 36);
    return EAO_OK;
}

}  // namespace

extern "C" {

eao_status eao_object_np_counts_batch(int32_t n_det, const int32_t* det_start, const float* det_xyz, int32_t n_map, const int32_t* map_start, const float* map_xyz,
                                      const int32_t* map_total, int32_t n_pair, const int32_t* pair_det, const int32_t* pair_map, int32_t* mns, uint32_t* counts) {
    EAO_REQUIRE(n_pair <= 0 || (mns && counts), "null argument");
    std::vector<Plan> plans;
    std::vector<uint32_t> c;
    const eao_status st = run_counts(Lists{n_det, n_map, n_pair, det_start, map_start, map_total, pair_det, pair_map, det_xyz, map_xyz}, plans, c);
    if (st) return st;
    for (int32_t p = 0; p < n_pair; p++) {
        mns[3 * p] = plans[p].m;
        mns[3 * p + 1] = plans[p].n;
        mns[3 * p + 2] = plans[p].step;
    }
    if (n_pair > 0) std::memcpy(counts, c.data(), c.size() * 4);
    return EAO_OK;
}

eao_status eao_object_np_association_batch(int32_t n_det, const int32_t* det_start, const float* det_xyz, int32_t n_map, const int32_t* map_start,
                                           const float* map_xyz, const int32_t* map_total, int32_t n_pair, const int32_t* pair_det, const int32_t* pair_map,
                                           int32_t* verdict, float* w, float* r) {
    EAO_REQUIRE(n_pair <= 0 || verdict, "null argument");
    std::vector<Plan> plans;
    std::vector<uint32_t> c;
    const eao_status st = run_counts(Lists{n_det, n_map, n_pair, det_start, map_start, map_total, pair_det, pair_map, det_xyz, map_xyz}, plans, c);
    if (st) return st;
    for (int32_t p = 0; p < n_pair; p++) {
        float wp[3] = {0, 0, 0}, rp[2] = {0, 0};
        verdict[p] = plans[p].verdict != kPending ? plans[p].verdict : decide(plans[p].m, plans[p].n, c.data() + (size_t)p * 9, wp, rp);
        if (w) std::memcpy(w + (size_t)p * 3, wp, 12);
        if (r) std::memcpy(r + (size_t)p * 2, rp, 8);
    }
    return EAO_OK;
}

eao_status eao_object_project_rects_batch(int32_t n_map, const int32_t* map_start, const float* map_xyz, const float* Tcw, float fx, float fy, float cx, float cy,
                                          int32_t cols, int32_t rows, int32_t* rect, uint8_t* status, float* uv) {
    EAO_REQUIRE(n_map >= 0 && cols >= 0 && rows >= 0, "a negative count");
    if (n_map == 0) return EAO_OK;
    EAO_REQUIRE(map_start && Tcw && rect && status, "null argument");
    const char* why = starts_refusal(n_map, map_start);
    EAO_REQUIRE(!why, "map_start: %s", why);
    const size_t nPts = (size_t)(map_start[n_map] - map_start[0]);
    if (nPts == 0) {
        std::memset(status, kRectEmpty, (size_t)n_map);
        return EAO_OK;
    }
    EAO_REQUIRE(map_xyz, "map_xyz is NULL");
    AssocCtx& ctx = g_assoc;
    eao_status st = ctx.ready(eao::StreamClass::Latency);
    if (st) return st;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t at = off; off = eao::align256(off + bytes); return at; };
    const size_t oXyz = take(nPts * 12), oStart = take(((size_t)n_map + 1) * 4), inEnd = off;
    const size_t oOut = take((size_t)n_map * sizeof(RectDev)), oUv = take(uv ? nPts * 8 : 0), end = off;
    if ((st = ctx.dev.reserve(end))) return st;
    if ((st = ctx.host.reserve(end))) return st;
    unsigned char *d = ctx.dev.p, *h = ctx.host.p;
    std::memcpy(h + oXyz, map_xyz + (size_t)map_start[0] * 3, nPts * 12);
    std::memcpy(h + oStart, map_start, ((size_t)n_map + 1) * 4);
    RectArgs A;
    std::memcpy(A.T, Tcw, sizeof(A.T));
    A.fx = fx; A.fy = fy; A.cx = cx; A.cy = cy;
    eao::Drain drain(ctx.stream);
    EAO_HIP(hipMemcpyAsync(d, h, inEnd, hipMemcpyHostToDevice, ctx.stream));
    ctx.clock.mark(1, ctx.stream);
    hipLaunchKernelGGL(k_project_rects, dim3((unsigned)eao::cdiv(n_map, kRectWaves)), dim3(64 * kRectWaves), 0, ctx.stream, (int)n_map, (const int*)(d + oStart),
                       (const float*)(d + oXyz), A, (RectDev*)(d + oOut), uv ? (float*)(d + oUv) : nullptr);
    EAO_HIP(hipGetLastError());
    ctx.clock.mark(2, ctx.stream);
    EAO_HIP(hipMemcpyAsync(h + oOut, d + oOut, end - oOut, hipMemcpyDeviceToHost, ctx.stream));
    EAO_HIP(drain.wait(eao::Drain::Latency));
    ctx.clock.collect();
    const RectDev* out = (const RectDev*)(h + oOut);
    for (int32_t j = 0; j < n_map; j++) {
        if (map_start[j + 1] == map_start[j]) {
            status[j] = kRectEmpty;      // `return` at :1631
            continue;
        }
        const Extent e{out[j].uMin, out[j].uMax, out[j].vMin, out[j].vMax, out[j].anyNan};
        status[j] = finish_rect(e, cols, rows, rect + (size_t)j * 4);
    }
    if (uv) std::memcpy(uv + (size_t)map_start[0] * 2, h + oUv, nPts * 8);
    return EAO_OK;
}

eao_status eao_object_assoc_set_profiling(int32_t on) {
    g_assoc.clock.arm(on != 0);
    return EAO_OK;
}

eao_status eao_object_assoc_last_kernel_ms(float* kernel_ms) {
    EAO_REQUIRE(kernel_ms, "null argument");
    return g_assoc.clock.read(kernel_ms, "no measurement on this thread: eao_object_assoc_set_profiling(1) and a rank-sum call that reaches the device or a rect call come first");
}

}  // extern "C"
