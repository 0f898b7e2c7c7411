// object_points.hip -- the update of a map object's point list on the device: the change gate, the append and the erase of Object_Map::DataAssociateUpdate
// (reference src/Object.cc:1364-1436, :1460-1535, :1538-1589), the append of Object_Map::MergeTwoMapObjs (:1766-1821) and the erases of BigToSmall (:2070-2087)
// and DivideEquallyTwoObjs (:2096-2120).  Bit for bit what upstream's loops compute (csrc/object_points_internal.h holds the literal form and the scalar rules
// both sides share).
//
// Upstream compares candidate j with a list that grows while it walks.  Equality of finite floats is transitive and equal positions share their gate, so the walk
// is a pure function of positions: j is new exactly when no list entry and no earlier candidate equals it, and its target is otherwise the first of those in the
// order (list entries, then candidates).  That is one all-pairs compare, an ordered compaction and an ordered sum:
//
//   match    a workgroup takes kCandBlock candidates.  One thread per candidate decides its gate; then the positions [list entries, earlier candidates] go
//            through LDS in tiles of kTile, each wavefront owns every sixteenth candidate and its 64 lanes compare 64 tile positions at a time, kSteps steps
//            between two looks at the ballots: the first set bit of the ballot of the first step with a hit is the smallest position (a wave-wide minimum
//            without a reduction).  first[j] = that position.
//   finish   one workgroup per desc: the change gate (all lanes project, the extrema are merged across the lanes, one lane decides), the new candidates' ranks by
//            a workgroup scan, target / count / list, the ordered float sum of the appended positions in chunks of kChunk through LDS (lanes 0-2, one coordinate
//            each), the erase rule per list position, the survivors' ranks by the same scan, and the ordered float subtractions of the erased positions (a kept
//            position contributes +0.0f: x - +0.0f is x for every float).
//
//   k_object_points        one workgroup per desc does both, the change gate first (a rejected desc stops there)
//   k_object_points_match  } the same two steps as two launches when a desc's compare exceeds kSplitPairs pairs: the match spread over
//   k_object_points_finish } ceil(n_cand / kCandBlock) workgroups per desc
// No atomics: two calls return the same bytes.
#include <cstring>
#include <vector>

#include "common.h"
#include "object_points_internal.h"

namespace {

using namespace eao::object_points;
namespace oa = eao::object_assoc;
namespace oc = eao::object_cuboid;

constexpr int kBlock = 1024;                 // sixteen wavefronts: the compare is a chain of dependent steps per wavefront, so a desc wants many of them
constexpr int kWaves = kBlock / 64;
constexpr int kTile = 1024;                  // positions of the compare that wait in LDS
constexpr int kCandBlock = 256;              // candidates of one match step
constexpr int kSteps = 4;                    // compare steps of 64 positions between two ballots' tests
constexpr int kChunk = 1024;                 // appended positions that wait in LDS for the ordered adds
constexpr int64_t kSplitPairs = (int64_t)1 << 22;      // compares of one desc above which the call runs as two launches
constexpr int kNone = 0x7fffffff;            // first[j] of a candidate that equals nothing in front of it
constexpr int kGatedOut = -2;                // first[j] of a candidate its gate skips

static_assert(sizeof(eao_object_points_rec) == 80, "record layout");
static_assert(kBlock <= kChunk && kCandBlock <= kBlock, "a step of the erase waits in the chunk's LDS; one thread per candidate of a block");
constexpr int kRecWords = sizeof(eao_object_points_rec) / 4;

struct Shared {
    float tile[3][kTile];
    float sum[3][kChunk];
    int first[kCandBlock];
    int scan[kWaves];
    Extent ext[kWaves];
    Pose inv;
    eao_object_points_rec rec;
};

// the exclusive prefix of v over the workgroup, and the total (two barriers)
__device__ __forceinline__ int block_scan(int v, int* sScan, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    if (lane == 63) sScan[wave] = inc;
    __syncthreads();
    int base = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < kWaves; w++) {
        if (w < wave) base += sScan[w];
        total += sScan[w];
    }
    __syncthreads();
    return base + inc - v;
}

__device__ __forceinline__ void set_inverse(const PtsDev& D, Shared& S) {
    if (threadIdx.x == 0) {
        Pose pose;
        pose_of(D.d, pose);
        oc::pose_inverse(pose, S.inv);
    }
    __syncthreads();
}

// gate and first of the candidates [c0, c0 + kCandBlock)
__device__ void match_block(const PtsDev& D, const Bufs& B, int c0, Shared& S) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int M = D.d.n_map, C = D.d.n_cand;
    const int c1 = C - c0 < kCandBlock ? C : c0 + kCandBlock;
    const float* P = B.mapPts + 3 * (size_t)D.mapStart;
    const float* Q = B.candPts + 3 * (size_t)D.candStart;
    for (int j = c0 + t; j < c1; j += kBlock) {
        const float q[3] = {Q[3 * (size_t)j], Q[3 * (size_t)j + 1], Q[3 * (size_t)j + 2]};
        const bool g = D.d.gate != kGateNone && gate_of(D.d, S.inv, q);
        B.gate[D.candStart + j] = g ? 1 : 0;
        S.first[j - c0] = g ? kNone : kGatedOut;
    }
    __syncthreads();
    const int64_t span = (int64_t)M + c1 - 1;      // candidate j reads the positions below M + j
    for (int64_t p0 = 0; p0 < span; p0 += kTile) {      // (uniform)
        const int len = span - p0 < kTile ? (int)(span - p0) : kTile;
        for (int k = t; k < len; k += kBlock) {
            const int64_t pos = p0 + k;
            const float* src = pos < M ? P + 3 * (size_t)pos : Q + 3 * (size_t)(pos - M);
            S.tile[0][k] = src[0]; S.tile[1][k] = src[1]; S.tile[2][k] = src[2];
        }
        __syncthreads();
        for (int j = c0 + wave; j < c1; j += kWaves) {      // (uniform within the wavefront)
            if (S.first[j - c0] != kNone) continue;         // gated out, or found in an earlier tile
            const int64_t room = (int64_t)M + j - p0;
            const int lim = room < len ? (int)room : len;
            if (lim <= 0) continue;
            const float q[3] = {Q[3 * (size_t)j], Q[3 * (size_t)j + 1], Q[3 * (size_t)j + 2]};
            for (int k0 = 0; k0 < lim; k0 += 64 * kSteps) {      // kSteps independent steps, then one question whether to stop
                unsigned long long mask[kSteps];
#pragma unroll
                for (int u = 0; u < kSteps; u++) {
                    const int k = k0 + 64 * u + lane;
                    const bool hit = k < lim && S.tile[0][k] == q[0] && S.tile[1][k] == q[1] && S.tile[2][k] == q[2];
                    mask[u] = __ballot(hit);
                }
                int at = -1;
#pragma unroll
                for (int u = kSteps - 1; u >= 0; u--)
                    if (mask[u]) at = k0 + 64 * u + (__ffsll((long long)mask[u]) - 1);      // the lowest step with a hit wins
                if (at >= 0) {
                    if (lane == 0) S.first[j - c0] = (int)p0 + at;
                    break;
                }
            }
        }
        __syncthreads();
    }
    for (int j = c0 + t; j < c1; j += kBlock) B.first[D.candStart + j] = S.first[j - c0];
    __syncthreads();
}

__device__ __forceinline__ void store_record(const Bufs& B, int desc, const Shared& S) {
    __syncthreads();
    for (int k = threadIdx.x; k < kRecWords; k += kBlock) ((uint32_t*)(B.recs + desc))[k] = ((const uint32_t*)&S.rec)[k];
}

// stage 1; the status is in S.rec for every thread afterwards
__device__ void change_gate(const PtsDev& D, const Bufs& B, Shared& S) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    for (int k = t; k < kRecWords; k += kBlock) ((uint32_t*)&S.rec)[k] = 0u;
    __syncthreads();
    if (!D.d.change_gate) {      // (uniform)
        if (t == 0) S.rec.status = kDone;
        __syncthreads();
        return;
    }
    const int64_t M = D.d.n_map, C = D.d.n_cand;
    const float* P = B.mapPts + 3 * (size_t)D.mapStart;
    const float* Q = B.candPts + 3 * (size_t)D.candStart;
    Extent e;
    oa::extent_init(e);
    for (int64_t i = t; i < C + M; i += kBlock) {
        const float* X = i < C ? Q + 3 * (size_t)i : P + 3 * (size_t)(i - C);
        const float x[3] = {X[0], X[1], X[2]};
        float u, v;
        project(D.d, x, &u, &v);
        oa::extent_add(e, u, v);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        Extent o;
        o.uMin = __shfl_xor(e.uMin, d, 64); o.uMax = __shfl_xor(e.uMax, d, 64);
        o.vMin = __shfl_xor(e.vMin, d, 64); o.vMax = __shfl_xor(e.vMax, d, 64);
        o.anyNan = __shfl_xor(e.anyNan, d, 64);
        extent_merge(e, o);
    }
    if (lane == 0) S.ext[wave] = e;
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < kWaves; w++) extent_merge(e, S.ext[w]);
        change_verdict(D.d, e, C + M, S.rec);
        if (S.rec.status == kRejected)
            for (int a = 0; a < 3; a++) S.rec.sum_pos_appended[a] = S.rec.sum_pos[a] = D.d.sum_pos[a];
    }
    __syncthreads();
}

// everything behind first[]: stage 2's ordered parts and stage 3
__device__ void finish(const PtsDev& D, const Bufs& B, int desc, Shared& S) {
    const int t = threadIdx.x;
    const int M = D.d.n_map, C = D.d.n_cand;
    const float* P = B.mapPts + 3 * (size_t)D.mapStart;
    const float* Q = B.candPts + 3 * (size_t)D.candStart;
    const int32_t* first = B.first + D.candStart;
    int32_t* rank = B.rank + D.candStart;
    int32_t* app = B.app + D.candStart;

    // the new candidates in order
    int nNew = 0, nGated = 0;
    for (int c0 = 0; c0 < C; c0 += kBlock) {      // (uniform)
        const int j = c0 + t;
        const int f = j < C ? first[j] : kGatedOut;
        const int isNew = f == kNone ? 1 : 0;
        int total;
        const int ex = block_scan(isNew, S.scan, total);
        if (j < C) rank[j] = isNew ? nNew + ex : -1;
        if (isNew) app[nNew + ex] = j;
        nNew += total;
        nGated += __syncthreads_count(f != kGatedOut);
    }
    __syncthreads();      // rank and app are read by other threads below
    for (int j = t; j < C; j += kBlock) {
        const int f = first[j];
        B.target[D.candStart + j] = (f == kNone || f == kGatedOut) ? -1 : (f < M ? f : M + rank[f - M]);
        B.count[D.candStart + j] = B.candCount[D.candStart + j] + (f != kGatedOut ? 1 : 0);
    }
    const int nL = M + nNew;      // (M + C <= 2^27)
    int32_t* list = B.list + 2 * (size_t)D.listStart;
    for (int k = t; k < nL; k += kBlock) {
        list[2 * (size_t)k] = k < M ? 0 : 1;
        list[2 * (size_t)k + 1] = k < M ? k : app[k - M];
    }
    // mSumPointsPos += x3d, in append order (:1532)
    float acc = t < 3 ? D.d.sum_pos[t] : 0.0f;
    for (int r0 = 0; r0 < nNew; r0 += kChunk) {      // (uniform)
        const int len = nNew - r0 < kChunk ? nNew - r0 : kChunk;
        for (int r = t; r < len; r += kBlock) {
            const float* q = Q + 3 * (size_t)app[r0 + r];
            S.sum[0][r] = q[0]; S.sum[1][r] = q[1]; S.sum[2][r] = q[2];
        }
        __syncthreads();
        if (t < 3)
            for (int r = 0; r < len; r++) acc = acc + S.sum[t][r];
        __syncthreads();
    }
    if (t < 3) S.rec.sum_pos_appended[t] = acc;

    // stage 3 over the list positions, kBlock at a time
    uint8_t* erased = B.erased + D.listStart;
    int32_t* surv = B.surv + 2 * (size_t)D.listStart;
    float* survPts = B.survPts + 3 * (size_t)D.listStart;
    const bool subtract = D.d.erase == kEraseProjection;
    int nSurv = 0;
    for (int k0 = 0; k0 < nL; k0 += kBlock) {      // (uniform)
        const int k = k0 + t;
        bool er = false;
        float x[3] = {0.0f, 0.0f, 0.0f};
        int src = 0, idx = 0;
        if (k < nL) {
            src = k < M ? 0 : 1;
            idx = k < M ? k : app[k - M];
            const float* X = src ? Q + 3 * (size_t)idx : P + 3 * (size_t)idx;
            x[0] = X[0]; x[1] = X[1]; x[2] = X[2];
            if (D.d.erase != kEraseNone) {
                const int32_t count = D.d.erase != kEraseProjection ? 0 : (src ? B.candCount[D.candStart + idx] + 1 : B.mapCount[D.mapStart + idx]);
                er = erase_entry(D.d, x, count);
            }
            erased[k] = er ? 1 : 0;
        }
        int total;
        const int ex = block_scan((k < nL && !er) ? 1 : 0, S.scan, total);
        if (k < nL && !er) {
            const size_t at = (size_t)(nSurv + ex);
            surv[2 * at] = src; surv[2 * at + 1] = idx;
            survPts[3 * at] = x[0]; survPts[3 * at + 1] = x[1]; survPts[3 * at + 2] = x[2];
        }
        nSurv += total;
        if (subtract && __syncthreads_or(er ? 1 : 0)) {      // (uniform) mSumPointsPos -= PointPosWorld, in list order (:1577)
            S.sum[0][t] = er ? x[0] : 0.0f; S.sum[1][t] = er ? x[1] : 0.0f; S.sum[2][t] = er ? x[2] : 0.0f;
            __syncthreads();
            const int len = nL - k0 < kBlock ? nL - k0 : kBlock;
            if (t < 3)
                for (int r = 0; r < len; r++) acc = acc - S.sum[t][r];
            __syncthreads();
        }
    }
    if (t < 3) S.rec.sum_pos[t] = acc;
    if (t == 0) {
        S.rec.n_gated = nGated;
        S.rec.n_appended = nNew;
        S.rec.n_list = nL;
        S.rec.n_erased = nL - nSurv;
        S.rec.n_survivors = nSurv;
    }
    store_record(B, desc, S);
}

__global__ __launch_bounds__(kBlock) void k_object_points(Bufs B) {
    __shared__ Shared S;
    const PtsDev& D = B.descs[blockIdx.x];
    change_gate(D, B, S);
    if (S.rec.status != kDone) {      // (uniform)
        store_record(B, blockIdx.x, S);
        return;
    }
    set_inverse(D, S);
    for (int c0 = 0; c0 < D.d.n_cand; c0 += kCandBlock) match_block(D, B, c0, S);
    finish(D, B, blockIdx.x, S);
}

__global__ __launch_bounds__(kBlock) void k_object_points_match(Bufs B) {
    __shared__ Shared S;
    const PtsDev& D = B.descs[blockIdx.y];
    const int64_t c0 = (int64_t)blockIdx.x * kCandBlock;
    if (c0 >= D.d.n_cand) return;      // (uniform)
    set_inverse(D, S);
    match_block(D, B, (int)c0, S);
}

__global__ __launch_bounds__(kBlock) void k_object_points_finish(Bufs B) {
    __shared__ Shared S;
    const PtsDev& D = B.descs[blockIdx.x];
    change_gate(D, B, S);
    if (S.rec.status != kDone) {      // (uniform)
        store_record(B, blockIdx.x, S);
        return;
    }
    finish(D, B, blockIdx.x, S);
}

struct ObjectPointsCtx : eao::ThreadStream {
    eao::DevBuf<unsigned char> dev;
    eao::PinBuf<hipHostMallocDefault> host;
    eao::KernelClock<2> clock;      // k_object_points_match, k_object_points (or k_object_points_finish) of the last call that reached the device
};
thread_local ObjectPointsCtx g_op;

}  // namespace

namespace eao {
namespace object_points {

bool launch_is_split(int64_t n_map, int64_t n_cand) { return n_cand * (n_map + n_cand) > kSplitPairs; }

hipError_t enqueue_match(hipStream_t stream, const Bufs& B, unsigned n_desc, int64_t max_cand) {
    const unsigned blocks = (unsigned)((max_cand + kCandBlock - 1) / kCandBlock);
    hipLaunchKernelGGL(k_object_points_match, dim3(blocks, n_desc), dim3(kBlock), 0, stream, B);
    return hipGetLastError();
}

hipError_t enqueue_finish(hipStream_t stream, const Bufs& B, unsigned n_desc, bool fused) {
    if (fused) hipLaunchKernelGGL(k_object_points, dim3(n_desc), dim3(kBlock), 0, stream, B);
    else hipLaunchKernelGGL(k_object_points_finish, dim3(n_desc), dim3(kBlock), 0, stream, B);
    return hipGetLastError();
}

}  // namespace object_points
}  // namespace eao

extern "C" {

eao_status eao_object_points_update_batch(int32_t n, const eao_object_points_desc* descs, const eao_object_points_out* outs) {
    EAO_REQUIRE(n >= 0 && n <= kMaxDescs, "n outside 0 .. %d", kMaxDescs);
    EAO_REQUIRE(n == 0 || (descs && outs), "null argument");
    int64_t nMap = 0, nCand = 0, maxCand = 0;
    bool split = false;
    for (int32_t k = 0; k < n; k++) {
        EAO_REQUIRE(descs[k].n_map >= 0 && descs[k].n_cand >= 0, "desc %d: a negative count", k);
        nMap += descs[k].n_map;
        nCand += descs[k].n_cand;
        EAO_REQUIRE(nMap + nCand <= kMaxBatchPoints, "more than 2^27 points in one call: split it");
        maxCand = descs[k].n_cand > maxCand ? descs[k].n_cand : maxCand;
        split = split || launch_is_split(descs[k].n_map, descs[k].n_cand);
    }
    for (int32_t k = 0; k < n; k++) {
        const char* why = desc_refusal(descs[k]);
        EAO_REQUIRE(!why, "desc %d: %s", k, why);
        why = out_refusal(descs[k], outs[k]);
        EAO_REQUIRE(!why, "desc %d: %s", k, why);
    }
    if (n == 0) return EAO_OK;

    ObjectPointsCtx& ctx = g_op;
    eao_status st = ctx.ready(eao::StreamClass::Latency);
    if (st) return st;
    const size_t N = (size_t)n, nM = (size_t)nMap, nC = (size_t)nCand, nL = nM + nC;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t at = off; off = eao::align256(off + bytes); return at; };
    const size_t oDesc = take(N * sizeof(PtsDev)), oMapPts = take(nM * 12), oMapCount = take(nM * 4), oCandPts = take(nC * 12), oCandCount = take(nC * 4), inEnd = off;
    const size_t oFirst = take(nC * 4), oRank = take(nC * 4), oApp = take(nC * 4);
    const size_t oGate = take(nC), oTarget = take(nC * 4), oCount = take(nC * 4), oList = take(nL * 8), oErased = take(nL), oSurv = take(nL * 8), oSurvPts = take(nL * 12),
                 oRec = take(N * sizeof(eao_object_points_rec)), end = off;
    if ((st = ctx.dev.reserve(end))) return st;
    if ((st = ctx.host.reserve(end))) return st;
    unsigned char *d = ctx.dev.p, *h = ctx.host.p;
    PtsDev* hd = (PtsDev*)(h + oDesc);
    int64_t m = 0, c = 0;
    for (int32_t k = 0; k < n; k++) {
        const eao_object_points_desc& D = descs[k];
        PtsDev O{};
        O.d = D;
        O.d.map_points = O.d.cand_points = nullptr;
        O.d.map_count = O.d.cand_count = nullptr;
        O.d.survivors = nullptr;
        O.mapStart = m; O.candStart = c; O.listStart = m + c;
        hd[k] = O;
        if (D.n_map > 0) {
            std::memcpy(h + oMapPts + (size_t)m * 12, D.map_points, (size_t)D.n_map * 12);
            if (D.map_count) std::memcpy(h + oMapCount + (size_t)m * 4, D.map_count, (size_t)D.n_map * 4);
            else std::memset(h + oMapCount + (size_t)m * 4, 0, (size_t)D.n_map * 4);
        }
        if (D.n_cand > 0) {
            std::memcpy(h + oCandPts + (size_t)c * 12, D.cand_points, (size_t)D.n_cand * 12);
            std::memcpy(h + oCandCount + (size_t)c * 4, D.cand_count, (size_t)D.n_cand * 4);
        }
        m += D.n_map;
        c += D.n_cand;
    }
    Bufs B;
    B.descs = (const PtsDev*)(d + oDesc);
    B.mapPts = (const float*)(d + oMapPts); B.mapCount = (const int32_t*)(d + oMapCount);
    B.candPts = (const float*)(d + oCandPts); B.candCount = (const int32_t*)(d + oCandCount);
    B.first = (int32_t*)(d + oFirst); B.rank = (int32_t*)(d + oRank); B.app = (int32_t*)(d + oApp);
    B.gate = d + oGate; B.target = (int32_t*)(d + oTarget); B.count = (int32_t*)(d + oCount);
    B.list = (int32_t*)(d + oList); B.erased = d + oErased; B.surv = (int32_t*)(d + oSurv); B.survPts = (float*)(d + oSurvPts);
    B.recs = (eao_object_points_rec*)(d + oRec);

    eao::Drain drain(ctx.stream);
    EAO_HIP(hipMemcpyAsync(d, h, inEnd, hipMemcpyHostToDevice, ctx.stream));
    if (split) {
        ctx.clock.mark(0, ctx.stream);
        EAO_HIP(enqueue_match(ctx.stream, B, (unsigned)N, maxCand));
        ctx.clock.mark(1, ctx.stream);
        EAO_HIP(enqueue_finish(ctx.stream, B, (unsigned)N, false));
    } else {
        ctx.clock.mark(1, ctx.stream);
        EAO_HIP(enqueue_finish(ctx.stream, B, (unsigned)N, true));
    }
    ctx.clock.mark(2, ctx.stream);
    EAO_HIP(hipMemcpyAsync(h + oGate, d + oGate, end - oGate, hipMemcpyDeviceToHost, ctx.stream));
    EAO_HIP(drain.wait(eao::Drain::Latency));
    ctx.clock.collect();

    const eao_object_points_rec* recs = (const eao_object_points_rec*)(h + oRec);
    m = c = 0;
    for (int32_t k = 0; k < n; k++) {
        const eao_object_points_desc& D = descs[k];
        const eao_object_points_out& O = outs[k];
        const eao_object_points_rec& r = recs[k];
        std::memcpy(O.rec, &r, sizeof(r));
        if (r.status == kDone) {
            const size_t C = (size_t)D.n_cand, at = (size_t)(m + c);
            if (C > 0) {
                std::memcpy(O.gate, h + oGate + (size_t)c, C);
                std::memcpy(O.target, h + oTarget + (size_t)c * 4, C * 4);
                std::memcpy(O.count, h + oCount + (size_t)c * 4, C * 4);
            }
            if (r.n_list > 0) {
                std::memcpy(O.list, h + oList + at * 8, (size_t)r.n_list * 8);
                std::memcpy(O.erased, h + oErased + at, (size_t)r.n_list);
            }
            if (r.n_survivors > 0) {
                std::memcpy(O.survivors, h + oSurv + at * 8, (size_t)r.n_survivors * 8);
                if (D.survivors) std::memcpy(D.survivors, h + oSurvPts + at * 12, (size_t)r.n_survivors * 12);
            }
        }
        m += D.n_map;
        c += D.n_cand;
    }
    return EAO_OK;
}

eao_status eao_object_points_update(const eao_object_points_desc* desc, const eao_object_points_out* out) {
    EAO_REQUIRE(desc && out, "null argument");
    return eao_object_points_update_batch(1, desc, out);
}

eao_status eao_object_points_set_profiling(int32_t on) {
    g_op.clock.arm(on != 0);
    return EAO_OK;
}

eao_status eao_object_points_last_kernel_ms(float* kernel_ms) {
    EAO_REQUIRE(kernel_ms, "null argument");
    return g_op.clock.read(kernel_ms, "no measurement on this thread: eao_object_points_set_profiling(1) and a call that reaches the device come first");
}

}  // extern "C"
