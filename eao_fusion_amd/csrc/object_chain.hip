// object_chain.hip -- the numeric steps of Object_Map::DataAssociateUpdate (reference src/Object.cc:1352-1601) chained in one device call: the point update of
// csrc/object_points.hip, the erase of the bad points (:1003-1024), the cuboid of csrc/object_cuboid.hip and the isolation forest of csrc/iforest.hip over the
// list the cuboid saw.  One upload, one download, one wait; the list a stage leaves is read by the next one from device memory and no count travels to the host
// in between (csrc/object_chain_internal.h holds the host half).
//
//   k_object_points[_match, _finish]   as in eao_object_points_update_batch, through its enqueue functions; the survivors and their positions stay on the device
//   k_object_chain_plan                one workgroup per desc: the survivors whose bad flag is set leave (an ordered compaction by a workgroup scan), the rest is the
//                                      final list and its positions; one lane then writes, from n_final, the ObjDev that k_object_cuboids reads and the ObjDev
//                                      that k_iforest_build and k_iforest_score read (object_runs, n / 2, the integer max_depth, lds_plan, max_nodes).  A desc whose
//                                      point update did not finish gets a cuboid ObjDev with skip set and a forest ObjDev of no points and no trees.
//   k_object_cuboids                   through its enqueue function, over the final positions
//   k_iforest_build, k_iforest_score   through their enqueue functions.  The grids, the dynamic LDS, the node arrays and the id workspace are sized from the bound
//                                      n_map + n_cand; what a tree reads of them follows from n_final.
// The kernels run in stream order; no atomics on floats anywhere: two calls return the same bytes.
#include <cstring>
#include <vector>

#include "common.h"
#include "object_chain_internal.h"

namespace {

using namespace eao::object_chain;

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;

struct PlanBufs {
    const op::PtsDev* descs;
    const ChainDev* chain;
    const eao_object_points_rec* recs;
    const uint8_t *mapBad, *candBad;
    const int32_t* surv;
    const float* survPts;
    int32_t* fin;
    float* finPts;
    oc::ObjDev* cuboidObjs;
    fo::ObjDev* forestObjs;
    int32_t* nFinal;
    unsigned* failed;      // zeroed here, raised by k_iforest_build
};

__global__ __launch_bounds__(kBlock) void k_object_chain_plan(PlanBufs B) {
    __shared__ int sScan[kWaves];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int desc = blockIdx.x;
    const op::PtsDev& D = B.descs[desc];
    const ChainDev& C = B.chain[desc];
    const bool done = B.recs[desc].status == op::kDone;      // (uniform)
    const int nS = done ? B.recs[desc].n_survivors : 0;
    const int32_t* surv = B.surv + 2 * (size_t)D.listStart;
    const float* survPts = B.survPts + 3 * (size_t)D.listStart;
    int32_t* fin = B.fin + 2 * (size_t)D.listStart;
    float* finPts = B.finPts + 3 * (size_t)D.listStart;
    int nFinal = 0;
    for (int k0 = 0; k0 < nS; k0 += kBlock) {      // (uniform)
        const int k = k0 + t;
        int src = 0, idx = 0, keep = 0;
        if (k < nS) {
            src = surv[2 * (size_t)k];
            idx = surv[2 * (size_t)k + 1];
            keep = (src ? B.candBad[D.candStart + idx] : B.mapBad[D.mapStart + idx]) ? 0 : 1;
        }
        int inc = keep;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(inc, d, 64);
            if (lane >= d) inc += o;
        }
        if (lane == 63) sScan[wave] = inc;
        __syncthreads();
        int base = 0, total = 0;
#pragma unroll
        for (int w = 0; w < kWaves; w++) {
            if (w < wave) base += sScan[w];
            total += sScan[w];
        }
        __syncthreads();
        if (keep) {
            const size_t at = (size_t)(nFinal + base + inc - 1);
            fin[2 * at] = src; fin[2 * at + 1] = idx;
            finPts[3 * at] = survPts[3 * (size_t)k]; finPts[3 * at + 1] = survPts[3 * (size_t)k + 1]; finPts[3 * at + 2] = survPts[3 * (size_t)k + 2];
        }
        nFinal += total;
    }
    if (t != 0) return;
    oc::ObjDev O{};
    O.pointStart = D.listStart; O.centroidStart = C.centroidStart;
    O.n = nFinal; O.m = C.m;
    for (int k = 0; k < 9; k++) O.Ryaw[k] = C.Ryaw[k];
    O.skip = done ? 0 : 1;
    for (int k = 0; k < 3; k++) O.prev[k] = C.prev[k];
    B.cuboidObjs[desc] = O;
    const bool runs = done && C.mayRun && (uint32_t)nFinal >= fo::kMinPoints;      // object_runs (:1241-1257) behind what the host decided
    fo::ObjDev F{};
    F.ptStart = (uint32_t)D.listStart;
    F.treeBase = C.treeBase;
    F.nodeBase = C.nodeBase; F.wsBase = C.wsBase;
    if (runs) {
        const uint32_t n = (uint32_t)nFinal, S = n / fo::kSampleDivisor;
        const fo::LdsPlan plan = fo::lds_plan(n, S);
        F.n = n; F.sampleSize = S; F.maxDepth = fo::max_depth_int(S);
        F.treeCount = fo::kTreeCount; F.inLds = plan.inLds ? 1u : 0u; F.idsBytes = (uint32_t)plan.idsBytes;
        F.stride = fo::max_nodes(S);
    }
    B.forestObjs[desc] = F;
    B.nFinal[desc] = nFinal;
    B.failed[desc] = 0u;
}

struct ObjectChainCtx : eao::ThreadStream {
    eao::DevBuf<unsigned char> dev;
    eao::DevBuf<fo::NodeDev> nodes;
    eao::DevBuf<unsigned short> ws;
    eao::DevBuf<double> cDev;           // CalculateC of 0 .. cHost.size() - 1: one table for every object, grown on demand
    std::vector<double> cHost;
    size_t cOnDevice = 0;               // entries of cHost that a finished upload has put into cDev
    eao::PinBuf<hipHostMallocDefault> host;
    eao::KernelClock<kKernels> clock;
};
thread_local ObjectChainCtx g_chain;

// the table of CalculateC up to `sample` on the device (a log per entry: computed once per thread, not once per call).  cOnDevice counts the entries a
// finished upload has put there: a call that fails on the way leaves it at zero and the next call uploads again.  The copy runs on the thread's own stream,
// which is empty between calls, and is waited for here.
eao_status c_table(ObjectChainCtx& ctx, uint32_t sample) {
    if (ctx.cOnDevice > (size_t)sample) return EAO_OK;
    size_t want = 1024;
    while (want <= (size_t)sample) want *= 2;
    ctx.cOnDevice = 0;
    for (size_t s = ctx.cHost.size(); s < want; s++) ctx.cHost.push_back(fo::c_of((uint32_t)s));
    const eao_status st = ctx.cDev.reserve(want);
    if (st) return st;
    EAO_HIP(hipMemcpyAsync(ctx.cDev.p, ctx.cHost.data(), want * 8, hipMemcpyHostToDevice, ctx.stream));
    EAO_HIP(hipStreamSynchronize(ctx.stream));
    ctx.cOnDevice = want;
    return EAO_OK;
}

}  // namespace

extern "C" {

eao_status eao_object_update_chain_batch(int32_t n, const eao_object_chain_desc* descs, const eao_object_chain_out* outs) {
    EAO_REQUIRE(n >= 0 && n <= op::kMaxDescs, "n outside 0 .. %d", op::kMaxDescs);
    EAO_REQUIRE(n == 0 || (descs && outs), "null argument");
    int64_t nMap = 0, nCand = 0, nCen = 0, maxCand = 0;
    bool split = false;
    for (int32_t k = 0; k < n; k++) {
        const eao_object_points_desc& P = descs[k].points;
        EAO_REQUIRE(P.n_map >= 0 && P.n_cand >= 0 && descs[k].n_centroids >= 0, "desc %d: a negative count", k);
        nMap += P.n_map;
        nCand += P.n_cand;
        nCen += descs[k].n_centroids;
        EAO_REQUIRE(nMap + nCand + nCen <= op::kMaxBatchPoints, "more than 2^27 points and centroids in one call: split it");
        maxCand = P.n_cand > maxCand ? P.n_cand : maxCand;
        split = split || op::launch_is_split(P.n_map, P.n_cand);
    }
    for (int32_t k = 0; k < n; k++) {
        const char* why = desc_refusal(descs[k]);
        EAO_REQUIRE(!why, "desc %d: %s", k, why);
        why = out_refusal(descs[k], outs[k]);
        EAO_REQUIRE(!why, "desc %d: %s", k, why);
    }
    if (n == 0) return EAO_OK;

    ObjectChainCtx& ctx = g_chain;
    eao_status st = ctx.ready(eao::StreamClass::Latency);
    if (st) return st;
    const size_t N = (size_t)n, nM = (size_t)nMap, nC = (size_t)nCand, nL = nM + nC;
    std::vector<ChainDev> chain(N, ChainDev{});
    Sizes Z;
    int64_t cen = 0;
    for (int32_t k = 0; k < n; k++) {
        ChainDev& C = chain[(size_t)k];
        C.centroidStart = cen;
        C.m = descs[k].n_centroids;
        std::memcpy(C.Ryaw, descs[k].Ryaw, sizeof(C.Ryaw));
        std::memcpy(C.prev, descs[k].prev_cuboid_center, sizeof(C.prev));
        size_desc(descs[k], C, Z);
        cen += descs[k].n_centroids;
    }
    const bool forests = Z.trees > 0;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t at = off; off = eao::align256(off + bytes); return at; };
    const size_t oDesc = take(N * sizeof(op::PtsDev)), oChain = take(N * sizeof(ChainDev)), oMapPts = take(nM * 12), oMapCount = take(nM * 4), oCandPts = take(nC * 12),
                 oCandCount = take(nC * 4), oMapBad = take(nM), oCandBad = take(nC), oCen = take((size_t)nCen * 12), oTreeObj = take(Z.trees * 4), oSeed = take(Z.trees * 4),
                 inEnd = off;
    const size_t oFirst = take(nC * 4), oRank = take(nC * 4), oApp = take(nC * 4), oSurvPts = take(nL * 12), oFinPts = take(nL * 12),
                 oCubObj = take(N * sizeof(oc::ObjDev)), oForObj = take(N * sizeof(fo::ObjDev)), oNodeCnt = take(Z.trees * 4);
    const size_t oGate = take(nC), oTarget = take(nC * 4), oCount = take(nC * 4), oList = take(nL * 8), oErased = take(nL), oSurv = take(nL * 8),
                 oRec = take(N * sizeof(eao_object_points_rec)), oFin = take(nL * 8), oNFinal = take(N * 4), oFailed = take(N * 4), oCubRec = take(N * sizeof(eao_object_cuboid_rec)),
                 oTot = take(nL * 8), end = off;
    if ((st = ctx.dev.reserve(end))) return st;
    if ((st = ctx.host.reserve(end))) return st;
    if (forests) {
        if ((st = ctx.nodes.reserve(Z.nodes))) return st;
        if ((st = ctx.ws.reserve(Z.ws > 0 ? Z.ws : 1))) return st;
        if ((st = c_table(ctx, Z.maxSample))) return st;
    }
    unsigned char *d = ctx.dev.p, *h = ctx.host.p;
    op::PtsDev* hd = (op::PtsDev*)(h + oDesc);
    int64_t m = 0, c = 0;
    for (int32_t k = 0; k < n; k++) {
        const eao_object_chain_desc& D = descs[k];
        const eao_object_points_desc& P = D.points;
        op::PtsDev O{};
        O.d = P;
        O.d.map_points = O.d.cand_points = nullptr;
        O.d.map_count = O.d.cand_count = nullptr;
        O.d.survivors = nullptr;
        O.mapStart = m; O.candStart = c; O.listStart = m + c;
        hd[k] = O;
        if (P.n_map > 0) {
            std::memcpy(h + oMapPts + (size_t)m * 12, P.map_points, (size_t)P.n_map * 12);
            aliased_counts(D, (int32_t*)(h + oMapCount) + m);
            std::memcpy(h + oMapBad + (size_t)m, D.map_bad, (size_t)P.n_map);
        }
        if (P.n_cand > 0) {
            std::memcpy(h + oCandPts + (size_t)c * 12, P.cand_points, (size_t)P.n_cand * 12);
            std::memcpy(h + oCandCount + (size_t)c * 4, P.cand_count, (size_t)P.n_cand * 4);
            std::memcpy(h + oCandBad + (size_t)c, D.cand_bad, (size_t)P.n_cand);
        }
        if (D.n_centroids > 0) std::memcpy(h + oCen + (size_t)chain[(size_t)k].centroidStart * 12, D.centroids, (size_t)D.n_centroids * 12);
        if (chain[(size_t)k].mayRun) {
            uint32_t* to = (uint32_t*)(h + oTreeObj) + chain[(size_t)k].treeBase;
            for (uint32_t t = 0; t < fo::kTreeCount; t++) to[t] = (uint32_t)k;
            fo::tree_seeds(fo::kSeed, fo::kTreeCount, (uint32_t*)(h + oSeed) + chain[(size_t)k].treeBase);
        }
        m += P.n_map;
        c += P.n_cand;
    }
    std::memcpy(h + oChain, chain.data(), N * sizeof(ChainDev));
    op::Bufs B;
    B.descs = (const op::PtsDev*)(d + oDesc);
    B.mapPts = (const float*)(d + oMapPts); B.mapCount = (const int32_t*)(d + oMapCount);
    B.candPts = (const float*)(d + oCandPts); B.candCount = (const int32_t*)(d + oCandCount);
    B.first = (int32_t*)(d + oFirst); B.rank = (int32_t*)(d + oRank); B.app = (int32_t*)(d + oApp);
    B.gate = d + oGate; B.target = (int32_t*)(d + oTarget); B.count = (int32_t*)(d + oCount);
    B.list = (int32_t*)(d + oList); B.erased = d + oErased; B.surv = (int32_t*)(d + oSurv); B.survPts = (float*)(d + oSurvPts);
    B.recs = (eao_object_points_rec*)(d + oRec);
    PlanBufs Q;
    Q.descs = B.descs; Q.chain = (const ChainDev*)(d + oChain); Q.recs = B.recs;
    Q.mapBad = d + oMapBad; Q.candBad = d + oCandBad;
    Q.surv = B.surv; Q.survPts = B.survPts;
    Q.fin = (int32_t*)(d + oFin); Q.finPts = (float*)(d + oFinPts);
    Q.cuboidObjs = (oc::ObjDev*)(d + oCubObj); Q.forestObjs = (fo::ObjDev*)(d + oForObj);
    Q.nFinal = (int32_t*)(d + oNFinal); Q.failed = (unsigned*)(d + oFailed);

    eao::Drain drain(ctx.stream);
    EAO_HIP(hipMemcpyAsync(d, h, inEnd, hipMemcpyHostToDevice, ctx.stream));
    if (split) {
        ctx.clock.mark(0, ctx.stream);
        EAO_HIP(op::enqueue_match(ctx.stream, B, (unsigned)N, maxCand));
    }
    ctx.clock.mark(1, ctx.stream);
    EAO_HIP(op::enqueue_finish(ctx.stream, B, (unsigned)N, !split));
    ctx.clock.mark(2, ctx.stream);
    hipLaunchKernelGGL(k_object_chain_plan, dim3((unsigned)N), dim3(kBlock), 0, ctx.stream, Q);
    EAO_HIP(hipGetLastError());
    ctx.clock.mark(3, ctx.stream);
    EAO_HIP(oc::enqueue_cuboids(ctx.stream, Q.cuboidObjs, Q.finPts, (const float*)(d + oCen), (eao_object_cuboid_rec*)(d + oCubRec), (unsigned)N));
    ctx.clock.mark(4, ctx.stream);
    if (forests) {
        EAO_HIP(fo::enqueue_build(ctx.stream, Q.forestObjs, (const unsigned*)(d + oTreeObj), (const unsigned*)(d + oSeed), Q.finPts, ctx.nodes.p, (unsigned*)(d + oNodeCnt),
                                  Q.failed, ctx.ws.p, nullptr, (unsigned)Z.trees, Z.dynLds));
        ctx.clock.mark(5, ctx.stream);
        EAO_HIP(fo::enqueue_score(ctx.stream, Q.forestObjs, Q.finPts, ctx.nodes.p, ctx.cDev.p, Q.failed, (double*)(d + oTot), Z.maxBound,
                                  (unsigned)N));
        ctx.clock.mark(6, ctx.stream);
    }
    EAO_HIP(hipMemcpyAsync(h + oGate, d + oGate, end - oGate, hipMemcpyDeviceToHost, ctx.stream));
    EAO_HIP(drain.wait(eao::Drain::Latency));
    ctx.clock.collect();

    const eao_object_points_rec* recs = (const eao_object_points_rec*)(h + oRec);
    const eao_object_cuboid_rec* cubs = (const eao_object_cuboid_rec*)(h + oCubRec);
    const int32_t* nFinal = (const int32_t*)(h + oNFinal);
    const uint32_t* failed = (const uint32_t*)(h + oFailed);
    m = c = 0;
    for (int32_t k = 0; k < n; k++) {
        const eao_object_chain_desc& D = descs[k];
        const eao_object_chain_out& O = outs[k];
        const eao_object_points_rec& r = recs[k];
        std::memcpy(O.points.rec, &r, sizeof(r));
        if (r.status == op::kDone) {
            const size_t C = (size_t)D.points.n_cand, at = (size_t)(m + c);
            if (C > 0) {
                std::memcpy(O.points.gate, h + oGate + (size_t)c, C);
                std::memcpy(O.points.target, h + oTarget + (size_t)c * 4, C * 4);
                std::memcpy(O.points.count, h + oCount + (size_t)c * 4, C * 4);
            }
            if (r.n_list > 0) {
                std::memcpy(O.points.list, h + oList + at * 8, (size_t)r.n_list * 8);
                std::memcpy(O.points.erased, h + oErased + at, (size_t)r.n_list);
            }
            if (r.n_survivors > 0) std::memcpy(O.points.survivors, h + oSurv + at * 8, (size_t)r.n_survivors * 8);
            const ChainWord W{nFinal[k], chain[(size_t)k].mayRun ? failed[k] : 0u};
            if (W.nFinal > 0) std::memcpy(O.final, h + oFin + at * 8, (size_t)W.nFinal * 8);
            std::memcpy(O.cuboid, cubs + k, sizeof(eao_object_cuboid_rec));
            const uint32_t S = (uint32_t)W.nFinal / fo::kSampleDivisor;
            finish_forest(D, W, (const double*)(h + oTot) + at, S < ctx.cHost.size() ? ctx.cHost[S] : fo::c_of(S), O.forest_flags, O.scores, *O.rec);
        }
        m += D.points.n_map;
        c += D.points.n_cand;
    }
    return EAO_OK;
}

eao_status eao_object_update_chain(const eao_object_chain_desc* desc, const eao_object_chain_out* out) {
    EAO_REQUIRE(desc && out, "null argument");
    return eao_object_update_chain_batch(1, desc, out);
}

eao_status eao_object_chain_set_profiling(int32_t on) {
    g_chain.clock.arm(on != 0);
    return EAO_OK;
}

eao_status eao_object_chain_last_kernel_ms(float* kernel_ms) {
    EAO_REQUIRE(kernel_ms, "null argument");
    return g_chain.clock.read(kernel_ms, "no measurement on this thread: eao_object_chain_set_profiling(1) and a call that reaches the device come first");
}

}  // extern "C"
