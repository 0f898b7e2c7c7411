// object_chain_internal.h -- the host half of eao_object_update_chain_batch (csrc/object_chain.hip): the point update, the erase of the bad points, the cuboid and
// the isolation forest of Object_Map::DataAssociateUpdate (reference src/Object.cc:1352-1601) chained on the device.  HIP-free: the argument checks, the alias
// rule, what is sized from the upper bound n_map + n_cand, the per-desc words the plan kernel reads, and the host finish of the forest through
// iforest_internal.h.  Nothing is transcribed here: the rules are those of object_points_internal.h, object_cuboid_internal.h and iforest_internal.h
// (DESIGN.md section 4s).
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/eao_fusion.h"
#include "iforest_internal.h"
#include "object_cuboid_internal.h"
#include "object_points_internal.h"

namespace eao {
namespace object_chain {

namespace op = eao::object_points;
namespace oc = eao::object_cuboid;
namespace fo = eao::iforest;

constexpr int32_t kForestSkipped = EAO_OBJECT_CHAIN_FOREST_SKIPPED, kForestDone = EAO_OBJECT_CHAIN_FOREST_DONE, kForestFailed = EAO_OBJECT_CHAIN_FOREST_FAILED;
constexpr int kKernels = 6;      // k_object_points_match, k_object_points (or _finish), k_object_chain_plan, k_object_cuboids, k_iforest_build, k_iforest_score

// the upper bound of a desc's final list: the true count is only known on the device
inline int64_t bound_of(const eao_object_chain_desc& D) { return (int64_t)D.points.n_map + D.points.n_cand; }

// whether the forest of a desc can run at all: what the host knows of object_runs (:1241-1257).  The device adds n_final >= kMinPoints.
inline bool may_run(const eao_object_chain_desc& D) { return fo::object_runs(D.bi_forest != 0, D.class_id, (size_t)fo::kMinPoints) && bound_of(D) >= (int64_t)fo::kMinPoints; }

// ---- what the entry points refuse beyond the three entries' own refusals (include/eao_fusion.h); nullptr = accepted
inline const char* desc_refusal(const eao_object_chain_desc& D) {
    if (D.points.n_map < 0 || D.points.n_cand < 0) return "a negative count";
    // (the counts alone decide: no list is read)
    if (may_run(D) && bound_of(D) > (int64_t)fo::kMaxPoints) return "n_map + n_cand above EAO_IFOREST_MAX_POINTS on a desc whose forest may run";
    const char* why = op::desc_refusal(D.points);
    if (why) return why;
    if (D.points.n_map > 0 && !D.map_bad) return "map_bad is NULL";
    if (D.points.n_cand > 0 && !D.cand_bad) return "cand_bad is NULL";
    if (D.cand_alias)
        for (int32_t j = 0; j < D.points.n_cand; j++)
            if (D.cand_alias[j] < -1 || D.cand_alias[j] >= D.points.n_map) return "an alias outside -1 .. n_map - 1";
    eao_object_cuboid_desc c = eao_object_cuboid_desc();      // the cuboid's own checks over what the host owns of its inputs
    c.n_centroids = D.n_centroids;
    c.centroids = D.centroids;
    std::memcpy(c.Ryaw, D.Ryaw, sizeof(c.Ryaw));
    std::memcpy(c.prev_cuboid_center, D.prev_cuboid_center, sizeof(c.prev_cuboid_center));
    if ((why = oc::object_refusal(c))) return why;
    return nullptr;
}

inline const char* out_refusal(const eao_object_chain_desc& D, const eao_object_chain_out& O) {
    const char* why = op::out_refusal(D.points, O.points);
    if (why) return why;
    if (!O.rec || !O.cuboid) return "rec or cuboid is NULL";
    if (bound_of(D) > 0 && !(O.final && O.forest_flags)) return "final or forest_flags is NULL";
    return nullptr;
}

// ---- the alias rule: map_count[k] plus the number of gated-in candidates whose alias is k (:1550-1559).  The gate is the rule the device runs (the same
// function, compiled for both sides); the sum is integers.
inline void aliased_counts(const eao_object_chain_desc& D, int32_t* out) {
    const eao_object_points_desc& P = D.points;
    if (P.map_count) std::memcpy(out, P.map_count, (size_t)P.n_map * 4);
    else std::memset(out, 0, (size_t)P.n_map * 4);
    if (!D.cand_alias || P.gate == op::kGateNone) return;
    op::Pose pose, inv;
    op::pose_of(P, pose);
    oc::pose_inverse(pose, inv);
    for (int32_t j = 0; j < P.n_cand; j++)
        if (D.cand_alias[j] >= 0 && op::gate_of(P, inv, P.cand_points + 3 * (size_t)j)) out[D.cand_alias[j]]++;
}

// ---- what the plan kernel reads per desc beside the points' PtsDev
struct ChainDev {
    int64_t centroidStart;      // in entries of the packed centroids
    uint64_t nodeBase;          // in NodeDev: 50 trees of max_nodes(bound / 2) each
    uint64_t wsBase;            // in uint16: 50 id lists of the bound's plan, where that plan is not in LDS
    int32_t m, mayRun;
    uint32_t treeBase, pad;
    float Ryaw[9];
    int32_t pad2;
    double prev[3];
};
static_assert(sizeof(ChainDev) == 104, "ChainDev layout");

// what the chain brings back per desc beside the records of the three stages
struct ChainWord {
    int32_t nFinal;
    uint32_t failed;            // upstream's Build returned false (include/isolation_forest.h:167)
};

// ---- what is sized from the bound: the trees' node arrays, the id workspace and the dynamic LDS of k_iforest_build
struct Sizes {
    size_t trees = 0, nodes = 0, ws = 0, dynLds = 0;
    uint32_t maxBound = 0, maxSample = 0;
};
inline void size_desc(const eao_object_chain_desc& D, ChainDev& C, Sizes& Z) {
    C.mayRun = may_run(D) ? 1 : 0;
    C.treeBase = (uint32_t)Z.trees;
    C.nodeBase = Z.nodes;
    C.wsBase = Z.ws;
    if (!C.mayRun) return;
    const uint32_t ub = (uint32_t)bound_of(D), S = ub / fo::kSampleDivisor;
    const fo::LdsPlan plan = fo::lds_plan(ub, S);      // bytes grows with n: a shorter list fits wherever the bound does
    Z.trees += fo::kTreeCount;
    Z.nodes += (size_t)fo::kTreeCount * fo::max_nodes(S);
    if (!plan.inLds) Z.ws += (size_t)fo::kTreeCount * (plan.idsBytes / 2);
    const size_t lds = plan.inLds ? plan.bytes : fo::kLdsBudget;      // (a list below the bound may still fit)
    Z.dynLds = lds > Z.dynLds ? lds : Z.dynLds;
    Z.maxBound = ub > Z.maxBound ? ub : Z.maxBound;
    Z.maxSample = S > Z.maxSample ? S : Z.maxSample;
}

// ---- the host finish of the forest (:1302-1347 behind the path lengths), as eao_object_iforest_outliers_batch finishes: flags, scores, the record.
// cOfSample = CalculateC(n_final / 2).
inline void finish_forest(const eao_object_chain_desc& D, const ChainWord& W, const double* totals, double cOfSample, uint8_t* flags, double* scores,
                          eao_object_chain_rec& R) {
    const size_t n = (size_t)W.nFinal;
    R = eao_object_chain_rec();
    R.n_final = W.nFinal;
    if (n > 0) std::memset(flags, 0, n);
    if (scores)
        for (size_t i = 0; i < n; i++) scores[i] = -1.0;
    if (!fo::object_runs(D.bi_forest != 0, D.class_id, n)) {
        R.forest_status = kForestSkipped;
        return;
    }
    if (W.failed) {      // upstream prints "Failed to build Isolation Forest." and returns (:1296-1300)
        R.forest_status = kForestFailed;
        return;
    }
    R.forest_status = kForestDone;
    const double th = fo::object_threshold(D.class_id);
    for (size_t i = 0; i < n; i++) {
        const double s = fo::finish_score(totals[i], fo::kTreeCount, cOfSample);
        if (scores) scores[i] = s;
        if (s > th) {      // :1317
            flags[i] = 1;
            R.removed++;
        }
    }
}

// ---- the three host walks chained (tools/object_chain_walk.cpp): the sanitizer target and the -O3 baseline of tools/bench_object_chain.py.
// plantedFailure hands the finish a failed word where no input is known on which upstream's Build fails.
struct Walk {
    op::Walk points;
    std::vector<int32_t> final;        // (source, index) pairs
    std::vector<float> finalPoints;
    eao_object_cuboid_rec cuboid;
    eao_object_chain_rec rec;
    std::vector<uint8_t> flags;
    std::vector<double> scores;
};

inline void walk_chain(const eao_object_chain_desc& D, Walk& W, bool plantedFailure = false) {
    W = Walk();
    eao_object_points_desc P = D.points;
    std::vector<int32_t> counts((size_t)P.n_map + 1);
    aliased_counts(D, counts.data());
    P.map_count = counts.data();
    op::walk_update(P, W.points);
    if (W.points.rec.status != op::kDone) return;
    // :1003-1024: the erase while iterating
    struct Entry { int32_t source, index; float pos[3]; };
    std::vector<Entry> list;
    for (size_t k = 0; k < (size_t)W.points.rec.n_survivors; k++)
        list.push_back(Entry{W.points.survivors[2 * k], W.points.survivors[2 * k + 1], {W.points.points[3 * k], W.points.points[3 * k + 1], W.points.points[3 * k + 2]}});
    for (std::vector<Entry>::iterator it = list.begin(); it != list.end();) {
        if (it->source ? D.cand_bad[it->index] : D.map_bad[it->index]) it = list.erase(it);
        else ++it;
    }
    for (const Entry& E : list) {
        W.final.push_back(E.source);
        W.final.push_back(E.index);
        for (int a = 0; a < 3; a++) W.finalPoints.push_back(E.pos[a]);
    }
    const size_t n = list.size();
    eao_object_cuboid_desc c = eao_object_cuboid_desc();
    c.n_points = (int32_t)n;
    c.points = W.finalPoints.data();
    c.n_centroids = D.n_centroids;
    c.centroids = D.centroids;
    std::memcpy(c.Ryaw, D.Ryaw, sizeof(c.Ryaw));
    std::memcpy(c.prev_cuboid_center, D.prev_cuboid_center, sizeof(c.prev_cuboid_center));
    oc::walk_object(c, W.cuboid);
    ChainWord word{(int32_t)n, plantedFailure ? 1u : 0u};
    std::vector<double> totals(n + 1, 0.0);
    double cS = 0.0;
    if (fo::object_runs(D.bi_forest != 0, D.class_id, n)) {
        fo::HostForest forest;
        const uint32_t S = (uint32_t)n / fo::kSampleDivisor;
        if (!forest.build(fo::kTreeCount, fo::kSeed, W.finalPoints.data(), (uint32_t)n, S)) word.failed = 1u;
        else
            for (size_t i = 0; i < n; i++) totals[i] = forest.total(W.finalPoints.data() + 3 * i);
        cS = fo::c_of(S);
    }
    W.flags.assign(n + 1, 0);
    W.scores.assign(n + 1, 0.0);
    finish_forest(D, word, totals.data(), cS, W.flags.data(), W.scores.data(), W.rec);
    W.flags.resize(n);
    W.scores.resize(n);
}

}  // namespace object_chain
}  // namespace eao
