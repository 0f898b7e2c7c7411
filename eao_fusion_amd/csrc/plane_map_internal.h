// plane_map_internal.h -- the host half of eao_plane_map_* (plane_map.hip), free of HIP: the table of the resident boundary clouds (id, offset, count, world
// position per MapPlane), the plan of a compaction, the work list of the distance kernel and upstream's selection loop (reference src/Map.cc:173-203, :264-290)
// in plain C++, which tools/plane_association_walk.cpp walks stand-alone.
//
// Storage: the policy of resident_arena.h over one arena of points, appended to by add and by update_boundary.  The table keeps ADD order, and a candidate
// list of NULL means the live planes in that order.
//
// Deviations from upstream:
//   - adding an id that is live is refused (upstream's ids are unique: MapPlane::nLastId++, src/MapPlane.cc:26);
//   - erasing an unknown id is a no-op (std::set::erase of an absent key, src/Map.cc:150);
//   - a candidate id the table does not hold is refused (upstream holds pointers; there is no such thing as an unknown one).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "resident_arena.h"

namespace eao {
namespace pmap {

constexpr int kMaxRows = 2048;               // EAO_PLANE_MAP_MAX_ROWS: 17 bytes of LDS per row in the distance kernel
constexpr int kMaxPointsPerPlane = 1 << 20;  // EAO_PLANE_MAP_MAX_POINTS
constexpr int kMaxCandidates = 1 << 16;      // EAO_PLANE_MAP_MAX_CANDIDATES
constexpr int64_t kMaxPairs = 1 << 24;       // rows x candidates of one call
constexpr uint64_t kMaxArenaPoints = 1ull << 28;      // 4 GiB of 16-byte points; an offset is 32 bits
constexpr int kChunk = 512;                  // points of one workgroup of the distance kernel: 256 lanes x 2 points
constexpr float kNoDistance = 100.0f;        // PointDistanceFromPlane's initial value, src/Map.cc:219

struct World {
    float world[4];      // mWorldPos
};
using Entry = arena::Entry<World>;      // one plane: points begin .. begin + count - 1 of the arena

struct Table : arena::Table<World> {
    // "" when a cloud of n points may be stored (for add: under an id that is not live; for update: under one that is)
    std::string check_cloud(uint64_t id, int64_t n, bool add) const {
        if (n < 0) return "n < 0";
        if (n > kMaxPointsPerPlane) return "the cloud has " + std::to_string(n) + " points; at most " + std::to_string(kMaxPointsPerPlane) + " are supported";
        if (add && byId.count(id)) return "plane " + std::to_string(id) + " is already held";
        if (!add && !byId.count(id)) return "plane " + std::to_string(id) + " is not held";
        if (used + (uint64_t)n > kMaxArenaPoints) return "the arena would hold more than " + std::to_string(kMaxArenaPoints) + " points";
        return "";
    }
    uint64_t append(uint64_t id, uint32_t n, const float world[4]) { return arena::Table<World>::append(id, n, World{{world[0], world[1], world[2], world[3]}}); }
    void set_world(uint64_t id, const float world[4]) { std::memcpy(entries[byId.at(id)].world, world, 16); }
};

// one candidate of a query as the kernels read it (32 bytes)
struct Cand {
    uint32_t begin, count;
    uint32_t pad[2];
    float world[4];
};
static_assert(sizeof(Cand) == 32, "a candidate record is 32 bytes");

// The candidate list of a query resolved against the table: candId == nullptr means every live plane in add order (nCand is then
// ignored unless it is 0: the empty list).  Returns "" or
// what is wrong; ids receives the ids in list order.
inline std::string resolve_candidates(const Table& t, int64_t nCand, const uint64_t* candId, std::vector<Cand>& out, std::vector<uint64_t>& ids) {
    out.clear();
    ids.clear();
    auto push = [&](const Entry& e) {
        Cand c{(uint32_t)e.begin, e.count, {0, 0}, {e.world[0], e.world[1], e.world[2], e.world[3]}};
        out.push_back(c);
        ids.push_back(e.id);
    };
    if (!candId) {
        if (nCand == 0) return "";      // (an empty list may come without a pointer)
        for (const Entry& e : t.entries)
            if (e.live) push(e);
        return "";
    }
    for (int64_t j = 0; j < nCand; j++) {
        const Entry* e = t.find(candId[j]);
        if (!e) return "candidate " + std::to_string(j) + " (plane " + std::to_string(candId[j]) + ") is not held";
        push(*e);
    }
    return "";
}

// The grid of the distance kernel: one workgroup per (candidate, chunk of kChunk of its points); a candidate without points still gets one, which writes its
// gate flags.  item = candidate << 12 | chunk would not hold 2^20 points / 512, so two words.
struct Work {
    uint32_t cand, chunk;
};
inline void plan_work(const std::vector<Cand>& cands, std::vector<Work>& work) {
    work.clear();
    for (size_t j = 0; j < cands.size(); j++) {
        const uint32_t chunks = cands[j].count == 0 ? 1u : (cands[j].count + (uint32_t)kChunk - 1) / (uint32_t)kChunk;
        for (uint32_t c = 0; c < chunks; c++) work.push_back(Work{(uint32_t)j, c});
    }
}

// pM = M^T c (Frame::ComputePlaneWorldCoeff, src/Frame.cc:373-379; ScwT * coefficients, src/Map.cc:250-261): a cv::Mat product -- accumulated in double,
// rounded once to float
inline void world_coefficients(const float M[16], const float c[4], float pM[4]) {
    for (int k = 0; k < 4; k++) {
        double s = 0.0;
        for (int j = 0; j < 4; j++) s += (double)M[j * 4 + k] * (double)c[j];
        pM[k] = (float)s;
    }
}

// src/Map.cc:179-187 / :269-276: float, left to right; a NaN fails both comparisons
inline bool gate(const float pM[4], const float pW[4], float angleTh) {
    const float angle = pM[0] * pW[0] + pM[1] * pW[1] + pM[2] * pW[2];
    return angle > angleTh || angle < -angleTh;
}

// Map::PointDistanceFromPlane, src/Map.cc:217-236, over 16-byte points: abs of a float expression; a NaN never wins
inline float point_distance(const float pM[4], const float* xyzw, uint32_t n) {
    float res = kNoDistance;
    for (uint32_t i = 0; i < n; i++) {
        const float* p = xyzw + 4 * (size_t)i;
        float d = pM[0] * p[0] + pM[1] * p[1] + pM[2] * p[2] + pM[3];
        d = std::fabs(d);
        if (d < res) res = d;
    }
    return res;
}

// src/Map.cc:173-203 / :264-290 for one row over its nCand distances and gate flags: strict <, so the first of equal minima wins and a distance equal to the
// threshold does not associate.  Returns the index into the candidate list or -1; ldTh comes back as upstream leaves it.
inline int32_t select(int64_t nCand, const float* dis, const uint8_t* gated, float disTh, float& ldTh) {
    ldTh = disTh;
    int32_t match = -1;
    for (int64_t j = 0; j < nCand; j++) {
        if (gated[j] && dis[j] < ldTh) {
            ldTh = dis[j];
            match = (int32_t)j;
        }
    }
    return match;
}

}  // namespace pmap
}  // namespace eao
