// plane_association_walk.cpp -- Map::AssociatePlanesByBoundary / Map::SearchMatchedPlanes as the reference runs them (src/Map.cc:155-292): one host thread, the
// literal loops, over the bookkeeping of eao_fusion_amd/csrc/plane_map_internal.h (the table and capacity rules of resident_arena.h) with a host arena in place of the device's.  Two uses:
//
//   g++ -O3 -march=native -ffp-contract=off -std=c++17 tools/plane_association_walk.cpp -o walk
//   ./walk bench <rows> <planes> <points> <sets> <reps>      the baseline of tools/bench_plane_association.py: microseconds per call, single thread
//
//   g++ -O1 -g -ffp-contract=off -fsanitize=address,undefined ... ; ./walk script [initial arena points] < commands
//       tests/test_plane_map_host_cpu.py: add / update / setw / erase / clear / table / query over an arena that grows and compacts exactly as the library's
//       does (allocations of exactly the capacity, so the sanitizer sees a point out of place), answers printed as bit patterns.
//
// Commands (floats as 8 hex digits of their bit pattern, points already in the world frame):
//   add <id> <w0..w3> <n> <n*3 floats>     update <id> <n> <n*3 floats>     setw <id> <w0..w3>     erase <id>     clear     table
//   query <dis_th> <angle_th> <n_sets> <n_sets*16 floats> <n_sets+1 starts> <rows*4 floats> <n_cand or -1> <ids>
// -ffp-contract=off in both builds: the float expressions are rounded operation by operation, as the library's.
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "../eao_fusion_amd/csrc/plane_map_internal.h"

namespace pmap = eao::pmap;

struct HostMap {
    pmap::Table table;
    std::unique_ptr<float[]> pts;      // 4 floats per point, exactly cap points
    size_t cap = 0, initial = 1 << 13;
    bool verbose = false;

    void reserve(uint64_t need) {
        if (need <= cap) return;
        const size_t c = (size_t)eao::arena::grown_capacity(cap, initial, need, eao::arena::kUnbounded);
        std::unique_ptr<float[]> q(new float[c * 4]);
        if (table.used) std::memcpy(q.get(), pts.get(), (size_t)table.used * 16);
        pts.swap(q);
        cap = c;
        if (verbose) std::printf("grew %zu\n", cap);
    }
    void compact() {
        std::vector<eao::arena::Move> moves;
        const uint64_t live = table.plan_compaction(moves);
        const size_t c = (size_t)eao::arena::compacted_capacity(initial, live, eao::arena::kUnbounded);
        std::unique_ptr<float[]> q(new float[c * 4]);
        for (const eao::arena::Move& m : moves) std::memcpy(q.get() + m.dst * 4, pts.get() + m.src * 4, (size_t)m.count * 16);
        pts.swap(q);
        cap = c;
        table.apply_compaction();
        if (verbose) std::printf("compacted %zu\n", cap);
    }
    void store(uint64_t begin, uint32_t n, const float* xyz) {
        for (uint32_t i = 0; i < n; i++) {
            float* p = pts.get() + (begin + i) * 4;
            p[0] = xyz[3 * i]; p[1] = xyz[3 * i + 1]; p[2] = xyz[3 * i + 2]; p[3] = 0.0f;
        }
    }
    bool add(uint64_t id, const float w[4], uint32_t n, const float* xyz) {
        if (!table.check_cloud(id, n, true).empty()) return false;
        const uint64_t begin = table.used;
        reserve(begin + n);
        store(begin, n, xyz);
        table.append(id, n, w);
        return true;
    }
    bool update(uint64_t id, uint32_t n, const float* xyz) {
        if (!table.check_cloud(id, n, false).empty()) return false;
        const uint64_t begin = table.used;
        reserve(begin + n);
        store(begin, n, xyz);
        table.replace(id, n);
        if (table.wants_compaction()) compact();
        return true;
    }
    void erase(uint64_t id) {
        if (table.erase(id) && table.wants_compaction()) compact();
    }
};

struct Result {
    std::vector<int32_t> match;
    std::vector<float> matchDis, worldCoef, dis;
    std::vector<uint8_t> gated;
};

// src/Map.cc:167-207 / :258-291 over every set: the loops as upstream nests them -- frame plane, candidate, point
static bool associate(const HostMap& hm, int nSets, const float* M, const int32_t* setStart, const float* coef, int64_t nCand, const uint64_t* candId,
                      float disTh, float angleTh, Result& r, bool full) {
    std::vector<pmap::Cand> cands;
    std::vector<uint64_t> ids;
    if (!pmap::resolve_candidates(hm.table, nCand, candId, cands, ids).empty()) return false;
    const size_t nc = cands.size(), rows = (size_t)setStart[nSets];
    r.match.assign(rows, -1);
    r.matchDis.assign(rows, 0.0f);
    r.worldCoef.assign(rows * 4, 0.0f);
    if (full) {
        r.dis.assign(rows * nc, pmap::kNoDistance);
        r.gated.assign(rows * nc, 0);
    }
    for (int s = 0; s < nSets; s++) {
        for (int32_t i = setStart[s]; i < setStart[s + 1]; i++) {
            float pM[4];
            pmap::world_coefficients(M + 16 * s, coef + 4 * i, pM);
            std::memcpy(&r.worldCoef[4 * (size_t)i], pM, 16);
            float ldTh = disTh;
            for (size_t j = 0; j < nc; j++) {
                if (pmap::gate(pM, cands[j].world, angleTh)) {
                    const float dis = pmap::point_distance(pM, hm.pts.get() + (size_t)cands[j].begin * 4, cands[j].count);
                    if (full) {
                        r.gated[(size_t)i * nc + j] = 1;
                        r.dis[(size_t)i * nc + j] = dis;
                    }
                    if (dis < ldTh) {
                        ldTh = dis;
                        r.match[i] = (int32_t)j;
                    }
                }
            }
            r.matchDis[i] = ldTh;
        }
    }
    return true;
}

static float hexf(const std::string& s) {
    const uint32_t u = (uint32_t)std::stoul(s, nullptr, 16);
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}
static uint32_t bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}
static float nextf() {
    std::string s;
    std::cin >> s;
    return hexf(s);
}

static int run_script(size_t initial) {
    HostMap hm;
    hm.initial = initial;
    hm.verbose = true;
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd == "add" || cmd == "update") {
            uint64_t id;
            float w[4] = {0, 0, 0, 0};
            uint32_t n;
            std::cin >> id;
            if (cmd == "add")
                for (float& v : w) v = nextf();
            std::cin >> n;
            std::vector<float> xyz((size_t)n * 3);
            for (float& v : xyz) v = nextf();
            const bool ok = cmd == "add" ? hm.add(id, w, n, xyz.data()) : hm.update(id, n, xyz.data());
            if (!ok) std::printf("refused\n");
        } else if (cmd == "setw") {
            uint64_t id;
            float w[4];
            std::cin >> id;
            for (float& v : w) v = nextf();
            if (hm.table.find(id)) hm.table.set_world(id, w);
            else std::printf("refused\n");
        } else if (cmd == "erase") {
            uint64_t id;
            std::cin >> id;
            hm.erase(id);
        } else if (cmd == "clear") {
            hm.table.clear();
        } else if (cmd == "table") {
            std::printf("table used %llu dead %llu live %d |", (unsigned long long)hm.table.used, (unsigned long long)hm.table.dead, hm.table.nLive);
            for (const pmap::Entry& e : hm.table.entries)
                if (e.live) std::printf(" %llu:%llu:%u", (unsigned long long)e.id, (unsigned long long)e.begin, e.count);
            std::printf("\n");
        } else if (cmd == "query") {
            const float disTh = nextf(), angleTh = nextf();
            int nSets;
            std::cin >> nSets;
            std::vector<float> M((size_t)nSets * 16);
            for (float& v : M) v = nextf();
            std::vector<int32_t> start((size_t)nSets + 1);
            for (int32_t& v : start) std::cin >> v;
            std::vector<float> coef((size_t)start[nSets] * 4);
            for (float& v : coef) v = nextf();
            long long nCand;
            std::cin >> nCand;
            std::vector<uint64_t> ids((size_t)(nCand < 0 ? 0 : nCand));
            for (uint64_t& v : ids) std::cin >> v;
            Result r;
            if (!associate(hm, nSets, M.data(), start.data(), coef.data(), nCand, nCand < 0 ? nullptr : ids.data(), disTh, angleTh, r, true)) {
                std::printf("refused\n");
                continue;
            }
            std::printf("match");
            for (int32_t m : r.match) std::printf(" %d", m);
            std::printf(" | mdis");
            for (float v : r.matchDis) std::printf(" %08x", bits(v));
            std::printf(" | coef");
            for (float v : r.worldCoef) std::printf(" %08x", bits(v));
            std::printf(" | dis");
            for (float v : r.dis) std::printf(" %08x", bits(v));
            std::printf(" | gated");
            for (uint8_t g : r.gated) std::printf(" %d", (int)g);
            std::printf("\n");
        } else {
            std::fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}

// the timing baseline: `planes` clouds of `points` on random planes, `rows` frame planes per set that coincide with the first planes of the map
static int run_bench(int rows, int planes, int points, int sets, int reps) {
    std::mt19937 rng(7);
    std::uniform_real_distribution<float> U(-1.5f, 1.5f);
    std::normal_distribution<float> N(0.0f, 1.0f);
    HostMap hm;
    std::vector<float> worlds;
    for (int k = 0; k < planes; k++) {
        float n[3] = {N(rng), N(rng), N(rng)};
        const float len = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
        for (float& v : n) v /= len;
        const float d = 0.5f + 3.5f * (float)k / (float)planes;
        std::vector<float> xyz((size_t)points * 3);
        for (int i = 0; i < points; i++) {
            float p[3] = {U(rng), U(rng), U(rng)};
            const float off = p[0] * n[0] + p[1] * n[1] + p[2] * n[2] + d;      // project onto the plane
            for (int a = 0; a < 3; a++) xyz[3 * (size_t)i + a] = p[a] - off * n[a];
        }
        const float w[4] = {n[0], n[1], n[2], d};
        hm.add((uint64_t)k, w, (uint32_t)points, xyz.data());
        worlds.insert(worlds.end(), w, w + 4);
    }
    std::vector<float> M((size_t)sets * 16, 0.0f), coef;
    std::vector<int32_t> start(1, 0);
    for (int s = 0; s < sets; s++) {
        for (int a = 0; a < 4; a++) M[16 * (size_t)s + 5 * a] = 1.0f;
        for (int r = 0; r < rows; r++) coef.insert(coef.end(), &worlds[4 * (size_t)((s * rows + r) % planes)], &worlds[4 * (size_t)((s * rows + r) % planes)] + 4);
        start.push_back((int32_t)coef.size() / 4);
    }
    Result r;
    long long sum = 0;
    const auto t0 = std::chrono::steady_clock::now();
    for (int it = 0; it < reps; it++) {
        associate(hm, sets, M.data(), start.data(), coef.data(), -1, nullptr, 0.2f, 0.8f, r, false);
        for (int32_t m : r.match) sum += m;
    }
    const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() / reps;
    std::printf("{\"rows\": %d, \"planes\": %d, \"points\": %d, \"sets\": %d, \"reps\": %d, \"us_per_call\": %.3f, \"checksum\": %lld}\n", rows, planes, points, sets,
                reps, us, sum);
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 2 && std::string(argv[1]) == "script") return run_script(argc >= 3 ? (size_t)std::atoll(argv[2]) : (size_t)(1 << 13));
    if (argc >= 7 && std::string(argv[1]) == "bench") return run_bench(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]), std::atoi(argv[6]));
    std::fprintf(stderr, "usage: %s script [initial arena points] < commands | bench <rows> <planes> <points> <sets> <reps>\n", argv[0]);
    return 2;
}
