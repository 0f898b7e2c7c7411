// keyframe_database_walk.cpp -- the host half of the device KeyFrameDatabase (eao_fusion_amd/csrc/keyframe_db_internal.h) as a stand-alone program.
//
//   g++ -std=c++17 -fsanitize=address,undefined tools/keyframe_database_walk.cpp -o walk     (tests/test_keyframe_database_host_cpu.py: under the sanitizers)
//   g++ -std=c++17 -O3 tools/keyframe_database_walk.cpp -o walk                                (tools/bench_keyframe_database.py: the host baseline)
//
// `walk script` reads commands from stdin, one per line, and answers each query on stdout.  Floats travel as their bit patterns (decimal integers).
//   words N                                   a new table over N word ids
//   add ID N w0 .. wN-1                        check_add + append; prints "refused" when check_add objects
//   erase ID                                   erase, and plan_compaction / apply_compaction when the dead share is exceeded
//   clear
//   query KIND QID MINSCORE NCONN c.. NLIVE (id common first_word score)..        the intersection arrays in storage order; prints stage 1
//   cand KIND QID MINCOMMON MINSCORE NSCORED (id score).. start0 .. startN nb..    prints stage 2
// `walk bench N_KF WORDS_PER_KF N_WORDS CALLS` times upstream's shape on the host: real inverted lists (std::list per word), the walk of
// DetectRelocalizationCandidates over them, and L1Scoring::score over std::map vectors for the keyframes that pass; prints the median, min and max in ms, the
// median of the walk alone and the keyframes scored per call.
#include <chrono>
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <list>
#include <map>
#include <sstream>

#include "../eao_fusion_amd/csrc/keyframe_db_internal.h"

namespace kfdb = eao::kfdb;

static float f32(uint32_t b) { float f; std::memcpy(&f, &b, 4); return f; }
static uint32_t bits32(float f) { uint32_t b; std::memcpy(&b, &f, 4); return b; }
static double f64(uint64_t b) { double f; std::memcpy(&f, &b, 8); return f; }

static int script() {
    kfdb::Table t;
    int64_t nWords = 0;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        if (cmd == "words") {
            in >> nWords;
            t = kfdb::Table();
        } else if (cmd == "add") {
            uint64_t id; int64_t n;
            in >> id >> n;
            std::vector<uint32_t> w((size_t)std::max<int64_t>(n, 0));
            for (auto& x : w) in >> x;
            const std::string err = t.check_add(id, n, w.data(), nWords);
            if (!err.empty()) std::printf("refused %s\n", err.c_str());
            else t.append(id, (uint32_t)n);
        } else if (cmd == "erase") {
            uint64_t id;
            in >> id;
            if (t.erase(id) && t.wants_compaction()) {
                std::vector<eao::arena::Move> moves;
                const uint64_t live = t.plan_compaction(moves);
                uint64_t moved = 0;
                for (const auto& m : moves) {
                    if (m.dst > m.src || m.dst != moved) return 3;      // the copies ascend and close every gap
                    moved += m.count;
                }
                t.apply_compaction();
                if (moved != live || t.used != live || t.dead != 0) return 3;
                std::printf("compacted %" PRIu64 "\n", live);
            }
        } else if (cmd == "clear") {
            t.clear();
        } else if (cmd == "query") {
            int kind, nconn, nlive; uint64_t qid; uint32_t ms;
            in >> kind >> qid >> ms >> nconn;
            std::unordered_set<uint64_t> connected;
            for (int i = 0; i < nconn; i++) { uint64_t c; in >> c; connected.insert(c); }
            in >> nlive;
            if (nlive != t.nLive) return 2;
            std::vector<uint64_t> id(nlive); std::vector<int32_t> common(nlive); std::vector<uint32_t> first(nlive); std::vector<double> score(nlive);
            for (int j = 0; j < nlive; j++) { uint64_t sb; in >> id[j] >> common[j] >> first[j] >> sb; score[j] = f64(sb); }
            size_t k = 0;
            for (const auto& e : t.entries)
                if (e.live && (k >= id.size() || id[k++] != e.id)) return 2;      // storage order is the add order of the keyframes held
            kfdb::Stage1 r;
            kfdb::walk(t, kind, qid, nlive, id.data(), common.data(), first.data(), score.data(), connected, f32(ms), r);
            std::printf("sharing %zu", r.sharingId.size());
            for (size_t i = 0; i < r.sharingId.size(); i++) std::printf(" %" PRIu64 ":%d", r.sharingId[i], r.sharingWords[i]);
            std::printf(" | %d %d %d | scored %zu", r.maxCommonWords, r.minCommonWords, r.nScores, r.scoredId.size());
            for (size_t i = 0; i < r.scoredId.size(); i++) std::printf(" %" PRIu64 ":%u", r.scoredId[i], bits32(r.scoredScore[i]));
            std::printf("\n");
        } else if (cmd == "cand") {
            int kind, minCommon, n; uint64_t qid; uint32_t ms;
            in >> kind >> qid >> minCommon >> ms >> n;
            std::vector<uint64_t> id(n); std::vector<float> sc(n); std::vector<int32_t> start(n + 1);
            for (int i = 0; i < n; i++) { uint32_t b; in >> id[i] >> b; sc[i] = f32(b); }
            for (auto& s : start) in >> s;
            std::vector<uint64_t> nb((size_t)start[n]);
            for (auto& x : nb) in >> x;
            kfdb::Stage2 r;
            kfdb::candidates(t, kind, qid, minCommon, f32(ms), n, id.data(), sc.data(), start.data(), nb.data(), r);
            std::printf("cand %zu", r.candId.size());
            for (uint64_t c : r.candId) std::printf(" %" PRIu64, c);
            std::printf(" | acc");
            for (float a : r.accScore) std::printf(" %u", bits32(a));
            std::printf(" | best");
            for (uint64_t b : r.bestId) std::printf(" %" PRIu64, b);
            std::printf(" | unset %d\n", r.usedUnset);
        } else {
            return 4;
        }
    }
    return 0;
}

// ---- the host baseline: upstream's data structures and loops
struct BenchKF {
    std::map<uint32_t, double> bow;
    uint64_t relocQuery = 0;
    int relocWords = 0;
    float relocScore = 0;
};

static double score_l1(const std::map<uint32_t, double>& v1, const std::map<uint32_t, double>& v2) {      // ScoringObject.cpp:23-68
    auto a = v1.begin(), b = v2.begin();
    double score = 0;
    while (a != v1.end() && b != v2.end()) {
        if (a->first == b->first) {
            score += std::fabs(a->second - b->second) - std::fabs(a->second) - std::fabs(b->second);
            ++a;
            ++b;
        } else if (a->first < b->first) {
            a = v1.lower_bound(b->first);
        } else {
            b = v2.lower_bound(a->first);
        }
    }
    return -score / 2.0;
}

static int bench(int nKf, int perKf, int nWords, int calls) {
    uint64_t x = 88172645463325252ull;
    auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    auto word = [&]() {      // skewed: a quarter of the draws fall on the first thousandth of the ids, so that lists are uneven
        const uint64_t r = rnd();
        return (uint32_t)((r & 3) == 0 ? (r >> 8) % (uint64_t)std::max(1, nWords / 1000) : (r >> 8) % (uint64_t)nWords);
    };
    auto draw = [&](std::map<uint32_t, double>& v) {
        while ((int)v.size() < perKf) v[word()] = 1.0 / perKf;
    };
    std::vector<BenchKF> kfs((size_t)nKf);
    std::vector<std::list<BenchKF*>> inverted((size_t)nWords);
    for (auto& k : kfs) {
        draw(k.bow);
        for (const auto& w : k.bow) inverted[w.first].push_back(&k);
    }
    std::vector<double> ms, msWalk;
    size_t sink = 0;
    for (int c = 0; c < calls + 10; c++) {
        std::map<uint32_t, double> q;
        draw(q);
        const uint64_t qid = (uint64_t)c + 1;
        const auto t0 = std::chrono::steady_clock::now();
        std::list<BenchKF*> sharing;
        for (const auto& w : q)
            for (BenchKF* k : inverted[w.first]) {
                if (k->relocQuery != qid) {
                    k->relocWords = 0;
                    k->relocQuery = qid;
                    sharing.push_back(k);
                }
                k->relocWords++;
            }
        const auto tw = std::chrono::steady_clock::now();
        int maxCommon = 0;
        for (BenchKF* k : sharing) maxCommon = std::max(maxCommon, k->relocWords);
        const int minCommon = maxCommon * 0.8f;
        for (BenchKF* k : sharing)
            if (k->relocWords > minCommon) {
                k->relocScore = score_l1(q, k->bow);
                sink++;
            }
        const auto t1 = std::chrono::steady_clock::now();
        if (c >= 10) {
            ms.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());
            msWalk.push_back(std::chrono::duration<double, std::milli>(tw - t0).count());
        }
    }
    std::sort(ms.begin(), ms.end());
    std::sort(msWalk.begin(), msWalk.end());
    std::printf("host_walk n_kf %d words %d n_words %d calls %d median_ms %.4f min_ms %.4f max_ms %.4f walk_only_median_ms %.4f scored_per_call %.1f\n", nKf, perKf, nWords,
                calls, ms[ms.size() / 2], ms.front(), ms.back(), msWalk[msWalk.size() / 2], (double)sink / (calls + 10));
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 2 && std::string(argv[1]) == "script") return script();
    if (argc == 6 && std::string(argv[1]) == "bench") return bench(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]));
    std::fprintf(stderr, "usage: %s script < commands | %s bench N_KF WORDS_PER_KF N_WORDS CALLS\n", argv[0], argv[0]);
    return 64;
}
