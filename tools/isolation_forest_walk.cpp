// isolation_forest_walk.cpp -- the host half of the device isolation forest (eao_fusion_amd/csrc/iforest_internal.h) as a program of its own: the forest built on
// the host in the sort-free form the kernel uses, scored and serialised, and upstream's rules and removal (src/Object.cc:1239-1348) over a stand-in object.
// tests/test_isolation_forest_host_cpu.py builds it with -fsanitize=address,undefined and holds its output to the fixtures of the reference's own header;
// built -O3 it is the host baseline of tools/bench_isolation_forest.py.
//
//   input, one command per line (floats as 8-digit hex bit patterns):
//     <tree_count> <seed> <sample_size> <n> <3n floats>      ->  "refused <why>" | "built 0" | "built 1" / "stream <bytes> <hex>" / "scores <n> <hex64>..." /
//                                                                 "totals <n> <hex64>..."
//     object <class> <biForest> <n> <3n floats>              ->  "skipped" | "refused <why>" | "flags <n> <0|1>..." / "kept <m> <indices>" / "sum <3 hex64>"
//     time <repeats> <tree_count> <seed> <sample_size> <n> <3n floats>   ->  "time_us <mean>"
#include <chrono>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "../eao_fusion_amd/csrc/iforest_internal.h"

using namespace eao::iforest;

static std::vector<float> read_points(std::istringstream& in, uint32_t n) {
    std::vector<float> xyz((size_t)n * 3);
    for (auto& v : xyz) {
        std::string h;
        in >> h;
        const uint32_t bits = (uint32_t)std::stoul(h, nullptr, 16);
        std::memcpy(&v, &bits, 4);
    }
    return xyz;
}

static void print_doubles(const char* tag, const std::vector<double>& v) {
    std::printf("%s %zu", tag, v.size());
    for (double d : v) {
        uint64_t bits;
        std::memcpy(&bits, &d, 8);
        std::printf(" %016llx", (unsigned long long)bits);
    }
    std::printf("\n");
}

// the stand-in for Object_Map: mvpMapObjectMappoints as indices into the points, mSumPointsPos as three doubles
struct StandInObject {
    std::vector<uint32_t> points;
    double sum[3] = {0, 0, 0};
};

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::string first;
        in >> first;
        if (first == "object") {
            int cls, bi;
            uint32_t n;
            in >> cls >> bi >> n;
            const std::vector<float> xyz = read_points(in, n);
            if (!object_runs(bi != 0, cls, n)) {
                std::printf("skipped\n");
                continue;
            }
            const uint32_t S = n / kSampleDivisor;
            if (const char* why = refusal(n, S, kTreeCount)) { std::printf("refused %s\n", why); continue; }
            if (!all_finite(xyz.data(), n)) { std::printf("refused a non-finite coordinate\n"); continue; }
            HostForest f;
            if (!f.build(kTreeCount, kSeed, xyz.data(), n, S)) { std::printf("skipped\n"); continue; }
            std::vector<uint8_t> flags(n);
            const double th = object_threshold(cls);
            for (uint32_t i = 0; i < n; i++) flags[i] = f.score(&xyz[3 * i]) > th;
            StandInObject obj;
            for (uint32_t i = 0; i < n; i++) {
                obj.points.push_back(i);
                for (int c = 0; c < 3; c++) obj.sum[c] += xyz[3 * i + c];
            }
            // the removal of :1324-1347 over the flagged indices, walked with a bound
            const std::vector<uint32_t> out = flagged_indices(flags.data(), n);
            size_t nextOut = 0;
            uint32_t index = 0;
            for (auto it = obj.points.begin(); it != obj.points.end(); index++) {
                if (nextOut < out.size() && index == out[nextOut]) {
                    nextOut++;
                    for (int c = 0; c < 3; c++) obj.sum[c] -= xyz[3 * *it + c];
                    it = obj.points.erase(it);
                } else {
                    ++it;
                }
            }
            std::printf("flags %u", n);
            for (uint8_t fl : flags) std::printf(" %d", fl);
            std::printf("\nkept %zu", obj.points.size());
            for (uint32_t p : obj.points) std::printf(" %u", p);
            std::printf("\n");
            print_doubles("sum", std::vector<double>(obj.sum, obj.sum + 3));
            continue;
        }
        int repeats = 0;
        uint32_t treeCount;
        if (first == "time") in >> repeats >> treeCount;
        else treeCount = (uint32_t)std::stoul(first);
        uint32_t seed, S, n;
        in >> seed >> S >> n;
        const std::vector<float> xyz = read_points(in, n);
        if (const char* why = refusal(n, S, treeCount)) { std::printf("refused %s\n", why); continue; }
        if (!all_finite(xyz.data(), n)) { std::printf("refused a non-finite coordinate\n"); continue; }
        if (repeats > 0) {
            const auto t0 = std::chrono::steady_clock::now();
            double sink = 0;
            for (int r = 0; r < repeats; r++) {
                HostForest f;
                if (f.build(treeCount, seed, xyz.data(), n, S))
                    for (uint32_t i = 0; i < n; i++) sink += f.score(&xyz[3 * i]);
            }
            std::printf("time_us %.3f %g\n", std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() / repeats, sink);
            continue;
        }
        HostForest f;
        if (!f.build(treeCount, seed, xyz.data(), n, S)) { std::printf("built 0\n"); continue; }
        std::printf("built 1\n");
        const std::vector<uint8_t> bytes = f.stream();
        std::printf("stream %zu ", bytes.size());
        for (uint8_t b : bytes) std::printf("%02x", b);
        std::printf("\n");
        std::vector<double> scores(n), totals(n);
        for (uint32_t i = 0; i < n; i++) {
            totals[i] = f.total(&xyz[3 * i]);
            scores[i] = finish_score(totals[i], treeCount, f.cTable[S]);
        }
        print_doubles("scores", scores);
        print_doubles("totals", totals);
    }
    return 0;
}
