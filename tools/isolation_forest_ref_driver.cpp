// isolation_forest_ref_driver.cpp -- runs the REFERENCE's include/isolation_forest.h (reached through -I only; none of its text is here) on point sets read from
// stdin and prints what tools/gen_golden_isolation_forest.py records: the bytes of IsolationForest::Serialize and the anomaly scores as bit patterns.
//
//   input, one scene per line:   <tree_count> <seed> <sample_size> <n> then 3n floats as 8-digit hex bit patterns
//   output, per scene:           "built 0"  |  "built 1" / "stream <bytes> <hex>" / "scores <n> <16-digit hex> ..."
//
// `time <repeats>` in front of the numbers instead prints the mean wall time in microseconds of Build + GetAnomalyScores (the host baseline quoted in
// profiles/isolation_forest_timing.txt).
#include <isolation_forest.h>

#include <chrono>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        int repeats = 0;
        std::string first;
        in >> first;
        uint32_t treeCount;
        if (first == "time") {
            in >> repeats >> treeCount;
        } else {
            treeCount = (uint32_t)std::stoul(first);
        }
        uint32_t seed, sampleSize, n;
        in >> seed >> sampleSize >> n;
        std::vector<std::array<float, 3>> data(n);
        for (uint32_t i = 0; i < n; i++)
            for (int c = 0; c < 3; c++) {
                std::string h;
                in >> h;
                const uint32_t bits = (uint32_t)std::stoul(h, nullptr, 16);
                std::memcpy(&data[i][c], &bits, 4);
            }
        if (repeats > 0) {
            const auto t0 = std::chrono::steady_clock::now();
            double sink = 0;
            for (int r = 0; r < repeats; r++) {
                iforest::IsolationForest<float, 3> forest;
                std::vector<double> scores;
                if (forest.Build(treeCount, seed, data, sampleSize) && forest.GetAnomalyScores(data, scores)) sink += scores[0];
            }
            const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() / repeats;
            std::printf("time_us %.3f %g\n", us, sink);
            continue;
        }
        iforest::IsolationForest<float, 3> forest;
        if (!forest.Build(treeCount, seed, data, sampleSize)) {
            std::printf("built 0\n");
            continue;
        }
        std::printf("built 1\n");
        std::ostringstream os;
        forest.Serialize(os);
        const std::string bytes = os.str();
        std::printf("stream %zu ", bytes.size());
        for (unsigned char b : bytes) std::printf("%02x", b);
        std::printf("\n");
        std::vector<double> scores;
        forest.GetAnomalyScores(data, scores);
        std::printf("scores %zu", scores.size());
        for (double s : scores) {
            uint64_t bits;
            std::memcpy(&bits, &s, 8);
            std::printf(" %016llx", (unsigned long long)bits);
        }
        std::printf("\n");
    }
    return 0;
}
