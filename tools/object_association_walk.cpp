// The host half of the object layer's data association (eao_fusion_amd/csrc/object_assoc_internal.h) as a program of its own: the plan of a pair, a brute-force
// count in the kernel's form (lb / ub over all good points, then the ceil rule), the decision, and the projection with the clamps and the float -> int
// conversion.  tests/test_object_association_host_cpu.py builds it with g++ -fsanitize=address,undefined and holds every scene to the yardstick;
// tools/bench_object_association.py builds it with -O3 for the host baseline.  Reads a script on stdin, floats as 8-digit hex:
//
//   np <S> <m> <3m floats> <nGood> <3nGood floats>
//        -> "mns <m> <n> <step>", "counts <9>", "w <3 hex>", "r <2 hex>", "verdict <v>"
//   rect <cols> <rows> <fx fy cx cy> <16 floats Tcw> <n> <3n floats>
//        -> "status <s>", "rect <x y w h>" (only with status 1), "uv <2n hex>"
//   time <nDet> <m> <nMap> <nGood> <reps>
//        -> "time <us per repetition: the kernel's form> <us: upstream's form, sort and three compares per pair>" for nDet x nMap pairs over
//           points of its own making, single-threaded
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../eao_fusion_amd/csrc/object_assoc_internal.h"

using namespace eao::object_assoc;

static float read_float(std::istream& in) {
    std::string h;
    in >> h;
    const uint32_t bits = (uint32_t)std::stoul(h, nullptr, 16);
    float f;
    std::memcpy(&f, &bits, 4);
    return f;
}
static std::vector<float> read_floats(std::istream& in, size_t n) {
    std::vector<float> v(n);
    for (size_t i = 0; i < n; i++) v[i] = read_float(in);
    return v;
}
static void print_hex(const char* tag, const float* v, size_t n) {
    std::printf("%s", tag);
    for (size_t i = 0; i < n; i++) {
        uint32_t bits;
        std::memcpy(&bits, &v[i], 4);
        std::printf(" %08x", bits);
    }
    std::printf("\n");
}

// one pair as the library decides it: plan, count, decide
static int32_t one_pair(const float* det, int32_t m, const float* map, int32_t nGood, int32_t S, Plan& p, uint32_t* c, float* w, float* r) {
    p = plan_pair(m, nGood, S);
    for (int k = 0; k < 9; k++) c[k] = 0;
    w[0] = w[1] = w[2] = r[0] = r[1] = 0.0f;
    if (p.verdict != kPending) return p.verdict;
    count_pair(det, m, map, nGood, p.step, p.n, c);
    return decide(p.m, p.n, c, w, r);
}

// src/Object.cc:776-961 as upstream runs it, for the timing only: sort each axis, stride, three compares per pair into float counters
static int32_t upstream_form(const float* det, int32_t m, const float* map, int32_t nGood, int32_t S) {
    const Plan p = plan_pair(m, nGood, S);
    if (p.verdict != kPending) return p.verdict;
    std::vector<float> axis[3], sample[3];
    for (int a = 0; a < 3; a++) {
        for (int32_t j = 0; j < nGood; j++) axis[a].push_back(map[3 * j + a]);
        if (nGood > kSampleRatio * m) {
            std::sort(axis[a].begin(), axis[a].end());
            for (int32_t j = 0; j < nGood; j += p.step) sample[a].push_back(axis[a][j]);
        } else {
            sample[a] = axis[a];
        }
    }
    float wc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int32_t i = 0; i < m; i++)
        for (size_t j = 0; j < sample[0].size(); j++)
            for (int a = 0; a < 3; a++) {
                const double x1 = det[3 * i + a], x2 = sample[a][j];
                if (x1 > x2) wc[3 * a]++;
                else if (x1 < x2) wc[3 * a + 1]++;
                else if (x1 == x2) wc[3 * a + 2]++;
            }
    uint32_t c[9];
    for (int k = 0; k < 9; k++) c[k] = (uint32_t)wc[k];
    float w[3], r[2];
    return decide(p.m, p.n, c, w, r);
}

static std::vector<float> made_up_points(size_t n, uint32_t& state) {
    std::vector<float> v(3 * n);
    for (float& f : v) {
        state = state * 1664525u + 1013904223u;
        f = (float)(state >> 8) / 16777216.0f;
    }
    return v;
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::string verb;
        in >> verb;
        if (verb == "np") {
            int32_t S, m, nGood;
            in >> S >> m;
            const std::vector<float> det = read_floats(in, 3 * (size_t)m);
            in >> nGood;
            const std::vector<float> map = read_floats(in, 3 * (size_t)nGood);
            Plan p;
            uint32_t c[9];
            float w[3], r[2];
            const int32_t verdict = one_pair(det.data(), m, map.data(), nGood, S, p, c, w, r);
            std::printf("mns %d %d %d\ncounts", p.m, p.n, p.step);
            for (int k = 0; k < 9; k++) std::printf(" %u", c[k]);
            std::printf("\n");
            print_hex("w", w, 3);
            print_hex("r", r, 2);
            std::printf("verdict %d\n", verdict);
        } else if (verb == "rect") {
            int32_t cols, rows, n;
            in >> cols >> rows;
            const std::vector<float> cam = read_floats(in, 4), T = read_floats(in, 16);
            in >> n;
            const std::vector<float> pts = read_floats(in, 3 * (size_t)n);
            std::vector<float> uv(2 * (size_t)n);
            Extent e;
            extent_init(e);
            for (int32_t i = 0; i < n; i++) {
                project_point(T.data(), cam[0], cam[1], cam[2], cam[3], pts.data() + 3 * i, &uv[2 * i], &uv[2 * i + 1]);
                extent_add(e, uv[2 * i], uv[2 * i + 1]);
            }
            int32_t rect[4] = {0, 0, 0, 0};
            const uint8_t status = n == 0 ? kRectEmpty : finish_rect(e, cols, rows, rect);
            std::printf("status %d\n", (int)status);
            if (status == kRectOk) std::printf("rect %d %d %d %d\n", rect[0], rect[1], rect[2], rect[3]);
            print_hex("uv", uv.data(), uv.size());
        } else if (verb == "time") {
            int32_t nDet, m, nMap, nGood, reps;
            in >> nDet >> m >> nMap >> nGood >> reps;
            uint32_t state = 12345u;
            std::vector<std::vector<float>> dets, maps;
            for (int32_t d = 0; d < nDet; d++) dets.push_back(made_up_points((size_t)m, state));
            for (int32_t j = 0; j < nMap; j++) maps.push_back(made_up_points((size_t)nGood, state));
            double us[2];
            long sink = 0;
            for (int form = 0; form < 2; form++) {
                const auto t0 = std::chrono::steady_clock::now();
                for (int32_t rep = 0; rep < reps; rep++)
                    for (int32_t d = 0; d < nDet; d++)
                        for (int32_t j = 0; j < nMap; j++) {
                            if (form == 0) {
                                Plan p;
                                uint32_t c[9];
                                float w[3], r[2];
                                sink += one_pair(dets[d].data(), m, maps[j].data(), nGood, nGood, p, c, w, r);
                            } else {
                                sink += upstream_form(dets[d].data(), m, maps[j].data(), nGood, nGood);
                            }
                        }
                us[form] = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() / reps;
            }
            std::printf("time %.1f %.1f sink %ld\n", us[0], us[1], sink);
        } else {
            std::fprintf(stderr, "unknown verb %s\n", verb.c_str());
            return 2;
        }
        std::fflush(stdout);
    }
    return 0;
}
