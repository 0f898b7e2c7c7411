// A frame's 2D objects in upstream's literal form (eao_fusion_amd/csrc/frame_objects_internal.h: push_back, sort, erase; reference src/Tracking.cc:1768-1973,
// :3031-3065, src/Object.cc:61-157) as a program of its own.  tests/test_frame_objects_host_cpu.py builds it with g++ -fsanitize=address,undefined and holds every
// scene to the yardstick; tools/bench_frame_objects.py builds it with -O3 for the host baseline.  Reads a script on stdin, floats as 8-digit hex:
//
//   frame <n_kp> <n_box> <cols> <rows> <fx fy cx cy> <16 floats Tcw> n_kp x (<kp_x kp_y> <mp_id> <x y z>) n_box x (<x y width height> <score>)
//        -> per box "rec <n_assigned n boxplot_ran has_feature_rect> <feature_rect x4> <num_overlaps bad on_edge> <14 floats: sum_pos pos std q1 q3 max_th
//           center_2d; a NaN prints as nan>", "a <the list after step 2>", "k <the list after the boxplot>"
//   load ...   a frame as above, kept for `time`, no output
//   time <reps>
//        -> "time <us per walk of every loaded frame>", single-threaded
//   refuse ... a frame as above -> "refused <reason>" or "accepted"
//   gate <n>   the inner gate of RemoveOutliersByBoxPlot (src/Object.cc:131) on a list of n points, which the `>= 8` gate in front of it never lets through:
//        -> "gate <1 = it returned> <the list's length afterwards>"
#include <chrono>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../eao_fusion_amd/csrc/frame_objects_internal.h"

using namespace eao::frame_objects;

static float read_float(std::istream& in) {
    std::string h;
    in >> h;
    const uint32_t bits = (uint32_t)std::stoul(h, nullptr, 16);
    float f;
    std::memcpy(&f, &bits, 4);
    return f;
}

struct Frame {
    std::vector<float> kx, ky, xyz, score;
    std::vector<int32_t> id, boxes;
    eao_frame_objects_desc d;
};

static void read_frame(std::istream& in, Frame& F) {
    eao_frame_objects_desc& d = F.d;
    in >> d.n_kp >> d.n_box >> d.cols >> d.rows;
    d.fx = read_float(in); d.fy = read_float(in); d.cx = read_float(in); d.cy = read_float(in);
    for (int k = 0; k < 16; k++) d.Tcw[k] = read_float(in);
    const size_t n = d.n_kp > 0 ? (size_t)d.n_kp : 0, m = d.n_box > 0 ? (size_t)d.n_box : 0;
    F.kx.resize(n); F.ky.resize(n); F.id.resize(n); F.xyz.resize(3 * n); F.boxes.resize(4 * m); F.score.resize(m);
    for (size_t i = 0; i < n; i++) {
        F.kx[i] = read_float(in);
        F.ky[i] = read_float(in);
        in >> F.id[i];
        for (int a = 0; a < 3; a++) F.xyz[3 * i + a] = read_float(in);
    }
    for (size_t k = 0; k < m; k++) {
        for (int a = 0; a < 4; a++) in >> F.boxes[4 * k + a];
        F.score[k] = read_float(in);
    }
    d.kp_x = F.kx.data(); d.kp_y = F.ky.data(); d.mp_id = F.id.data(); d.mp_xyz = F.xyz.data();
    d.boxes = F.boxes.data(); d.score = F.score.data();
}

static void print_list(const char* tag, const std::vector<int32_t>& v) {
    std::printf("%s", tag);
    for (int32_t i : v) std::printf(" %d", i);
    std::printf("\n");
}

int main() {
    std::string line;
    std::vector<Frame*> loaded;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::string verb;
        in >> verb;
        if (verb == "frame") {
            Frame F;
            read_frame(in, F);
            Walk W;
            walk_frame(F.d, W);
            for (size_t k = 0; k < W.rec.size(); k++) {
                const eao_frame_object_record& r = W.rec[k];
                std::printf("rec %d %d %d %d %d %d %d %d %d %d %d", r.n_assigned, r.n, r.boxplot_ran, r.has_feature_rect, r.feature_rect[0], r.feature_rect[1],
                            r.feature_rect[2], r.feature_rect[3], r.num_overlaps, r.bad, r.on_edge);
                const float fl[14] = {r.sum_pos[0], r.sum_pos[1], r.sum_pos[2], r.pos[0], r.pos[1], r.pos[2], r.std[0], r.std[1], r.std[2],
                                      r.q1, r.q3, r.max_th, r.center_2d[0], r.center_2d[1]};
                for (int j = 0; j < 14; j++) {
                    uint32_t bits;
                    std::memcpy(&bits, &fl[j], 4);
                    if (std::isnan(fl[j])) std::printf(" nan");
                    else std::printf(" %08x", bits);
                }
                std::printf("\n");
                print_list("a", W.assigned[k]);
                print_list("k", W.kept[k]);
            }
        } else if (verb == "load") {
            Frame* F = new Frame;
            read_frame(in, *F);
            loaded.push_back(F);
        } else if (verb == "time") {
            int reps;
            in >> reps;
            long sink = 0;
            const auto t0 = std::chrono::steady_clock::now();
            for (int rep = 0; rep < reps; rep++)
                for (Frame* F : loaded) {
                    Walk W;
                    walk_frame(F->d, W);
                    for (const eao_frame_object_record& r : W.rec) sink += r.n + r.bad;
                }
            const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() / reps;
            std::printf("time %.1f sink %ld\n", us, sink);
        } else if (verb == "refuse") {
            Frame F;
            read_frame(in, F);
            const char* why = frame_refusal(F.d);
            std::printf("%s%s\n", why ? "refused " : "accepted", why ? why : "");
        } else if (verb == "gate") {
            int n;
            in >> n;
            Frame F;
            F.d = eao_frame_objects_desc{};
            for (int k = 0; k < 16; k++) F.d.Tcw[k] = (k % 5 == 0) ? 1.0f : 0.0f;
            std::vector<int32_t> list;
            for (int i = 0; i < n; i++) {
                list.push_back(i);
                F.xyz.push_back(0.0f); F.xyz.push_back(0.0f); F.xyz.push_back(i == n - 1 ? 1000.0f : 1.0f + 0.01f * (float)i);      // the last point lies far behind
            }
            F.d.mp_xyz = F.xyz.data();
            float q1 = 0, q3 = 0, th = 0;
            const bool ran = boxplot(F.d, list, &q1, &q3, &th);
            std::printf("gate %d %d\n", ran ? 0 : 1, (int)list.size());
        } else {
            std::fprintf(stderr, "unknown verb %s\n", verb.c_str());
            return 2;
        }
        std::fflush(stdout);
    }
    for (Frame* F : loaded) delete F;
    return 0;
}
