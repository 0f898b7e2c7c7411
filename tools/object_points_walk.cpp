// The update of a map object's point list in upstream's literal form (eao_fusion_amd/csrc/object_points_internal.h: the growing list, the `break`, the erase while
// iterating; reference src/Object.cc:1364-1589, :1766-1821, :2070-2120) as a program of its own.  tests/test_object_points_host_cpu.py builds it with
// g++ -fsanitize=address,undefined and holds every scene to the yardstick; tests/test_gpu_object_points.py holds the device to it;
// tools/bench_object_points.py builds it with -O3 for the host baseline.  Reads a script on stdin, floats as 8-digit and doubles as 16-digit hex:
//
//   update <change_gate gate erase box_off_edge cols rows n_frames_after_push> <n_map> <n_cand> <fx fy cx cy rmax lenth width height> <16 floats Tcw>
//          <4 ints project_rect1> <4 ints box_rect> <3 floats center> <4 doubles pose_q> <3 doubles pose_t> <3 doubles cuboid_center> <6 floats bounds>
//          <3 floats overlap> <3 floats sum_pos> n_map x <x y z> n_map x <count> n_cand x <x y z> n_cand x <count>
//        -> "rec <status n_gated n_appended n_list n_erased n_survivors> <rect2> <iou iou2> <sum_pos_appended> <sum_pos>" and, with status DONE,
//           " | gate | target | count | list | erased | survivors | the surviving positions"; a NaN prints as nan
//   load ...   a desc as above, kept for `time`, no output
//   time <reps>
//        -> "time <us per walk of every loaded desc>", single-threaded
//   refuse ... a desc as above -> "refused <reason>" or "accepted"
#include <chrono>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../eao_fusion_amd/csrc/object_points_internal.h"

using namespace eao::object_points;

static float read_float(std::istream& in) {
    std::string h;
    in >> h;
    const uint32_t bits = (uint32_t)std::stoul(h, nullptr, 16);
    float f;
    std::memcpy(&f, &bits, 4);
    return f;
}

static double read_double(std::istream& in) {
    std::string h;
    in >> h;
    const uint64_t bits = (uint64_t)std::stoull(h, nullptr, 16);
    double d;
    std::memcpy(&d, &bits, 8);
    return d;
}

struct Desc {
    std::vector<float> mapPoints, candPoints;
    std::vector<int32_t> mapCount, candCount;
    eao_object_points_desc d;
};

static void read_desc(std::istream& in, Desc& O) {
    eao_object_points_desc& d = O.d;
    d = eao_object_points_desc{};
    in >> d.change_gate >> d.gate >> d.erase >> d.box_off_edge >> d.cols >> d.rows >> d.n_frames_after_push >> d.n_map >> d.n_cand;
    d.fx = read_float(in); d.fy = read_float(in); d.cx = read_float(in); d.cy = read_float(in);
    d.rmax = read_float(in); d.lenth = read_float(in); d.width = read_float(in); d.height = read_float(in);
    for (float& v : d.Tcw) v = read_float(in);
    for (int32_t& v : d.project_rect1) in >> v;
    for (int32_t& v : d.box_rect) in >> v;
    for (float& v : d.center) v = read_float(in);
    for (double& v : d.pose_q) v = read_double(in);
    for (double& v : d.pose_t) v = read_double(in);
    for (double& v : d.cuboid_center) v = read_double(in);
    for (float& v : d.bounds) v = read_float(in);
    for (float& v : d.overlap) v = read_float(in);
    for (float& v : d.sum_pos) v = read_float(in);
    const size_t M = d.n_map > 0 ? (size_t)d.n_map : 0, C = d.n_cand > 0 ? (size_t)d.n_cand : 0;
    O.mapPoints.resize(3 * M); O.mapCount.resize(M);
    O.candPoints.resize(3 * C); O.candCount.resize(C);
    for (float& v : O.mapPoints) v = read_float(in);
    for (int32_t& v : O.mapCount) in >> v;
    for (float& v : O.candPoints) v = read_float(in);
    for (int32_t& v : O.candCount) in >> v;
    d.map_points = O.mapPoints.data(); d.map_count = O.mapCount.data();
    d.cand_points = O.candPoints.data(); d.cand_count = O.candCount.data();
}

static void print_f(float v) {
    uint32_t bits;
    std::memcpy(&bits, &v, 4);
    if (std::isnan(v)) std::printf(" nan");
    else std::printf(" %08x", bits);
}

template <class T>
static void print_ints(const std::vector<T>& v) {
    std::printf(" |");
    for (T x : v) std::printf(" %d", (int)x);
}

static void print_walk(const Walk& W) {
    const eao_object_points_rec& r = W.rec;
    std::printf("rec %d %d %d %d %d %d", r.status, r.n_gated, r.n_appended, r.n_list, r.n_erased, r.n_survivors);
    for (int32_t v : r.rect2) std::printf(" %d", v);
    print_f(r.iou); print_f(r.iou2);
    for (float v : r.sum_pos_appended) print_f(v);
    for (float v : r.sum_pos) print_f(v);
    if (r.status == kDone) {
        print_ints(W.gate); print_ints(W.target); print_ints(W.count); print_ints(W.list); print_ints(W.erased); print_ints(W.survivors);
        std::printf(" |");
        for (float v : W.points) print_f(v);
    }
    std::printf("\n");
}

int main() {
    std::string line;
    std::vector<Desc*> loaded;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::string verb;
        in >> verb;
        if (verb == "update") {
            Desc O;
            read_desc(in, O);
            Walk W;
            walk_update(O.d, W);
            print_walk(W);
        } else if (verb == "load") {
            Desc* O = new Desc;
            read_desc(in, *O);
            loaded.push_back(O);
        } else if (verb == "time") {
            int reps;
            in >> reps;
            double sink = 0;
            const auto t0 = std::chrono::steady_clock::now();
            for (int rep = 0; rep < reps; rep++)
                for (Desc* O : loaded) {
                    Walk W;
                    walk_update(O->d, W);
                    sink += W.rec.sum_pos[0] + W.rec.n_survivors;
                }
            const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() / reps;
            std::printf("time %.1f sink %g\n", us, sink);
        } else if (verb == "refuse") {
            Desc O;
            read_desc(in, O);
            const char* why = desc_refusal(O.d);
            std::printf("%s%s\n", why ? "refused " : "accepted", why ? why : "");
        } else {
            std::fprintf(stderr, "unknown verb %s\n", verb.c_str());
            return 2;
        }
        std::fflush(stdout);
    }
    for (Desc* O : loaded) delete O;
    return 0;
}
