// The chained update of a map object on the host (eao_fusion_amd/csrc/object_chain_internal.h: the three HIP-free headers of the point update, the cuboid and the
// isolation forest chained in upstream's order, reference src/Object.cc:1352-1601) as a program of its own.  tests/test_object_chain_host_cpu.py builds it with
// g++ -fsanitize=address,undefined and holds every scene to the yardstick; tools/bench_object_chain.py builds it with -O3 for the host baseline.  Reads a script
// on stdin, floats as 8-digit and doubles as 16-digit hex:
//
//   chain <the desc of tools/object_points_walk.cpp's `update`> <class_id> <bi_forest> <planted_failure> <has_alias> <n_centroids> <9 floats Ryaw>
//         <3 doubles prev_cuboid_center> n_centroids x <x y z> n_map x <bad> n_cand x <bad> [n_cand x <alias>]
//        -> the points line of tools/object_points_walk.cpp without the positions and, with status DONE,
//           " || <final pairs> || <the record line of tools/object_cuboid_walk.cpp> || <n_final forest_status removed> | <flags> | <scores>"; a NaN prints as nan
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

#include "../eao_fusion_amd/csrc/object_chain_internal.h"

using namespace eao::object_chain;

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
    std::vector<float> mapPoints, candPoints, centroids;
    std::vector<int32_t> mapCount, candCount, alias;
    std::vector<uint8_t> mapBad, candBad;
    eao_object_chain_desc d;
    bool planted = false;
};

static void read_desc(std::istream& in, Desc& O) {
    O.d = eao_object_chain_desc{};
    eao_object_points_desc& d = O.d.points;
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
    int planted = 0, hasAlias = 0;
    in >> O.d.class_id >> O.d.bi_forest >> planted >> hasAlias >> O.d.n_centroids;
    O.planted = planted != 0;
    for (float& v : O.d.Ryaw) v = read_float(in);
    for (double& v : O.d.prev_cuboid_center) v = read_double(in);
    O.centroids.resize(3 * (O.d.n_centroids > 0 ? (size_t)O.d.n_centroids : 0));
    for (float& v : O.centroids) v = read_float(in);
    O.mapBad.resize(M); O.candBad.resize(C);
    for (uint8_t& v : O.mapBad) { int b; in >> b; v = (uint8_t)b; }
    for (uint8_t& v : O.candBad) { int b; in >> b; v = (uint8_t)b; }
    if (hasAlias) {
        O.alias.resize(C);
        for (int32_t& v : O.alias) in >> v;
    }
    O.d.centroids = O.centroids.data();
    O.d.map_bad = O.mapBad.data(); O.d.cand_bad = O.candBad.data();
    O.d.cand_alias = hasAlias ? O.alias.data() : nullptr;
}

static void print_f(float v) {
    uint32_t bits;
    std::memcpy(&bits, &v, 4);
    if (std::isnan(v)) std::printf(" nan");
    else std::printf(" %08x", bits);
}

static void print_d(double v) {
    uint64_t bits;
    std::memcpy(&bits, &v, 8);
    if (std::isnan(v)) std::printf(" nan");
    else std::printf(" %016llx", (unsigned long long)bits);
}

template <class T>
static void print_ints(const std::vector<T>& v) {
    std::printf(" |");
    for (T x : v) std::printf(" %d", (int)x);
}

static void print_cuboid(const eao_object_cuboid_rec& r) {
    std::printf(" rec %d %d", r.status, r.bounds_written);
    for (float v : r.sum_pos) print_f(v);
    for (float v : r.center) print_f(v);
    for (float v : r.standar) print_f(v);
    for (float v : r.center_standar) print_f(v);
    print_f(r.center_standar_dis);
    for (float v : r.bounds) print_f(v);
    print_f(r.lenth); print_f(r.width); print_f(r.height); print_f(r.rmax);
    for (float v : r.Twobj) print_f(v);
    for (float v : r.Twobj_without_yaw) print_f(v);
    for (double v : r.cuboid_center) print_d(v);
    for (int c = 0; c < 8; c++) for (double v : r.corners[c]) print_d(v);
    for (int c = 0; c < 8; c++) for (double v : r.corners_w[c]) print_d(v);
    for (double v : r.pose_q) print_d(v);
    for (double v : r.pose_t) print_d(v);
    for (double v : r.pose_without_yaw_q) print_d(v);
    for (double v : r.pose_without_yaw_t) print_d(v);
}

static void print_walk(const Walk& W) {
    const eao_object_points_rec& r = W.points.rec;
    std::printf("rec %d %d %d %d %d %d", r.status, r.n_gated, r.n_appended, r.n_list, r.n_erased, r.n_survivors);
    for (int32_t v : r.rect2) std::printf(" %d", v);
    print_f(r.iou); print_f(r.iou2);
    for (float v : r.sum_pos_appended) print_f(v);
    for (float v : r.sum_pos) print_f(v);
    if (r.status == op::kDone) {
        print_ints(W.points.gate); print_ints(W.points.target); print_ints(W.points.count); print_ints(W.points.list); print_ints(W.points.erased);
        print_ints(W.points.survivors);
        std::printf(" |");
        print_ints(W.final);
        std::printf(" ||");
        print_cuboid(W.cuboid);
        std::printf(" || %d %d %d", W.rec.n_final, W.rec.forest_status, W.rec.removed);
        print_ints(W.flags);
        std::printf(" |");
        for (double v : W.scores) print_d(v);
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
        if (verb == "chain") {
            Desc O;
            read_desc(in, O);
            Walk W;
            walk_chain(O.d, W, O.planted);
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
                    walk_chain(O->d, W);
                    sink += W.points.rec.sum_pos[0] + W.rec.n_final + W.rec.removed;
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
