// A map object's cuboid in upstream's literal form (eao_fusion_amd/csrc/object_cuboid_internal.h: push_back, sort, the early returns; reference
// src/Object.cc:999-1235, :1954-1970, :2243-2303) as a program of its own.  tests/test_object_cuboid_host_cpu.py builds it with g++ -fsanitize=address,undefined
// and holds every scene to the yardstick; tests/test_gpu_object_cuboid.py holds the device to it; tools/bench_object_cuboid.py builds it with -O3 for the host
// baseline.  Reads a script on stdin, floats as 8-digit and doubles as 16-digit hex:
//
//   object <n> <m> <9 floats Ryaw> <3 doubles prev_cuboid_center> n x <x y z> m x <x y z>
//        -> "rec <status> <bounds_written> <the record's float and double fields in the record's order; a NaN prints as nan>"
//   load ...   an object as above, kept for `time`, no output
//   time <reps>
//        -> "time <us per walk of every loaded object>", single-threaded
//   refuse ... an object as above -> "refused <reason>" or "accepted"
//   overlaps <m> m x (<3 doubles cuboid_center> <lenth width height> <eligible>)
//        -> "ov <m * m verdicts>", then "ex <i> <j> <3 floats>" per pair whose verdict is 1
#include <chrono>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../eao_fusion_amd/csrc/object_cuboid_internal.h"

using namespace eao::object_cuboid;

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

struct Object {
    std::vector<float> points, centroids;
    eao_object_cuboid_desc d;
};

static void read_object(std::istream& in, Object& O) {
    eao_object_cuboid_desc& d = O.d;
    in >> d.n_points >> d.n_centroids;
    for (int k = 0; k < 9; k++) d.Ryaw[k] = read_float(in);
    for (int k = 0; k < 3; k++) d.prev_cuboid_center[k] = read_double(in);
    const size_t n = d.n_points > 0 ? (size_t)d.n_points : 0, m = d.n_centroids > 0 ? (size_t)d.n_centroids : 0;
    O.points.resize(3 * n);
    O.centroids.resize(3 * m);
    for (float& v : O.points) v = read_float(in);
    for (float& v : O.centroids) v = read_float(in);
    d.points = O.points.data();
    d.centroids = O.centroids.data();
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

static void print_record(const eao_object_cuboid_rec& r) {
    std::printf("rec %d %d", r.status, r.bounds_written);
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
    std::printf("\n");
}

int main() {
    std::string line;
    std::vector<Object*> loaded;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::string verb;
        in >> verb;
        if (verb == "object") {
            Object O;
            read_object(in, O);
            eao_object_cuboid_rec r;
            walk_object(O.d, r);
            print_record(r);
        } else if (verb == "load") {
            Object* O = new Object;
            read_object(in, *O);
            loaded.push_back(O);
        } else if (verb == "time") {
            int reps;
            in >> reps;
            double sink = 0;
            const auto t0 = std::chrono::steady_clock::now();
            for (int rep = 0; rep < reps; rep++)
                for (Object* O : loaded) {
                    eao_object_cuboid_rec r;
                    walk_object(O->d, r);
                    sink += r.rmax + r.status;
                }
            const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() / reps;
            std::printf("time %.1f sink %g\n", us, sink);
        } else if (verb == "refuse") {
            Object O;
            read_object(in, O);
            const char* why = object_refusal(O.d);
            std::printf("%s%s\n", why ? "refused " : "accepted", why ? why : "");
        } else if (verb == "overlaps") {
            int m;
            in >> m;
            std::vector<eao_object_overlap_row> rows((size_t)m);
            std::vector<uint8_t> eligible((size_t)m), verdict((size_t)m * m);
            std::vector<float> extents((size_t)m * m * 3);
            for (int i = 0; i < m; i++) {
                rows[i] = eao_object_overlap_row{};
                for (int k = 0; k < 3; k++) rows[i].cuboid_center[k] = read_double(in);
                rows[i].lenth = read_float(in); rows[i].width = read_float(in); rows[i].height = read_float(in);
                int e;
                in >> e;
                eligible[i] = (uint8_t)e;
            }
            walk_overlaps(m, rows.data(), eligible.data(), verdict.data(), extents.data());
            std::printf("ov ");
            for (uint8_t v : verdict) std::printf("%d", v);
            std::printf("\n");
            for (int i = 0; i < m; i++)
                for (int j = 0; j < m; j++)
                    if (verdict[(size_t)i * m + j]) {
                        std::printf("ex %d %d", i, j);
                        for (int k = 0; k < 3; k++) print_f(extents[3 * ((size_t)i * m + j) + k]);
                        std::printf("\n");
                    }
        } else {
            std::fprintf(stderr, "unknown verb %s\n", verb.c_str());
            return 2;
        }
        std::fflush(stdout);
    }
    for (Object* O : loaded) delete O;
    return 0;
}
