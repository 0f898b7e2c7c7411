// Drives include/eaofusion/ObjectMap.h over a stand-in Object_Map / MapPoint with the reference's member names, from a script on stdin.  Linked with
// object_map_stub.cpp it needs no device (tests/test_object_map_class_cpu.py reads what both print); linked with the library itself it is the adapter's GPU test
// (tests/test_gpu_isolation_forest.py).
//
//   input:   single <biForest> <class> <n> <3n floats as 8-digit hex>
//            batch <biForest> <k> then k times: <class> <n> <3n floats>
//   output:  "ret <r>", then per object "kept <m> <ids of the points left, in order>" and "sum <3 hex32>" (mSumPointsPos)
#include <cstdio>
#include <cstring>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>

#include <eaofusion/ObjectMap.h>

struct Pos {      // what cv::Mat 3x1 CV_32F offers the adapter
    float v[3] = {0, 0, 0};
    template <class T> const T& at(int i) const { return v[i]; }
    Pos& operator-=(const Pos& o) { for (int c = 0; c < 3; c++) v[c] -= o.v[c]; return *this; }
    Pos& operator+=(const Pos& o) { for (int c = 0; c < 3; c++) v[c] += o.v[c]; return *this; }
};
struct MapPoint {
    int id;
    Pos pos;
    Pos GetWorldPos() const { return pos; }
};
struct Object_Map {
    int mnClass = 0;
    std::vector<MapPoint*> mvpMapObjectMappoints;
    std::mutex mMutexMapPoints;
    Pos mSumPointsPos;
    std::vector<std::unique_ptr<MapPoint>> owned;
};

static void read_object(std::istringstream& in, Object_Map& o) {
    int n;
    in >> o.mnClass >> n;
    for (int i = 0; i < n; i++) {
        o.owned.emplace_back(new MapPoint{i, Pos()});
        for (int c = 0; c < 3; c++) {
            std::string h;
            in >> h;
            const uint32_t bits = (uint32_t)std::stoul(h, nullptr, 16);
            std::memcpy(&o.owned.back()->pos.v[c], &bits, 4);
        }
        o.mvpMapObjectMappoints.push_back(o.owned.back().get());
        o.mSumPointsPos += o.owned.back()->pos;
    }
}

static void print_object(const Object_Map& o) {
    std::printf("kept %zu", o.mvpMapObjectMappoints.size());
    for (const MapPoint* p : o.mvpMapObjectMappoints) std::printf(" %d", p->id);
    std::printf("\nsum");
    for (int c = 0; c < 3; c++) {
        uint32_t bits;
        std::memcpy(&bits, &o.mSumPointsPos.v[c], 4);
        std::printf(" %08x", bits);
    }
    std::printf("\n");
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::string verb;
        int bi;
        in >> verb >> bi;
        if (verb == "single") {
            Object_Map o;
            read_object(in, o);
            std::printf("ret %d\n", eaofusion::IsolationForestDeleteOutliers(o, bi != 0));
            print_object(o);
        } else {
            int k;
            in >> k;
            std::vector<std::unique_ptr<Object_Map>> objs;
            std::vector<Object_Map*> ptrs;
            for (int j = 0; j < k; j++) {
                objs.emplace_back(new Object_Map);
                read_object(in, *objs.back());
                ptrs.push_back(objs.back().get());
            }
            std::printf("ret %d\n", eaofusion::IsolationForestDeleteOutliers(ptrs, bi != 0));
            for (const auto& o : objs) print_object(*o);
        }
        std::fflush(stdout);
    }
    return 0;
}
