// Drives include/eaofusion/ObjectAssociation.h over stand-ins for Object_2D / Object_Map / MapPoint / Frame with the reference's member names and types, from a
// script on stdin.  Linked with object_association_stub.cpp it needs no device (tests/test_object_association_class_cpu.py reads what both print); linked with the
// library itself it is the adapter's GPU test (tests/test_gpu_object_association.py).
//
//   <points>  := <n> then n times: <flag: 0 good, 1 isBad(), 2 out_point> <3 floats as 8-digit hex>
//   <det>     := <class> <points>
//   <mapobj>  := <class> <bBadErase> <mnLastAddID> <points>
//   <frame>   := <mnId> <fx fy cx cy> <16 floats Tcw>
//   input:   single <det> <mapobj>                      -> "ret <NoParaDataAssociation>"
//            cands <det> <k> then k times <mapobj>      -> "ret <NoParaCandidates>", "ids <vObjByNPId, after a planted 777>"
//            rect <frame> <cols> <rows> <mapobj>        -> "ret <r>", "rect <x y w h>" (mRectProject, planted as -1 -2 -3 -4)
//            rects <frame> <cols> <rows> <k> <mapobj>*k -> "ret <r>", then "rect .." per object
#include <cstdio>
#include <cstring>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>

#include <eaofusion/ObjectAssociation.h>

struct Pos {      // what cv::Mat 3x1 CV_32F offers the adapter
    float v[3] = {0, 0, 0};
    template <class T> const T& at(int i) const { return v[i]; }
};
struct Mat44 {
    float v[16];
    template <class T> const T& at(int r, int c) const { return v[4 * r + c]; }
};
struct Rect {
    int x = 0, y = 0, width = 0, height = 0;
    Rect() = default;
    Rect(int x_, int y_, int w_, int h_) : x(x_), y(y_), width(w_), height(h_) {}
};
struct MapPoint {
    Pos pos;
    bool bad = false;
    bool out_point = false;
    bool isBad() const { return bad; }
    Pos GetWorldPos() const { return pos; }
};
struct Object_2D {
    int _class_id = 0;
    std::vector<MapPoint*> Obj_c_MapPonits;
    std::vector<std::unique_ptr<MapPoint>> owned;
};
struct Object_Map {
    int mnClass = 0;
    bool bBadErase = false;
    int mnLastAddID = 0;
    Rect mRectProject = Rect(-1, -2, -3, -4);
    std::vector<MapPoint*> mvpMapObjectMappoints;
    std::vector<std::unique_ptr<MapPoint>> owned;
};
struct Frame {
    long unsigned int mnId = 0;
    float fx = 0, fy = 0, cx = 0, cy = 0;
    Mat44 mTcw;
};

static float read_float(std::istream& in) {
    std::string h;
    in >> h;
    const uint32_t bits = (uint32_t)std::stoul(h, nullptr, 16);
    float f;
    std::memcpy(&f, &bits, 4);
    return f;
}
static void read_points(std::istream& in, std::vector<MapPoint*>& into, std::vector<std::unique_ptr<MapPoint>>& owned) {
    int n;
    in >> n;
    for (int i = 0; i < n; i++) {
        int flag;
        in >> flag;
        owned.emplace_back(new MapPoint);
        owned.back()->bad = flag == 1;
        owned.back()->out_point = flag == 2;
        for (int c = 0; c < 3; c++) owned.back()->pos.v[c] = read_float(in);
        into.push_back(owned.back().get());
    }
}
static void read_det(std::istream& in, Object_2D& d) {
    in >> d._class_id;
    read_points(in, d.Obj_c_MapPonits, d.owned);
}
static void read_map(std::istream& in, Object_Map& o) {
    int erase;
    in >> o.mnClass >> erase >> o.mnLastAddID;
    o.bBadErase = erase != 0;
    read_points(in, o.mvpMapObjectMappoints, o.owned);
}
static void read_frame(std::istream& in, Frame& f) {
    in >> f.mnId;
    f.fx = read_float(in); f.fy = read_float(in); f.cx = read_float(in); f.cy = read_float(in);
    for (int i = 0; i < 16; i++) f.mTcw.v[i] = read_float(in);
}
static void print_rect(const Object_Map& o) { std::printf("rect %d %d %d %d\n", o.mRectProject.x, o.mRectProject.y, o.mRectProject.width, o.mRectProject.height); }

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::string verb;
        in >> verb;
        if (verb == "single") {
            Object_2D d;
            Object_Map o;
            read_det(in, d);
            read_map(in, o);
            std::printf("ret %d\n", eaofusion::NoParaDataAssociation(d, o));
        } else if (verb == "cands") {
            Object_2D d;
            read_det(in, d);
            int k;
            in >> k;
            std::vector<std::unique_ptr<Object_Map>> objs;
            std::vector<Object_Map*> ptrs;
            for (int j = 0; j < k; j++) {
                objs.emplace_back(new Object_Map);
                read_map(in, *objs.back());
                ptrs.push_back(objs.back().get());
            }
            std::vector<int> ids(1, 777);
            std::printf("ret %d\nids", eaofusion::NoParaCandidates(d, ptrs, ids));
            for (int i : ids) std::printf(" %d", i);
            std::printf("\n");
        } else if (verb == "rect" || verb == "rects") {
            Frame f;
            int cols, rows, k = 1;
            read_frame(in, f);
            in >> cols >> rows;
            if (verb == "rects") in >> k;
            std::vector<std::unique_ptr<Object_Map>> objs;
            std::vector<Object_Map*> ptrs;
            for (int j = 0; j < k; j++) {
                objs.emplace_back(new Object_Map);
                read_map(in, *objs.back());
                ptrs.push_back(objs.back().get());
            }
            if (verb == "rect") std::printf("ret %d\n", eaofusion::ComputeProjectRectFrame(*objs[0], f, cols, rows));
            else std::printf("ret %d\n", eaofusion::ComputeProjectRectFrames(ptrs, f, cols, rows));
            for (const auto& o : objs) print_rect(*o);
        } else {
            std::fprintf(stderr, "unknown verb %s\n", verb.c_str());
            return 2;
        }
        std::fflush(stdout);
    }
    return 0;
}
