// Drives the cuboid half of include/eaofusion/ObjectMap.h (ComputeMeanAndStandard, RefineObjects, OverlapMatrix) over a stand-in Object_Map / MapPoint /
// Object_2D with the reference's member names, from a script on stdin.  Linked with object_cuboid_stub.cpp it needs no device
// (tests/test_object_cuboid_class_cpu.py reads what both print); linked with the library itself it is the adapter's GPU test (tests/test_gpu_object_cuboid.py).
// The conversion policy is a recording one: it prints the matrix it receives and keeps it as the "pose".
//
//   an object:  <class> <rotP rotR rotY as hex32> <3 hex64 cuboidCenter> <n> n x (<bad 0/1> <x y z hex32>) <m> m x <x y z hex32>
//   input:   cuboid single <object>        ComputeMeanAndStandard(ObjT&)
//            cuboid batch <k> k x <object> ComputeMeanAndStandard(std::vector<ObjT*>&)
//            refine <biForest> <k> k x <object>
//            overlap <extents 0/1> <k> k x (<3 hex64 cuboidCenter> <lenth width height hex32> <eligible>)
//   output:  "ret <r>", then per object "kept <ids of the points left>" and "members <every member ComputeMeanAndStandard can write: floats as hex32, doubles as
//            hex64; a NaN as nan>"; every member starts as the sentinel 777 (hex32 44424000, hex64 4088480000000000)
#include <cstdio>
#include <cstring>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>

#include <eaofusion/ObjectMap.h>

static float read_f(std::istream& in) {
    std::string h;
    in >> h;
    const uint32_t bits = (uint32_t)std::stoul(h, nullptr, 16);
    float f;
    std::memcpy(&f, &bits, 4);
    return f;
}
static double read_d(std::istream& in) {
    std::string h;
    in >> h;
    const uint64_t bits = (uint64_t)std::stoull(h, nullptr, 16);
    double d;
    std::memcpy(&d, &bits, 8);
    return d;
}
static void print_f(float v) {
    uint32_t bits;
    std::memcpy(&bits, &v, 4);
    if (v != v) std::printf(" nan");
    else std::printf(" %08x", bits);
}
static void print_d(double v) {
    uint64_t bits;
    std::memcpy(&bits, &v, 8);
    if (v != v) std::printf(" nan");
    else std::printf(" %016llx", (unsigned long long)bits);
}

static cv::Mat mat3(float x, float y, float z) {
    cv::Mat m(3, 1, CV_32F);
    m.at<float>(0) = x; m.at<float>(1) = y; m.at<float>(2) = z;
    return m;
}
namespace cv {
inline Mat& operator-=(Mat& a, const Mat& b) {      // (the forest's erase: mSumPointsPos -= pos; found by argument-dependent lookup)
    for (int c = 0; c < 3; c++) a.at<float>(c) -= b.at<float>(c);
    return a;
}
}  // namespace cv

struct Vec3 {      // what Eigen::Vector3d offers the adapter
    double v[3] = {777, 777, 777};
    Vec3() {}
    Vec3(double x, double y, double z) { v[0] = x; v[1] = y; v[2] = z; }
    double& operator[](int i) { return v[i]; }
    const double& operator[](int i) const { return v[i]; }
};
struct Pose {      // what the recording policy makes of a matrix
    float T[16];
    Pose() { for (float& t : T) t = 777; }
};
struct RecordingConverter {
    static Pose toSE3Quat(const cv::Mat& m) {
        Pose p;
        std::printf("conv");
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++) {
                p.T[4 * r + c] = m.at<float>(r, c);
                print_f(p.T[4 * r + c]);
            }
        std::printf("\n");
        return p;
    }
};
struct MapPoint {
    int id;
    bool bad;
    cv::Mat pos;
    cv::Mat GetWorldPos() const { return pos.clone(); }
    bool isBad() const { return bad; }
};
struct Object_2D {
    cv::Mat _Pos;
};
struct Cuboid3D {
    Vec3 corner_1, corner_2, corner_3, corner_4, corner_5, corner_6, corner_7, corner_8;
    Vec3 corner_1_w, corner_2_w, corner_3_w, corner_4_w, corner_5_w, corner_6_w, corner_7_w, corner_8_w;
    float x_min = 777, x_max = 777, y_min = 777, y_max = 777, z_min = 777, z_max = 777;
    Vec3 cuboidCenter;
    float lenth = 777, width = 777, height = 777;
    Pose pose, pose_without_yaw;
    float rotY = 0, rotP = 0, rotR = 0;
    float mfRMax = 777;
};
struct Object_Map {
    int mnClass = 0;
    std::vector<MapPoint*> mvpMapObjectMappoints;
    std::vector<Object_2D*> mObjectFrame;
    std::mutex mMutexMapPoints, mMutex;
    cv::Mat mSumPointsPos = mat3(777, 777, 777), mCenter3D = mat3(777, 777, 777);
    float mStandar_x = 777, mStandar_y = 777, mStandar_z = 777;
    float mCenterStandar_x = 777, mCenterStandar_y = 777, mCenterStandar_z = 777;
    float mCenterStandar = 777;
    Cuboid3D mCuboid3D;
    std::vector<std::unique_ptr<MapPoint>> owned;
    std::vector<std::unique_ptr<Object_2D>> frames;
};

static void read_object(std::istringstream& in, Object_Map& o) {
    int n, m;
    in >> o.mnClass;
    o.mCuboid3D.rotP = read_f(in); o.mCuboid3D.rotR = read_f(in); o.mCuboid3D.rotY = read_f(in);
    for (int c = 0; c < 3; c++) o.mCuboid3D.cuboidCenter[c] = read_d(in);
    in >> n;
    for (int i = 0; i < n; i++) {
        int bad;
        in >> bad;
        const float x = read_f(in), y = read_f(in), z = read_f(in);
        o.owned.emplace_back(new MapPoint{i, bad != 0, mat3(x, y, z)});
        o.mvpMapObjectMappoints.push_back(o.owned.back().get());
    }
    in >> m;
    for (int i = 0; i < m; i++) {
        const float x = read_f(in), y = read_f(in), z = read_f(in);
        o.frames.emplace_back(new Object_2D{mat3(x, y, z)});
        o.mObjectFrame.push_back(o.frames.back().get());
    }
}

static void print_object(const Object_Map& o) {
    std::printf("kept");
    for (const MapPoint* p : o.mvpMapObjectMappoints) std::printf(" %d", p->id);
    std::printf("\nmembers");
    const Cuboid3D& C = o.mCuboid3D;
    for (int c = 0; c < 3; c++) print_f(o.mSumPointsPos.at<float>(c));
    for (int c = 0; c < 3; c++) print_f(o.mCenter3D.at<float>(c));
    print_f(o.mStandar_x); print_f(o.mStandar_y); print_f(o.mStandar_z);
    print_f(o.mCenterStandar_x); print_f(o.mCenterStandar_y); print_f(o.mCenterStandar_z);
    print_f(o.mCenterStandar);
    print_f(C.x_min); print_f(C.x_max); print_f(C.y_min); print_f(C.y_max); print_f(C.z_min); print_f(C.z_max);
    print_f(C.lenth); print_f(C.width); print_f(C.height); print_f(C.mfRMax);
    for (float t : C.pose.T) print_f(t);
    for (float t : C.pose_without_yaw.T) print_f(t);
    for (int c = 0; c < 3; c++) print_d(C.cuboidCenter[c]);
    const Vec3* corners[16] = {&C.corner_1, &C.corner_2, &C.corner_3, &C.corner_4, &C.corner_5, &C.corner_6, &C.corner_7, &C.corner_8,
                               &C.corner_1_w, &C.corner_2_w, &C.corner_3_w, &C.corner_4_w, &C.corner_5_w, &C.corner_6_w, &C.corner_7_w, &C.corner_8_w};
    for (const Vec3* v : corners)
        for (int c = 0; c < 3; c++) print_d((*v)[c]);
    std::printf("\n");
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::string verb;
        in >> verb;
        if (verb == "cuboid") {
            std::string how;
            in >> how;
            if (how == "single") {
                Object_Map o;
                read_object(in, o);
                std::printf("ret %d\n", eaofusion::ComputeMeanAndStandard<RecordingConverter>(o));
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
                std::printf("ret %d\n", eaofusion::ComputeMeanAndStandard<RecordingConverter>(ptrs));
                for (const auto& o : objs) print_object(*o);
            }
        } else if (verb == "refine") {
            int bi, k;
            in >> bi >> k;
            std::vector<std::unique_ptr<Object_Map>> objs;
            std::vector<Object_Map*> ptrs;
            for (int j = 0; j < k; j++) {
                objs.emplace_back(new Object_Map);
                read_object(in, *objs.back());
                ptrs.push_back(objs.back().get());
            }
            std::printf("ret %d\n", eaofusion::RefineObjects<RecordingConverter>(ptrs, bi != 0));
            for (const auto& o : objs) print_object(*o);
        } else if (verb == "overlap") {
            int want, k;
            in >> want >> k;
            std::vector<std::unique_ptr<Object_Map>> objs;
            std::vector<Object_Map*> ptrs;
            std::vector<uint8_t> eligible;
            for (int j = 0; j < k; j++) {
                objs.emplace_back(new Object_Map);
                Cuboid3D& C = objs.back()->mCuboid3D;
                for (int c = 0; c < 3; c++) C.cuboidCenter[c] = read_d(in);
                C.lenth = read_f(in); C.width = read_f(in); C.height = read_f(in);
                int e;
                in >> e;
                eligible.push_back((uint8_t)e);
                ptrs.push_back(objs.back().get());
            }
            std::vector<uint8_t> verdict;
            std::vector<float> extents;
            std::printf("ret %d\n", eaofusion::OverlapMatrix(ptrs, eligible, verdict, want ? &extents : nullptr));
            std::printf("ov ");
            for (uint8_t v : verdict) std::printf("%d", v);
            std::printf("\n");
            for (size_t p = 0; want && p < verdict.size(); p++)
                if (verdict[p]) {
                    std::printf("ex %zu %zu", p / (size_t)k, p % (size_t)k);
                    for (int c = 0; c < 3; c++) print_f(extents[3 * p + c]);
                    std::printf("\n");
                }
        } else {
            std::fprintf(stderr, "unknown verb %s\n", verb.c_str());
            return 2;
        }
        std::fflush(stdout);
    }
    return 0;
}
