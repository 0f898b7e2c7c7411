// Drives DataAssociateUpdate and DataAssociateUpdateChained of include/eaofusion/ObjectMap.h over the same stand-in Object_Map / MapPoint / Object_2D / Frame
// (the reference's member names), from a script on stdin.  Linked with object_chain_stub.cpp it needs no device (tests/test_object_chain_class_cpu.py reads what
// both print); linked with the library itself it is the adapter's GPU test (tests/test_gpu_object_chain.py).
//
//   a point:    <id> <x y z hex32> <count under the object's id, -1 = absent> <have_feature> <feature>      (an id seen before names the same MapPoint; an id of
//               1000 or more is a bad point)
//   an object:  <mnId> <mnClass> <frames in mObjectFrame> <mfRMax hex32> <n> n x <point>
//   input:   dau | chained  <Flag> <biForest> <step2's answer 0/1> <mBox x y w h> <mRectProject.x> <object> <_class_id> <C> C x <point>
//   output:  "step2" where the callable ran, "ret <r>", "list <ids>", "new <ids of mvpMapCurrentNewMappoints>", "sum <mSumPointsPos hex32>", "members <the float
//            members the cuboid writes, hex32>", then per MapPoint in id order "pt <id> <object_id> <object_class> <count, -1 = absent> <have_feature> <feature>"
#include <cstdio>
#include <cstring>
#include <iostream>
#include <map>
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
static void print_f(float v) {
    uint32_t bits;
    std::memcpy(&bits, &v, 4);
    std::printf(" %08x", bits);
}

static cv::Mat mat3(float x, float y, float z) {
    cv::Mat m(3, 1, CV_32F);
    m.at<float>(0) = x; m.at<float>(1) = y; m.at<float>(2) = z;
    return m;
}
namespace cv {
inline Mat& operator-=(Mat& a, const Mat& b) {
    for (int c = 0; c < 3; c++) a.at<float>(c) -= b.at<float>(c);
    return a;
}
}  // namespace cv

struct Vec3 {
    double v[3] = {0, 0, 0};
    Vec3() {}
    Vec3(double x, double y, double z) { v[0] = x; v[1] = y; v[2] = z; }
    double& operator[](int i) { return v[i]; }
    const double& operator[](int i) const { return v[i]; }
};
struct Quat {
    double q[4] = {0.125, -0.25, 0.5, 0.75};
    double x() const { return q[0]; }
    double y() const { return q[1]; }
    double z() const { return q[2]; }
    double w() const { return q[3]; }
};
struct Pose {      // what g2o::SE3Quat offers the adapter
    Quat r;
    Vec3 t = Vec3(1.5, 2.5, 3.5);
    const Quat& rotation() const { return r; }
    const Vec3& translation() const { return t; }
};
struct Converter {
    static Pose toSE3Quat(const cv::Mat&) { return Pose(); }
};
struct MapPoint {
    int id = 0;
    cv::Mat pos;
    int object_id = -1, object_class = -1;
    std::map<int, int> object_id_vector;
    bool have_feature = false;
    int feature = 0;      // (a descriptor upstream; anything assignable)
    cv::Mat GetWorldPos() const { return pos.clone(); }
    bool isBad() const { return id >= 1000; }      // (an id of 1000 or more names a bad point)
};
struct Rect {
    int x = 0, y = 0, width = 0, height = 0;
};
struct Object_2D {
    int _class_id = 0;
    std::vector<MapPoint*> Obj_c_MapPonits;
    Rect mBox, mBoxRect;
    cv::Mat _Pos = mat3(0, 0, 0);
};
struct Cuboid3D {
    Vec3 corner_1, corner_2, corner_3, corner_4, corner_5, corner_6, corner_7, corner_8;
    Vec3 corner_1_w, corner_2_w, corner_3_w, corner_4_w, corner_5_w, corner_6_w, corner_7_w, corner_8_w;
    float x_min = 0, x_max = 0, y_min = 0, y_max = 0, z_min = 0, z_max = 0;
    Vec3 cuboidCenter;
    float lenth = 2.5f, width = 3.5f, height = 4.5f;
    Pose pose, pose_without_yaw;
    float rotY = 0, rotP = 0, rotR = 0;
    float mfRMax = 0;
};
struct Object_Map {
    int mnId = 0, mnClass = 0;
    std::vector<MapPoint*> mvpMapObjectMappoints, mvpMapCurrentNewMappoints;
    std::vector<Object_2D*> mObjectFrame;
    std::mutex mMutexMapPoints, mMutex;
    cv::Mat mSumPointsPos = mat3(0, 0, 0), mCenter3D = mat3(0.25f, 0.5f, 0.75f);
    float mStandar_x = 0, mStandar_y = 0, mStandar_z = 0, mCenterStandar_x = 0, mCenterStandar_y = 0, mCenterStandar_z = 0, mCenterStandar = 0;
    Cuboid3D mCuboid3D;
    Rect mRectProject;
    std::vector<std::unique_ptr<Object_2D>> frames;
};
struct Frame {
    cv::Mat mTcw = cv::Mat(4, 4, CV_32F);
    float fx = 500, fy = 501, cx = 320, cy = 240;
    Frame() {
        const float T[16] = {1, 0, 0, 0.5f, 0, 1, 0, -0.25f, 0, 0, 1, 2.0f, 0, 0, 0, 1};      // a camera two units in front of the origin
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++) mTcw.at<float>(r, c) = T[4 * r + c];
    }
};
struct Image {
    int cols = 640, rows = 480;
};

static std::map<int, std::unique_ptr<MapPoint>> g_points;

static MapPoint* read_point(std::istream& in, int objectId) {
    int id, count, have, feature;
    in >> id;
    const float x = read_f(in), y = read_f(in), z = read_f(in);
    in >> count >> have >> feature;
    auto it = g_points.find(id);
    if (it != g_points.end()) return it->second.get();      // the same MapPoint again
    std::unique_ptr<MapPoint> p(new MapPoint);
    p->id = id;
    p->pos = mat3(x, y, z);
    if (count >= 0) p->object_id_vector[objectId] = count;
    p->have_feature = have != 0;
    p->feature = feature;
    MapPoint* raw = p.get();
    g_points[id] = std::move(p);
    return raw;
}

static void read_object(std::istream& in, Object_Map& o) {
    int frames, n;
    in >> o.mnId >> o.mnClass >> frames;
    o.mCuboid3D.mfRMax = read_f(in);
    for (int i = 0; i < frames; i++) {
        o.frames.emplace_back(new Object_2D);
        o.mObjectFrame.push_back(o.frames.back().get());
    }
    in >> n;
    for (int i = 0; i < n; i++) o.mvpMapObjectMappoints.push_back(read_point(in, o.mnId));
    float s[3] = {0, 0, 0};
    for (MapPoint* p : o.mvpMapObjectMappoints)
        for (int a = 0; a < 3; a++) s[a] += p->pos.at<float>(a);
    o.mSumPointsPos = mat3(s[0], s[1], s[2]);
}

static void print_state(int ret, const Object_Map& o) {
    std::printf("ret %d\nlist", ret);
    for (MapPoint* p : o.mvpMapObjectMappoints) std::printf(" %d", p->id);
    std::printf("\nnew");
    for (MapPoint* p : o.mvpMapCurrentNewMappoints) std::printf(" %d", p->id);
    std::printf("\nsum");
    for (int a = 0; a < 3; a++) print_f(o.mSumPointsPos.at<float>(a));
    std::printf("\n");
    for (const auto& kv : g_points) {
        const MapPoint& p = *kv.second;
        const auto it = p.object_id_vector.find(o.mnId);
        std::printf("pt %d %d %d %d %d %d\n", p.id, p.object_id, p.object_class, it == p.object_id_vector.end() ? -1 : it->second, p.have_feature ? 1 : 0, p.feature);
    }
}

static void print_members(const Object_Map& o) {
    std::printf("members");
    for (int a = 0; a < 3; a++) print_f(o.mCenter3D.at<float>(a));
    print_f(o.mStandar_x); print_f(o.mStandar_y); print_f(o.mStandar_z);
    print_f(o.mCenterStandar_x); print_f(o.mCenterStandar_y); print_f(o.mCenterStandar_z); print_f(o.mCenterStandar);
    const Cuboid3D& C = o.mCuboid3D;
    print_f(C.x_min); print_f(C.x_max); print_f(C.y_min); print_f(C.y_max); print_f(C.z_min); print_f(C.z_max);
    print_f(C.lenth); print_f(C.width); print_f(C.height); print_f(C.mfRMax);
    for (int a = 0; a < 3; a++) print_f((float)C.cuboidCenter[a]);
    for (int a = 0; a < 3; a++) print_f((float)C.corner_1[a]);
    for (int a = 0; a < 3; a++) print_f((float)C.corner_8_w[a]);
    std::printf(" frames %d\n", (int)o.mObjectFrame.size());
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        g_points.clear();
        std::istringstream in(line);
        std::string verb;
        in >> verb;
        if (verb != "dau" && verb != "chained") {
            std::fprintf(stderr, "unknown verb %s\n", verb.c_str());
            return 2;
        }
        Object_Map o;
        int Flag, bi, ok, C;
        Object_2D f;
        in >> Flag >> bi >> ok >> f.mBox.x >> f.mBox.y >> f.mBox.width >> f.mBox.height >> o.mRectProject.x;
        o.mRectProject.y = 2; o.mRectProject.width = 3; o.mRectProject.height = 4;
        f.mBoxRect = f.mBox;
        f._Pos = mat3(0.5f, 0.25f, 1.5f);
        read_object(in, o);
        in >> f._class_id >> C;
        for (int j = 0; j < C; j++) f.Obj_c_MapPonits.push_back(read_point(in, o.mnId));
        Frame frame;
        Image image;
        auto step2 = [&] {
            std::printf("step2\n");
            if (ok) o.mObjectFrame.push_back(&f);      // :1451
            return ok != 0;
        };
        const int r = verb == "dau" ? eaofusion::DataAssociateUpdate<Converter>(o, &f, frame, image, Flag, bi != 0, step2)
                                    : eaofusion::DataAssociateUpdateChained<Converter>(o, &f, frame, image, Flag, bi != 0, step2);
        print_state(r, o);
        print_members(o);
        std::fflush(stdout);
    }
    return 0;
}
