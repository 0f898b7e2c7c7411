// Drives include/eaofusion/FrameObjects.h over stand-ins for Frame / MapPoint / Object_2D with the reference's member names and types.  Linked with
// frame_objects_stub.cpp it needs no device (tests/test_frame_objects_class_cpu.py reads what both print); linked with the library itself (and compiled with
// -DFRAME_OBJECTS_DEVICE) it is the adapter's GPU test (tests/test_gpu_frame_objects.py).
//
//   stdin:  one line per frame, as tools/frame_objects_walk.cpp reads it:
//           frame <n_kp> <n_box> <cols> <rows> <fx fy cx cy> <16 floats Tcw> n_kp x (<kp_x kp_y> <mp_id> <x y z>) n_box x (<x y width height> <score>)
//           mp_id -1: mvpMapPoints[i] is NULL; -2: a map point of its own whose isBad() is true; equal ids >= 0: one MapPoint
//   argv:   single | batch   one BuildFrameObjects call per frame | the overload over all frames
//   stdout: per frame "frame <f> ret <r>" (batch: "ret <r>" first, then the frames), "write <map point id> <kp index>" per `feature` assignment in the order
//           they happened, "survivors <original box indices>", per survivor "obj <box> <mCountMappoint> <bOnEdge> <mRectFeaturePoints x4> <sum_pos_3d _Pos
//           mStandar_x/y/z point_center_2d as hex>" and "list <box> <keypoint indices of Obj_c_MapPonits>", "views <map point ids with object_view, ascending>";
//           with -DFRAME_OBJECTS_DEVICE, for the first survivor of at least 20 points, "np <box> <NoParaDataAssociation against a map object of the same points>"
#include <cstdio>
#include <cstring>
#include <iostream>
#include <map>
#include <memory>
#include <set>
#include <sstream>
#include <string>
#include <vector>

#include <eaofusion/FrameObjects.h>
#ifdef FRAME_OBJECTS_DEVICE
#include <eaofusion/ObjectAssociation.h>
#endif

struct MapPoint;
struct Write { int frame, id, keypoint; };
static std::vector<Write> g_writes;      // per `feature` assignment, in the order they happened
struct FeatureSlot {                                   // cv::KeyPoint feature, with a log of its assignments
    cv::KeyPoint kp;
    int owner = -1, frame = -1;
    FeatureSlot& operator=(const cv::KeyPoint& k) {
        kp = k;
        g_writes.push_back(Write{frame, owner, k.class_id});      // (the driver numbers the keypoints in class_id)
        return *this;
    }
};
struct MapPoint {
    cv::Mat pos = cv::Mat::zeros(3, 1, CV_32F);
    bool bad = false, out_point = false, object_view = false;
    int id = -1;
    std::set<int> frame_id;
    FeatureSlot feature;
    bool isBad() const { return bad; }
    cv::Mat GetWorldPos() const { return pos.clone(); }
};
struct Object_2D {
    int _class_id = 0, box = -1;
    float mScore = 0;
    cv::Rect mBoxRect, mRectFeaturePoints = cv::Rect(-1, -2, -3, -4);
    std::vector<MapPoint*> Obj_c_MapPonits;
    cv::Mat _Pos = cv::Mat::zeros(3, 1, CV_32F), sum_pos_3d = cv::Mat::zeros(3, 1, CV_32F);
    float mStandar_x = -1, mStandar_y = -1, mStandar_z = -1;
    int mCountMappoint = -1;
    cv::Point2f point_center_2d;
    bool bOnEdge = false, bad = false;
};
struct Frame {
    int N = 0;
    long unsigned int mnId = 0;
    float fx = 0, fy = 0, cx = 0, cy = 0;
    cv::Mat mTcw = cv::Mat::eye(4, 4, CV_32F);
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<MapPoint*> mvpMapPoints;
    std::vector<std::unique_ptr<MapPoint>> points;
    std::vector<std::unique_ptr<Object_2D>> objects;
    std::vector<Object_2D*> objs_2d;
    int cols = 0, rows = 0;
};
#ifdef FRAME_OBJECTS_DEVICE
struct Object_Map {
    int mnClass = 0, mnLastAddID = 0;
    bool bBadErase = false;
    cv::Rect mRectProject;
    std::vector<MapPoint*> mvpMapObjectMappoints;
};
#endif

static float read_float(std::istream& in) {
    std::string h;
    in >> h;
    const uint32_t bits = (uint32_t)std::stoul(h, nullptr, 16);
    float f;
    std::memcpy(&f, &bits, 4);
    return f;
}
static void print_hex(float v) {
    uint32_t bits;
    std::memcpy(&bits, &v, 4);
    std::printf(" %08x", bits);
}

static void read_frame(std::istream& in, Frame& F, unsigned long id) {
    int n_box;
    in >> F.N >> n_box >> F.cols >> F.rows;
    F.mnId = id;
    F.fx = read_float(in); F.fy = read_float(in); F.cx = read_float(in); F.cy = read_float(in);
    for (int k = 0; k < 16; k++) F.mTcw.at<float>(k / 4, k % 4) = read_float(in);
    std::map<int, MapPoint*> byId;
    for (int i = 0; i < F.N; i++) {
        const float x = read_float(in), y = read_float(in);
        F.mvKeysUn.emplace_back(x, y, 31.f, -1.f, 0.f, 0, i);
        int id_i;
        in >> id_i;
        float p[3];
        for (int a = 0; a < 3; a++) p[a] = read_float(in);
        MapPoint* pMP = nullptr;
        if (id_i != -1 && (id_i < 0 || !byId.count(id_i))) {
            F.points.emplace_back(new MapPoint);
            pMP = F.points.back().get();
            pMP->id = id_i;
            pMP->bad = id_i == -2;
            pMP->feature.owner = id_i;
            pMP->feature.frame = (int)id;
            for (int a = 0; a < 3; a++) pMP->pos.at<float>(a) = p[a];
            if (id_i >= 0) byId[id_i] = pMP;
        } else if (id_i >= 0) {
            pMP = byId[id_i];
        }
        F.mvpMapPoints.push_back(pMP);
    }
    for (int k = 0; k < n_box; k++) {
        F.objects.emplace_back(new Object_2D);
        Object_2D& o = *F.objects.back();
        o.box = k;
        in >> o.mBoxRect.x >> o.mBoxRect.y >> o.mBoxRect.width >> o.mBoxRect.height;
        o.mScore = read_float(in);
        F.objs_2d.push_back(&o);
    }
}

static void report(Frame& F) {
    for (const Write& w : g_writes)
        if (w.frame == (int)F.mnId) std::printf("write %d %d\n", w.id, w.keypoint);
    std::printf("survivors");
    for (const Object_2D* o : F.objs_2d) std::printf(" %d", o->box);
    std::printf("\n");
    for (const Object_2D* o : F.objs_2d) {
        std::printf("obj %d %d %d %d %d %d %d", o->box, o->mCountMappoint, o->bOnEdge ? 1 : 0, o->mRectFeaturePoints.x, o->mRectFeaturePoints.y,
                    o->mRectFeaturePoints.width, o->mRectFeaturePoints.height);
        for (int a = 0; a < 3; a++) print_hex(o->sum_pos_3d.at<float>(a));
        for (int a = 0; a < 3; a++) print_hex(o->_Pos.at<float>(a));
        print_hex(o->mStandar_x); print_hex(o->mStandar_y); print_hex(o->mStandar_z);
        print_hex(o->point_center_2d.x); print_hex(o->point_center_2d.y);
        std::printf("\nlist %d", o->box);
        for (const MapPoint* p : o->Obj_c_MapPonits) {
            int at = -1;      // the first keypoint that holds it
            for (int i = 0; i < F.N && at < 0; i++)
                if (F.mvpMapPoints[(size_t)i] == p) at = i;
            std::printf(" %d", at);
        }
        std::printf("\n");
    }
    std::printf("views");
    std::set<int> seen;
    for (const auto& p : F.points)
        if (p->object_view && p->frame_id.count((int)F.mnId)) seen.insert(p->id);
    for (int v : seen) std::printf(" %d", v);
    std::printf("\n");
#ifdef FRAME_OBJECTS_DEVICE
    for (Object_2D* o : F.objs_2d)
        if (o->Obj_c_MapPonits.size() >= 20) {
            Object_Map m;
            m.mvpMapObjectMappoints = o->Obj_c_MapPonits;
            std::printf("np %d %d\n", o->box, eaofusion::NoParaDataAssociation(*o, m));
            break;
        }
#endif
}

int main(int argc, char** argv) {
    const bool batch = argc > 1 && std::string(argv[1]) == "batch";
    std::vector<std::unique_ptr<Frame>> frames;
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::string verb;
        in >> verb;
        if (verb != "frame") {
            std::fprintf(stderr, "unknown verb %s\n", verb.c_str());
            return 2;
        }
        frames.emplace_back(new Frame);
        read_frame(in, *frames.back(), 100 + frames.size());
    }
    if (batch) {
        std::vector<std::vector<Object_2D*>*> objs;
        std::vector<Frame*> fs;
        for (auto& F : frames) {
            objs.push_back(&F->objs_2d);
            fs.push_back(F.get());
        }
        std::printf("ret %d\n", eaofusion::BuildFrameObjects(objs, fs, frames.empty() ? 0 : frames[0]->cols, frames.empty() ? 0 : frames[0]->rows));
        for (size_t f = 0; f < frames.size(); f++) {
            std::printf("frame %zu\n", f);
            report(*frames[f]);
        }
    } else {
        for (size_t f = 0; f < frames.size(); f++) {
            Frame& F = *frames[f];
            std::printf("frame %zu ret %d\n", f, eaofusion::BuildFrameObjects(F.objs_2d, F, F.cols, F.rows));
            report(F);
        }
    }
    return 0;
}
