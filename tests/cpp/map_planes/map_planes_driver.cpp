// include/eaofusion/MapPlanes.h over stand-in Map / Frame / KeyFrame / MapPlane types (the members upstream's loops touch, nothing else), linked with
// map_planes_stub.cpp; tests/test_map_planes_class_cpu.py reads what is printed.
#include <cstdio>
#include <set>
#include <stdexcept>
#include <vector>

#include <eaofusion/MapPlanes.h>

struct Pt { float x, y, z; unsigned rgb; };
struct Cloud { std::vector<Pt> points; };

static cv::Mat col4(float a, float b, float c, float d) {
    cv::Mat m(4, 1, CV_32F);
    m.at<float>(0, 0) = a; m.at<float>(1, 0) = b; m.at<float>(2, 0) = c; m.at<float>(3, 0) = d;
    return m;
}
static cv::Mat pose(float s, float tx) {      // diag(s, s, s, 1) with t = (tx, 2 tx, 3 tx) and a mark off the diagonal, so that a transpose would show
    cv::Mat m = cv::Mat::eye(4, 4, CV_32F);
    for (int i = 0; i < 3; i++) { m.at<float>(i, i) = s; m.at<float>(i, 3) = tx * (i + 1); }
    m.at<float>(0, 1) = 0.125f;
    return m;
}

struct MapPlane {
    unsigned long mnId = 0;
    cv::Mat world;
    cv::Mat GetWorldPos() { return world.clone(); }
};
struct KeyFrame {
    int mnPlaneNum = 0;
    std::vector<cv::Mat> mvPlaneCoefficients;
    std::vector<Cloud> mvBoundaryPoints;
    cv::Mat Tcw;
    cv::Mat GetPose() { return Tcw.clone(); }
};
struct Frame {
    int mnPlaneNum = 0;
    std::vector<cv::Mat> mvPlaneCoefficients;
    std::vector<Cloud> mvBoundaryPoints;
    cv::Mat mTcw;
    std::vector<MapPlane*> mvpMapPlanes;
    bool mbNewPlane = false;
};
struct Map { std::set<MapPlane*> mspMapPlanes; };

static void show(const char* tag, const std::vector<MapPlane*>& v) {
    printf("%s", tag);
    for (MapPlane* p : v) p ? printf(" %lu", p->mnId) : printf(" -");
    printf("\n");
}

int main() {
    eaofusion::MapPlanesT<MapPlane, Frame, KeyFrame> planes;
    MapPlane mp[4];      // one array: the std::set orders by address, which is the array's order, NOT the order of the ids
    const unsigned long ids[4] = {7, 3, 9, 5};
    for (int k = 0; k < 4; k++) { mp[k].mnId = ids[k]; mp[k].world = col4(0, 0, 1, -0.5f * k); }

    KeyFrame kf;
    kf.Tcw = pose(1, 0.25f);
    kf.mvBoundaryPoints = {Cloud{{{9, 9, 9, 0}}}, Cloud{{{1, 2, 3, 0xffffff}, {4, 5, 6, 0}}}};
    planes.Constructed(&mp[0], &kf, 1);
    try {
        planes.Constructed(&mp[0], &kf, 0);
    } catch (const std::runtime_error& e) {
        printf("threw %s\n", e.what());
    }
    Frame fr;
    fr.mTcw = pose(1, 0.5f);
    fr.mvBoundaryPoints = {Cloud{}, Cloud{{{7, 8, 9, 0}}}};
    planes.BoundaryUpdated(&mp[0], fr, 1);
    planes.BoundaryUpdated(&mp[0], fr, 0);      // an empty cloud
    mp[0].world = col4(1, 0, 0, -2);
    planes.WorldPosSet(&mp[0]);

    // AssociatePlanesByBoundary: three frame planes, the slots hold (stale, null, null)
    Map map;
    for (int k = 0; k < 4; k++) map.mspMapPlanes.insert(&mp[3 - k]);
    fr.mnPlaneNum = 3;
    fr.mvPlaneCoefficients = {col4(0, 0, 1, 1), col4(0, 1, 0, 2), col4(1, 0, 0, 3)};
    MapPlane stale;
    stale.mnId = 99;
    fr.mvpMapPlanes = {&stale, &stale, nullptr};
    fr.mbNewPlane = true;
    planes.AssociatePlanesByBoundary(map, fr);
    show("frame", fr.mvpMapPlanes);
    printf("new %d\n", (int)fr.mbNewPlane);
    fr.mvpMapPlanes = {nullptr, nullptr, nullptr};
    planes.AssociatePlanesByBoundary(map, fr, true);
    show("frame", fr.mvpMapPlanes);
    printf("new %d\n", (int)fr.mbNewPlane);

    // SearchMatchedPlanes: the vector's order, an id twice, a stale vpMatched
    kf.mnPlaneNum = 2;
    kf.mvPlaneCoefficients = {col4(0, 0, 1, 4), col4(0, 0, -1, 5)};
    std::vector<MapPlane*> vpPlanes = {&mp[2], &mp[0], &mp[2]}, vpMatched = {&stale, &stale, &stale, &stale};
    planes.SearchMatchedPlanes(&kf, pose(2, 1), vpPlanes, vpMatched, false);
    show("matched", vpMatched);
    planes.SearchMatchedPlanes(&kf, pose(2, 1), std::vector<MapPlane*>(), vpMatched, false);      // no candidates
    show("matched", vpMatched);

    // the batch of SearchAndFuse: three keyframes, the middle one without planes
    KeyFrame kf2, kf3;
    kf2.mnPlaneNum = 0;
    kf3.mnPlaneNum = 1;
    kf3.mvPlaneCoefficients = {col4(0, 1, 0, 6)};
    std::vector<std::vector<MapPlane*>> vv;
    planes.SearchMatchedPlanes(std::vector<KeyFrame*>{&kf, &kf2, &kf3}, std::vector<cv::Mat>{pose(2, 1), pose(3, 1), pose(4, 1)}, vpPlanes, vv);
    for (const auto& v : vv) show("batch", v);

    planes.Erased(&mp[0]);
    planes.Cleared();
    return 0;
}
