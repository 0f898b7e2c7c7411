// Stand-ins of the reference's Map / KeyFrame / MapPoint / MapPlane / g2o::Sim3 members that include/eaofusion/OptimizerEssentialGraph.h reads, and a driver over them.
//   essential_graph_driver walk < scene   flattens the scene through WalkEssentialGraph and prints the problem
//   essential_graph_driver run  < scene   (built with -DESSENTIAL_GRAPH_RUN, links libeaofusion_hip.so) calls OptimizeEssentialGraph and prints what it wrote and how often
// Scene (whitespace text): nKF fix_scale loop cur (pool indices) / per keyframe: mnId bad parent(-1) T[16], nLoopEdges ..., nCovisible (keyframe weight) ... by falling weight,
// nChildren ... / nCorrected, per entry: keyframe q[4] t[3] s / nNonCorrected likewise / nLoopConnections, per entry: keyframe count ... /
// nMapPoints, per point: x y z bad mnCorrectedByKF mnCorrectedReference referenceKeyframe / nPlanes, per plane: a b c d bad mnCorrectedByKF mnCorrectedReference referenceKeyframe.
// The keyframes live in one vector, so the pointer order std::map / std::set iterate in is the pool order.
#include <cstdio>
#include <iostream>
#include <map>
#include <mutex>
#include <set>
#include <vector>

#include <eaofusion/OptimizerEssentialGraph.h>

namespace standin {

struct Quaterniond {
    double w_, x_, y_, z_;
    Quaterniond(double w, double x, double y, double z) : w_(w), x_(x), y_(y), z_(z) {}
    double x() const { return x_; }
    double y() const { return y_; }
    double z() const { return z_; }
    double w() const { return w_; }
};
struct Vector3d {
    double v[3];
    Vector3d(double a, double b, double c) : v{a, b, c} {}
    double operator[](int i) const { return v[i]; }
};
struct Sim3 {
    Quaterniond r;
    Vector3d t;
    double s;
    Sim3(const Quaterniond& r_, const Vector3d& t_, double s_) : r(r_), t(t_), s(s_) {}
    const Quaterniond& rotation() const { return r; }
    const Vector3d& translation() const { return t; }
    const double& scale() const { return s; }
};

struct KeyFrame {
    long unsigned int mnId = 0;
    bool bad = false;
    cv::Mat Tcw;
    KeyFrame* parent = nullptr;
    std::set<KeyFrame*> loopEdges, children;
    std::vector<std::pair<KeyFrame*, int> > covisible;      // by falling weight
    int nSetPose = 0;
    bool isBad() { return bad; }
    cv::Mat GetRotation() { return Tcw.roi(0, 0, 3, 3).clone(); }
    cv::Mat GetTranslation() { return Tcw.roi(3, 0, 1, 3).clone(); }
    KeyFrame* GetParent() { return parent; }
    std::set<KeyFrame*> GetLoopEdges() { return loopEdges; }
    bool hasChild(KeyFrame* p) { return children.count(p) != 0; }
    std::vector<KeyFrame*> GetCovisiblesByWeight(const int& w) {
        std::vector<KeyFrame*> out;
        for (auto& c : covisible) if (c.second >= w) out.push_back(c.first);
        return out;
    }
    int GetWeight(KeyFrame* p) {
        for (auto& c : covisible) if (c.first == p) return c.second;
        return 0;
    }
    void SetPose(const cv::Mat& T) { Tcw = T.clone(); nSetPose++; }
};

struct MapPoint {
    cv::Mat pos;
    bool bad = false;
    long unsigned int mnCorrectedByKF = 0, mnCorrectedReference = 0;
    KeyFrame* ref = nullptr;
    int nSetWorldPos = 0, nUpdate = 0;
    bool isBad() { return bad; }
    KeyFrame* GetReferenceKeyFrame() { return ref; }
    cv::Mat GetWorldPos() { return pos.clone(); }
    void SetWorldPos(const cv::Mat& P) { pos = P.clone(); nSetWorldPos++; }
    void UpdateNormalAndDepth() { nUpdate++; }
};
struct MapPlane {      // (no UpdateNormalAndDepth: the plane loop must not call one)
    cv::Mat pos;
    bool bad = false;
    long unsigned int mnCorrectedByKF = 0, mnCorrectedReference = 0;
    KeyFrame* ref = nullptr;
    int nSetWorldPos = 0;
    bool isBad() { return bad; }
    KeyFrame* GetReferenceKeyFrame() { return ref; }
    cv::Mat GetWorldPos() { return pos.clone(); }
    void SetWorldPos(const cv::Mat& P) { pos = P.clone(); nSetWorldPos++; }
};

struct Map {
    std::mutex mMutexMapUpdate;
    std::vector<KeyFrame*> kfs;
    std::vector<MapPoint*> mps;
    std::vector<MapPlane*> planes;
    int nGetAll = 0;      // the three lists are taken once each, before the optimisation (src/Optimizer.cc:1157-1159)
    std::vector<KeyFrame*> GetAllKeyFrames() { nGetAll++; return kfs; }
    std::vector<MapPoint*> GetAllMapPoints() { nGetAll++; return mps; }
    std::vector<MapPlane*> GetAllMapPlanes() { nGetAll++; return planes; }
    long unsigned int GetMaxKFid() { long unsigned int m = 0; for (KeyFrame* k : kfs) m = std::max(m, k->mnId); return m; }
};

}  // namespace standin

using namespace standin;
typedef std::map<KeyFrame*, Sim3> KeyFrameAndPose;

static void read_poses(std::vector<KeyFrame>& pool, KeyFrameAndPose& out) {
    int cnt;
    std::cin >> cnt;
    for (int e = 0; e < cnt; e++) {
        int k;
        double q[4], t[3], s;
        std::cin >> k;
        for (double& v : q) std::cin >> v;
        for (double& v : t) std::cin >> v;
        std::cin >> s;
        out.insert(std::make_pair(&pool[k], Sim3(Quaterniond(q[3], q[0], q[1], q[2]), Vector3d(t[0], t[1], t[2]), s)));
    }
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "walk";
    int nKF, fix, loop, cur;
    std::cin >> nKF >> fix >> loop >> cur;
    std::vector<KeyFrame> pool(nKF);
    for (KeyFrame& kf : pool) {
        int bad, parent, cnt;
        std::cin >> kf.mnId >> bad >> parent;
        kf.bad = bad != 0;
        kf.parent = parent >= 0 ? &pool[parent] : nullptr;
        kf.Tcw = cv::Mat(4, 4, CV_32F);
        for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) std::cin >> kf.Tcw.at<float>(r, c);
        std::cin >> cnt;
        for (int e = 0; e < cnt; e++) { int k; std::cin >> k; kf.loopEdges.insert(&pool[k]); }
        std::cin >> cnt;
        for (int e = 0; e < cnt; e++) { int k, wgt; std::cin >> k >> wgt; kf.covisible.push_back(std::make_pair(&pool[k], wgt)); }
        std::cin >> cnt;
        for (int e = 0; e < cnt; e++) { int k; std::cin >> k; kf.children.insert(&pool[k]); }
    }
    KeyFrameAndPose Corrected, NonCorrected;
    read_poses(pool, Corrected);
    read_poses(pool, NonCorrected);
    std::map<KeyFrame*, std::set<KeyFrame*> > LoopConnections;
    int nLC;
    std::cin >> nLC;
    for (int e = 0; e < nLC; e++) {
        int k, cnt;
        std::cin >> k >> cnt;
        for (int f = 0; f < cnt; f++) { int j; std::cin >> j; LoopConnections[&pool[k]].insert(&pool[j]); }
    }
    int nMP;
    std::cin >> nMP;
    std::vector<MapPoint> mps(nMP);
    for (MapPoint& m : mps) {
        int bad, ref;
        m.pos = cv::Mat(3, 1, CV_32F);
        std::cin >> m.pos.at<float>(0) >> m.pos.at<float>(1) >> m.pos.at<float>(2) >> bad >> m.mnCorrectedByKF >> m.mnCorrectedReference >> ref;
        m.bad = bad != 0; m.ref = &pool[ref];
    }
    int nPl;
    std::cin >> nPl;
    std::vector<MapPlane> planes(nPl);
    for (MapPlane& m : planes) {
        int bad, ref;
        m.pos = cv::Mat(4, 1, CV_32F);
        std::cin >> m.pos.at<float>(0) >> m.pos.at<float>(1) >> m.pos.at<float>(2) >> m.pos.at<float>(3) >> bad >> m.mnCorrectedByKF >> m.mnCorrectedReference >> ref;
        m.bad = bad != 0; m.ref = &pool[ref];
    }
    if (!std::cin) { fprintf(stderr, "short scene\n"); return 3; }
    Map map;
    for (KeyFrame& k : pool) map.kfs.push_back(&k);
    for (MapPoint& m : mps) map.mps.push_back(&m);
    for (MapPlane& m : planes) map.planes.push_back(&m);
    const bool bFixScale = fix != 0;
    if (mode == "walk") {
        const eaofusion::EssentialGraphWalk w = eaofusion::WalkEssentialGraph<MapPoint, MapPlane>(map.GetAllKeyFrames(), map.GetAllMapPoints(), map.GetAllMapPlanes(), &pool[loop], &pool[cur], NonCorrected, Corrected, LoopConnections, bFixScale);
        const eao_essential_graph_problem p = w.problem();
        printf("n %d fixed %d fix_scale %d\nids", p.n, p.fixed, p.fix_scale);
        for (unsigned long id : w.ids) printf(" %lu", id);
        printf("\nedges");
        for (int k = 0; k < p.n_edges; k++) printf(" %d,%d,%d", p.edges[3 * k], p.edges[3 * k + 1], p.edges[3 * k + 2]);
        printf("\nhas_nc");
        for (int v = 0; v < p.n; v++) printf(" %d", p.has_nc[v]);
        printf("\n");
        for (int v = 0; v < p.n; v++) {
            printf("S");
            for (int k = 0; k < 8; k++) printf(" %.17g", p.Scw[8 * v + k]);
            for (int k = 0; k < 8; k++) printf(" %.17g", p.Snc[8 * v + k]);
            printf("\n");
        }
        printf("points %zu planes %zu\nref", w.point_index.size(), w.plane_index.size());
        for (int k = 0; k < p.n_points; k++) printf(" %d", p.ref[k]);
        printf("\nX");
        for (int k = 0; k < 3 * p.n_points; k++) printf(" %.9g", p.Xw[k]);
        printf("\n");
        return 0;
    }
#ifdef ESSENTIAL_GRAPH_RUN
    eaofusion::OptimizeEssentialGraph<MapPoint, MapPlane>(&map, &pool[loop], &pool[cur], NonCorrected, Corrected, LoopConnections, bFixScale);
    for (KeyFrame& k : pool) {
        printf("kf %d", k.nSetPose);
        for (int i = 0; i < 16; i++) printf(" %.9g", k.Tcw.at<float>(i / 4, i % 4));
        printf("\n");
    }
    for (MapPoint& m : mps) printf("mp %d %d %d %.9g %.9g %.9g\n", m.nSetWorldPos, m.nUpdate, m.pos.rows, m.pos.at<float>(0), m.pos.at<float>(1), m.pos.at<float>(2));
    printf("lists %d\n", map.nGetAll);
    for (MapPlane& m : planes) printf("pl %d %d %.9g %.9g %.9g\n", m.nSetWorldPos, m.pos.rows, m.pos.at<float>(0), m.pos.at<float>(1), m.pos.at<float>(2));
    return 0;
#else
    fprintf(stderr, "built without ESSENTIAL_GRAPH_RUN\n");
    return 2;
#endif
}
