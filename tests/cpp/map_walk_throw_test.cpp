// map_walk_throw_test.cpp -- an exception inside the threaded map walk of eaofusion::BundleAdjustment (include/eaofusion/OptimizerImpl.h) reaches the caller.
// A program of its own (tests/test_adapter_walk_throw_cpu.py builds it plain and with -fsanitize=thread and runs it); the library call is replaced by an
// identity result and nothing of the library is linked.
//
//   map_walk_throw_test none      no accessor throws: the call returns, every observation became an edge
//   map_walk_throw_test caller    the observation accessor of a map point of range 0 -- the calling thread's own -- throws std::runtime_error("boom")
//   map_walk_throw_test helper    ... of a map point of the LAST range, which a helper thread walks when there is more than one walk thread
//   map_walk_throw_test both      one of each, with different messages: the one of the lower range arrives
// Each prints "walk_threads N" (the distinct threads that called the accessor; the walk takes hardware_concurrency() / 2 of them, three at most on this
// map) and, where something was thrown, "caught: <what>" from main.  Exit code 0; an exception that escaped a thread would have ended the process.
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <set>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include <eao_fusion.h>

static int g_edges = -1;
static eao_status identity_ba(const eao_ba_problem* p, const eao_ba_planes*, int32_t, const volatile uint8_t*, eao_ba_result* r, float*) {
    g_edges = p->n_edges;
    std::memcpy(r->cam_Tcw, p->cam_Tcw, sizeof(float) * 16 * (size_t)p->n_cams);
    std::memcpy(r->points, p->points, sizeof(float) * 3 * (size_t)p->n_points);
    r->aborted = 0;
    return EAO_OK;
}
extern "C" const char* eao_last_error(void) { return "stub"; }
#define eao_bundle_adjustment_planes identity_ba
#include <eaofusion/OptimizerImpl.h>
#undef eao_bundle_adjustment_planes

// ---- stand-ins with upstream's locking (src/MapPoint.cc, src/KeyFrame.cc): the members BundleAdjustment's template names
static std::mutex g_seenMutex;
static std::set<std::thread::id> g_seen;

struct KeyFrame;
struct MapPoint {
    std::mutex mMutexPos, mMutexFeatures;
    long unsigned int mnId = 0, mnBAGlobalForKF = 0;
    cv::Mat mWorldPos, mPosGBA;
    std::map<KeyFrame*, size_t> mObservations;
    const char* mThrow = nullptr;
    bool isBad() { std::unique_lock<std::mutex> l(mMutexFeatures); std::unique_lock<std::mutex> l2(mMutexPos); return false; }
    cv::Mat GetWorldPos() { std::unique_lock<std::mutex> l(mMutexPos); return mWorldPos.clone(); }
    void SetWorldPos(const cv::Mat& p) { std::unique_lock<std::mutex> l(mMutexPos); p.copyTo(mWorldPos); }
    std::map<KeyFrame*, size_t> GetObservations() {
        { std::unique_lock<std::mutex> l(g_seenMutex); g_seen.insert(std::this_thread::get_id()); }
        if (mThrow) throw std::runtime_error(mThrow);
        std::unique_lock<std::mutex> l(mMutexFeatures);
        return mObservations;
    }
    void UpdateNormalAndDepth() {}
};
struct MapPlane {
    long unsigned int mnId = 0, mnBAGlobalForKF = 0;
    cv::Mat mWorldPos, mPosGBA;
    bool isBad() { return false; }
    cv::Mat GetWorldPos() { return mWorldPos.clone(); }
    void SetWorldPos(const cv::Mat& p) { p.copyTo(mWorldPos); }
    std::map<KeyFrame*, int> GetObservations() { return std::map<KeyFrame*, int>(); }
};
struct KeyFrame {
    std::mutex mMutexPose, mMutexConnections;
    long unsigned int mnId = 0, mnBAGlobalForKF = 0;
    float fx = 500.f, fy = 500.f, cx = 320.f, cy = 240.f, mbf = 40.f;
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvuRight, mvInvLevelSigma2;
    std::vector<cv::Mat> mvPlaneCoefficients;
    cv::Mat Tcw, mTcwGBA;
    bool isBad() { std::unique_lock<std::mutex> l(mMutexConnections); return false; }
    cv::Mat GetPose() { std::unique_lock<std::mutex> l(mMutexPose); return Tcw.clone(); }
    void SetPose(const cv::Mat& T) { std::unique_lock<std::mutex> l(mMutexPose); T.copyTo(Tcw); }
};

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode != "none" && mode != "caller" && mode != "helper" && mode != "both") { std::fprintf(stderr, "usage: %s none|caller|helper|both\n", argv[0]); return 2; }
    const int nKF = 4, nKeys = 8, nPts = 3 * 4096;      // a walk thread per 4096 points
    std::vector<KeyFrame> kfs(nKF);
    std::vector<KeyFrame*> vk;
    for (int c = 0; c < nKF; c++) {
        kfs[c].mnId = (unsigned long)c;
        kfs[c].Tcw = cv::Mat::eye(4, 4, CV_32F);
        for (int i = 0; i < nKeys; i++) { kfs[c].mvKeysUn.push_back(cv::KeyPoint(10.f * i + c, 5.f * i, 31.f)); kfs[c].mvuRight.push_back(-1.f); }
        kfs[c].mvInvLevelSigma2.assign(8, 1.f);
        vk.push_back(&kfs[c]);
    }
    std::vector<MapPoint> pts(nPts);
    std::vector<MapPoint*> vm;
    for (int i = 0; i < nPts; i++) {      // mnId ascending: the sorted order of the walk is this order, range t holds points [nPts t / nWalk, nPts (t + 1) / nWalk)
        pts[i].mnId = (unsigned long)i;
        pts[i].mWorldPos = cv::Mat::zeros(3, 1, CV_32F);
        pts[i].mWorldPos.at<float>(2) = 1.f + 0.001f * i;
        pts[i].mObservations[&kfs[i % nKF]] = (size_t)(i % nKeys);
        vm.push_back(&pts[i]);
    }
    if (mode == "caller") pts[100].mThrow = "boom";
    if (mode == "helper") pts[nPts - 100].mThrow = "boom";
    if (mode == "both") { pts[100].mThrow = "boom in range 0"; pts[nPts - 100].mThrow = "boom in the last range"; }
    const std::vector<MapPlane*> noPlanes;
    bool stop = false;
    try {
        eaofusion::BundleAdjustment(vk, vm, noPlanes, 10, &stop, 0, false);
        std::printf("returned: %d edges\n", g_edges);
    } catch (const std::exception& e) {
        std::printf("caught: %s\n", e.what());
    }
    std::printf("walk_threads %d\n", (int)g_seen.size());
    return 0;
}
