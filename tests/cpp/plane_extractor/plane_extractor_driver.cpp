// include/eaofusion/PlaneExtractor.h over stand-in Frame / MapPlane / MapPlanes types (the members upstream's function touches, nothing else), linked with
// plane_extractor_stub.cpp; tests/test_plane_extractor_class_cpu.py reads what is printed.
#include <cstdio>
#include <stdexcept>
#include <vector>

#include <eaofusion/PlaneExtractor.h>

struct PointT { float x, y, z; unsigned rgb; };
struct PointCloud { std::vector<PointT> points; };

struct Frame {
    static float fx, fy, cx, cy;
    unsigned long mnId = 0;
    int plane_num_ = -1;
    std::vector<cv::Mat> mvPlaneCoefficients;
    std::vector<PointCloud> mvBoundaryPoints, mvPlanePoints;
};
float Frame::fx = 500.f, Frame::fy = 501.f, Frame::cx = 20.5f, Frame::cy = 15.25f;

struct MapPlane {
    unsigned long mnId = 0;
    cv::Mat GetWorldPos() {
        cv::Mat m(4, 1, CV_32F);
        for (int i = 0; i < 4; i++) m.at<float>(i, 0) = 0.5f * (i + 1);
        return m;
    }
};
struct MapPlanes {      // stands for eaofusion::MapPlanesT: only handle() is used
    eao_plane_map* handle() const { return (eao_plane_map*)nullptr; }
};

static void show(const Frame& F) {
    printf("frame plane_num_ %d coef", F.plane_num_);
    for (const cv::Mat& c : F.mvPlaneCoefficients) printf(" [%d x %d: %g %g %g %g]", c.rows, c.cols, c.at<float>(0, 0), c.at<float>(1, 0), c.at<float>(2, 0), c.at<float>(3, 0));
    printf(" boundary");
    for (const PointCloud& c : F.mvBoundaryPoints) { printf(" ("); for (const PointT& p : c.points) printf(" %g %g %g", p.x, p.y, p.z); printf(" )"); }
    printf(" points");
    for (const PointCloud& c : F.mvPlanePoints) printf(" %zu", c.points.size());
    printf("\n");
}

int main() {
    cv::Mat big(30, 48, CV_32F);      // a 40 x 30 view into a wider image: the stride is the wider image's
    for (int y = 0; y < 30; y++)
        for (int x = 0; x < 48; x++) big.at<float>(y, x) = 1.f + 0.001f * (y * 48 + x);
    cv::Mat depth = big.roi(0, 0, 40, 30);
    cv::Mat T = cv::Mat::eye(4, 4, CV_32F);
    T.at<float>(0, 1) = 0.125f; T.at<float>(0, 3) = 1.f; T.at<float>(1, 3) = 2.f; T.at<float>(2, 3) = 3.f;
    {
        eaofusion::PlaneExtractor ex;
        Frame F;
        F.mnId = 41;
        ex.ComputePlanesFromPEAC(F, depth);
        show(F);
        Frame G;
        G.mnId = 42;
        G.mvPlaneCoefficients.push_back(cv::Mat::zeros(4, 1, CV_32F));      // what is there stays: upstream appends
        ex.ComputePlanesFromPEAC(G, depth);                                 // the same geometry: no second handle
        show(G);
        MapPlanes planes;
        MapPlane mp;
        mp.mnId = 7;
        ex.Constructed(planes, &mp, 42, 1, T);          // frame plane 1 is the handle's plane 2 (plane 1 was not kept)
        ex.BoundaryUpdated(planes, &mp, 42, 0, T);
        try { ex.Constructed(planes, &mp, 41, 0, T); } catch (const std::runtime_error& e) { printf("threw %s\n", e.what()); }      // the extractor has moved on
        try { ex.Constructed(planes, &mp, 42, 2, T); } catch (const std::runtime_error& e) { printf("threw %s\n", e.what()); }      // two planes were kept
        mp.mnId = 666;
        try { ex.Constructed(planes, &mp, 42, 0, T); } catch (const std::runtime_error& e) { printf("threw %s\n", e.what()); }      // a refused call throws
        depth.at<float>(0, 0) = -1.f;
        Frame H;
        H.mnId = 43;
        try { ex.ComputePlanesFromPEAC(H, depth); } catch (const std::runtime_error& e) { printf("threw %s\n", e.what()); }
        show(H);
        printf("holds %d %d\n", (int)ex.Holds(42), (int)ex.Holds(43));      // a failed run leaves the extractor without a frame
        depth.at<float>(0, 0) = 1.f;
        cv::Mat small(20, 30, CV_32F);
        for (int y = 0; y < 20; y++)
            for (int x = 0; x < 30; x++) small.at<float>(y, x) = 2.f;
        ex.ComputePlanesFromPEAC(H, small);      // another geometry: a new handle, the old one destroyed
        try { ex.ComputePlanesFromPEAC(H, cv::Mat(20, 30, CV_8U)); } catch (const std::runtime_error& e) { printf("threw %s\n", e.what()); }
    }
    Frame F;
    eaofusion::ComputePlanesFromPEAC(F, depth);      // the free function: the calling thread's extractor
    printf("free plane_num_ %d kept %zu\n", F.plane_num_, F.mvPlaneCoefficients.size());
    return 0;
}
