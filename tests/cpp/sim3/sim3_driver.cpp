// Stand-ins of the reference's KeyFrame / MapPoint / g2o::Sim3 members that include/eaofusion/OptimizerSim3.h reads, and a driver over them.
//   sim3_driver walk  < scene   flattens the scene through WalkSim3 and prints the problem, then writes a fixed Sim3 back through WriteSim3
//   sim3_driver run   < scene   (built with -DSIM3_RUN, links libeaofusion_hip.so) calls OptimizeSim3 and prints what it changed
// Scene (whitespace text): N1 N2 / K1[4] K2[4] / T1w[16] T2w[16] / q[4] t[3] s th2 fix / nMP, per map point x y z bad index_in_kf2 /
// per KF1 keypoint x y octave mp1 match (pool indices or -1) / per KF2 keypoint x y octave / 8 inverse level sigma^2.
#include <cstdio>
#include <iostream>
#include <vector>

#include <eaofusion/OptimizerSim3.h>

namespace standin {

struct Quaterniond {   // Eigen's constructor order (w, x, y, z), accessors x() .. w()
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

struct KeyFrame;
struct MapPoint {
    cv::Mat pos;
    bool bad = false;
    int idx2 = -1;
    cv::Mat GetWorldPos() { return pos.clone(); }
    bool isBad() { return bad; }
    int GetIndexInKeyFrame(KeyFrame*) { return idx2; }
};
struct KeyFrame {
    cv::Mat mK, Tcw;
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvInvLevelSigma2;
    std::vector<MapPoint*> mvpMapPoints;
    cv::Mat GetRotation() { return Tcw.roi(0, 0, 3, 3).clone(); }
    cv::Mat GetTranslation() { return Tcw.roi(3, 0, 1, 3).clone(); }
    std::vector<MapPoint*> GetMapPointMatches() { return mvpMapPoints; }
};

}  // namespace standin

using namespace standin;

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "walk";
    int N1, N2;
    std::cin >> N1 >> N2;
    KeyFrame kf1, kf2;
    for (KeyFrame* kf : {&kf1, &kf2}) {
        float k[4];
        for (float& v : k) std::cin >> v;
        kf->mK = cv::Mat::eye(3, 3, CV_32F);
        kf->mK.at<float>(0, 0) = k[0]; kf->mK.at<float>(1, 1) = k[1]; kf->mK.at<float>(0, 2) = k[2]; kf->mK.at<float>(1, 2) = k[3];
    }
    for (KeyFrame* kf : {&kf1, &kf2}) {
        kf->Tcw = cv::Mat(4, 4, CV_32F);
        for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) std::cin >> kf->Tcw.at<float>(r, c);
    }
    double q[4], t[3], s;
    float th2;
    int fix;
    for (double& v : q) std::cin >> v;
    for (double& v : t) std::cin >> v;
    std::cin >> s >> th2 >> fix;
    int nMP;
    std::cin >> nMP;
    std::vector<MapPoint> pool(nMP);
    for (MapPoint& m : pool) {
        m.pos = cv::Mat(3, 1, CV_32F);
        int bad;
        std::cin >> m.pos.at<float>(0) >> m.pos.at<float>(1) >> m.pos.at<float>(2) >> bad >> m.idx2;
        m.bad = bad != 0;
    }
    std::vector<MapPoint*> matches(N1, nullptr);
    kf1.mvpMapPoints.assign(N1, nullptr);
    kf1.mvKeysUn.resize(N1);
    for (int i = 0; i < N1; i++) {
        int mp1, mt;
        std::cin >> kf1.mvKeysUn[i].pt.x >> kf1.mvKeysUn[i].pt.y >> kf1.mvKeysUn[i].octave >> mp1 >> mt;
        if (mp1 >= 0) kf1.mvpMapPoints[i] = &pool[mp1];
        if (mt >= 0) matches[i] = &pool[mt];
    }
    kf2.mvKeysUn.resize(N2);
    for (int j = 0; j < N2; j++) std::cin >> kf2.mvKeysUn[j].pt.x >> kf2.mvKeysUn[j].pt.y >> kf2.mvKeysUn[j].octave;
    std::vector<float> inv(8);
    for (float& v : inv) std::cin >> v;
    kf1.mvInvLevelSigma2 = kf2.mvInvLevelSigma2 = inv;
    Sim3 S(Quaterniond(q[3], q[0], q[1], q[2]), Vector3d(t[0], t[1], t[2]), s);
    std::vector<MapPoint*> before = matches;
    if (mode == "walk") {
        const eaofusion::Sim3Walk w = eaofusion::WalkSim3<MapPoint>(&kf1, &kf2, matches, S, th2, fix != 0);
        const eao_sim3_problem p = w.problem();
        printf("n %d\nindex", p.n);
        for (int i : w.index) printf(" %d", i);
        printf("\nT1w"); for (int k = 0; k < 16; k++) printf(" %.9g", p.T1w[k]);
        printf("\nT2w"); for (int k = 0; k < 16; k++) printf(" %.9g", p.T2w[k]);
        printf("\nK %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g\n", p.fx1, p.fy1, p.cx1, p.cy1, p.fx2, p.fy2, p.cx2, p.cy2);
        printf("S %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.9g %d\n", p.q[0], p.q[1], p.q[2], p.q[3], p.t[0], p.t[1], p.t[2], p.s, p.th2, p.fix_scale);
        for (int k = 0; k < p.n; k++)
            printf("c %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g\n", p.Xw1[3 * k], p.Xw1[3 * k + 1], p.Xw1[3 * k + 2], p.Xw2[3 * k],
                   p.Xw2[3 * k + 1], p.Xw2[3 * k + 2], p.obs1[2 * k], p.obs1[2 * k + 1], p.obs2[2 * k], p.obs2[2 * k + 1], p.inv_sigma2_1[k], p.inv_sigma2_2[k]);
        const double wq[4] = {0.1, -0.2, 0.3, 0.9}, wt[3] = {1.5, -2.5, 3.5};
        eaofusion::WriteSim3(S, wq, wt, 1.25);
        printf("written %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", S.rotation().x(), S.rotation().y(), S.rotation().z(), S.rotation().w(),
               S.translation()[0], S.translation()[1], S.translation()[2], S.scale());
        return 0;
    }
#ifdef SIM3_RUN
    const int nIn = eaofusion::OptimizeSim3<MapPoint>(&kf1, &kf2, matches, S, th2, fix != 0);
    printf("ret %d\nnulled", nIn);
    for (int i = 0; i < N1; i++) if (before[i] && !matches[i]) printf(" %d", i);
    printf("\nS %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", S.rotation().x(), S.rotation().y(), S.rotation().z(), S.rotation().w(),
           S.translation()[0], S.translation()[1], S.translation()[2], S.scale());
    return 0;
#else
    fprintf(stderr, "built without SIM3_RUN\n");
    return 2;
#endif
}
