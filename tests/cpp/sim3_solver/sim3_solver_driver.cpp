// Stand-ins of the reference's KeyFrame / MapPoint / DUtils::Random / g2o::Sim3 members that include/eaofusion/Sim3Solver.h (and OptimizerSim3.h) read, and a
// driver over them.
//   sim3_solver_driver surface < scene+script   one candidate; runs the script (params P MIN MAX | iterate N | find) and prints what each call gave back and how
//                                               many draws it consumed.  Linked with sim3_solver_stub.cpp (records the library calls) in the CPU suite.
//   sim3_solver_driver loop    < scenes         LoopClosing::ComputeSim3's loop (src/LoopClosing.cc:286-342, without the matcher steps) over the candidates with a
//                                               seeded generator; a returned Sim3 goes on to eaofusion::OptimizeSim3.  Links libeaofusion_hip.so.
// Scene block (whitespace text): N1 fix / K1[4] K2[4] / T1w[16] T2w[16] / 8 level sigma^2 / nMP, per map point x y z bad index_in_kf1 index_in_kf2 /
// per KF1 entry mp1 match (pool indices or -1) / nk1, per key x y octave / nk2, per key x y octave.
#include <cmath>
#include <cstdio>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

#include <eaofusion/OptimizerSim3.h>
#include <eaofusion/Sim3Solver.h>

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

// DUtils::Random::RandomInt(min, max), counting its calls: a 64-bit LCG (tests/sim3_solver_keyframes.py restates it)
struct Random {
    static unsigned long long state;
    static long calls;
    static void Seed(unsigned long long s) { state = s; calls = 0; }
    static int RandomInt(int min, int max) {
        calls++;
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        return min + (int)((state >> 33) % (unsigned long long)(max - min + 1));
    }
};
unsigned long long Random::state = 1;
long Random::calls = 0;

struct KeyFrame;
struct MapPoint {
    cv::Mat pos;
    bool bad = false;
    int idx1 = -1, idx2 = -1;
    KeyFrame* kf1 = nullptr;
    cv::Mat GetWorldPos() { return pos.clone(); }
    bool isBad() { return bad; }
    int GetIndexInKeyFrame(KeyFrame* kf) { return kf == kf1 ? idx1 : idx2; }
};
struct KeyFrame {
    cv::Mat mK, Tcw;
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvLevelSigma2, mvInvLevelSigma2;
    std::vector<MapPoint*> mvpMapPoints;
    cv::Mat GetRotation() { return Tcw.roi(0, 0, 3, 3).clone(); }
    cv::Mat GetTranslation() { return Tcw.roi(3, 0, 1, 3).clone(); }
    std::vector<MapPoint*> GetMapPointMatches() { return mvpMapPoints; }
};

struct Candidate {
    KeyFrame kf1, kf2;
    std::vector<MapPoint> pool;
    std::vector<MapPoint*> matches;
    int fix = 1;
};

inline void read_candidate(std::istream& in, Candidate& c) {
    int N1;
    in >> N1 >> c.fix;
    for (KeyFrame* kf : {&c.kf1, &c.kf2}) {
        float k[4];
        for (float& v : k) in >> v;
        kf->mK = cv::Mat::eye(3, 3, CV_32F);
        kf->mK.at<float>(0, 0) = k[0]; kf->mK.at<float>(1, 1) = k[1]; kf->mK.at<float>(0, 2) = k[2]; kf->mK.at<float>(1, 2) = k[3];
    }
    for (KeyFrame* kf : {&c.kf1, &c.kf2}) {
        kf->Tcw = cv::Mat(4, 4, CV_32F);
        for (int r = 0; r < 4; r++) for (int col = 0; col < 4; col++) in >> kf->Tcw.at<float>(r, col);
    }
    std::vector<float> sig(8), inv(8);
    for (int k = 0; k < 8; k++) { in >> sig[k]; inv[k] = 1.0f / sig[k]; }
    c.kf1.mvLevelSigma2 = c.kf2.mvLevelSigma2 = sig;
    c.kf1.mvInvLevelSigma2 = c.kf2.mvInvLevelSigma2 = inv;
    int nMP;
    in >> nMP;
    c.pool.resize(nMP);
    for (MapPoint& m : c.pool) {
        m.pos = cv::Mat(3, 1, CV_32F);
        int bad;
        in >> m.pos.at<float>(0) >> m.pos.at<float>(1) >> m.pos.at<float>(2) >> bad >> m.idx1 >> m.idx2;
        m.bad = bad != 0;
        m.kf1 = &c.kf1;
    }
    c.matches.assign(N1, nullptr);
    c.kf1.mvpMapPoints.assign(N1, nullptr);
    for (int i = 0; i < N1; i++) {
        int mp1, mt;
        in >> mp1 >> mt;
        if (mp1 >= 0) c.kf1.mvpMapPoints[i] = &c.pool[mp1];
        if (mt >= 0) c.matches[i] = &c.pool[mt];
    }
    for (KeyFrame* kf : {&c.kf1, &c.kf2}) {
        int nk;
        in >> nk;
        kf->mvKeysUn.resize(nk);
        for (int j = 0; j < nk; j++) in >> kf->mvKeysUn[j].pt.x >> kf->mvKeysUn[j].pt.y >> kf->mvKeysUn[j].octave;
    }
}

// Converter::toMatrix3d + Eigen::Quaterniond(Matrix3d)
inline Quaterniond quat_of(const cv::Mat& R) {
    double m[3][3];
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) m[i][j] = R.at<float>(i, j);
    double t = m[0][0] + m[1][1] + m[2][2];
    if (t > 0) {
        t = std::sqrt(t + 1.0);
        const double w = 0.5 * t;
        t = 0.5 / t;
        return Quaterniond(w, (m[2][1] - m[1][2]) * t, (m[0][2] - m[2][0]) * t, (m[1][0] - m[0][1]) * t);
    }
    int i = 0;
    if (m[1][1] > m[0][0]) i = 1;
    if (m[2][2] > m[i][i]) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    t = std::sqrt(m[i][i] - m[j][j] - m[k][k] + 1.0);
    double q[3];
    q[i] = 0.5 * t;
    t = 0.5 / t;
    const double w = (m[k][j] - m[j][k]) * t;
    q[j] = (m[j][i] + m[i][j]) * t;
    q[k] = (m[k][i] + m[i][k]) * t;
    return Quaterniond(w, q[0], q[1], q[2]);
}

}  // namespace standin

using namespace standin;
using Sim3Solver = eaofusion::Sim3SolverT<KeyFrame, MapPoint, Random>;

static void print_call(const char* what, const cv::Mat& T, bool noMore, const std::vector<bool>& vb, int nInliers, Sim3Solver& s) {
    printf("%s empty %d nomore %d ninliers %d draws %ld iterations %d maxits %d size %zu vb", what, T.empty() ? 1 : 0, noMore ? 1 : 0, nInliers, Random::calls,
           s.Iterations(), s.MaxIterations(), vb.size());
    for (size_t i = 0; i < vb.size(); i++) if (vb[i]) printf(" %zu", i);
    printf("\n");
    if (!T.empty()) {
        printf("T");
        for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) printf(" %.9g", T.at<float>(r, c));
        const cv::Mat R = s.GetEstimatedRotation(), t = s.GetEstimatedTranslation();
        printf("\nbest R00 %.9g t2 %.9g s %.9g rows %d %d\n", R.at<float>(0, 0), t.at<float>(2), s.GetEstimatedScale(), R.rows, t.rows);
    }
}

static int surface() {
    Candidate c;
    read_candidate(std::cin, c);
    unsigned long long seed;
    std::cin >> seed;
    Random::Seed(seed);
    Sim3Solver solver(&c.kf1, &c.kf2, c.matches, c.fix != 0);
    printf("constructed n %d maxits %d indices", solver.problem().n, solver.MaxIterations());
    for (size_t i : solver.Indices1()) printf(" %zu", i);
    printf("\n");
    std::string op;
    while (std::cin >> op) {
        std::vector<bool> vb;
        int nInliers = -1;
        bool noMore = false;
        if (op == "params") {
            double p; int mi, mx;
            std::cin >> p >> mi >> mx;
            solver.SetRansacParameters(p, mi, mx);
            printf("params maxits %d iterations %d\n", solver.MaxIterations(), solver.Iterations());
        } else if (op == "iterate") {
            int n;
            std::cin >> n;
            const cv::Mat T = solver.iterate(n, noMore, vb, nInliers);
            print_call("iterate", T, noMore, vb, nInliers, solver);
        } else if (op == "find") {
            const cv::Mat T = solver.find(vb, nInliers);
            print_call("find", T, false, vb, nInliers, solver);
        }
    }
    return 0;
}

static int loop() {
    int nInitialCandidates;
    unsigned long long seed;
    std::cin >> nInitialCandidates >> seed;
    Random::Seed(seed);
    std::vector<std::unique_ptr<Candidate>> cands;
    std::vector<std::unique_ptr<Sim3Solver>> vpSim3Solvers;
    std::vector<bool> vbDiscarded(nInitialCandidates, false);
    int nCandidates = 0;
    for (int i = 0; i < nInitialCandidates; i++) {
        cands.emplace_back(new Candidate);
        read_candidate(std::cin, *cands.back());
        Candidate& c = *cands.back();
        vpSim3Solvers.emplace_back(new Sim3Solver(&c.kf1, &c.kf2, c.matches, c.fix != 0));
        vpSim3Solvers.back()->SetRansacParameters(0.99, 20, 300);
        nCandidates++;
    }
    bool bMatch = false;
    while (nCandidates > 0 && !bMatch) {
        for (int i = 0; i < nInitialCandidates; i++) {
            if (vbDiscarded[i]) continue;
            Candidate& c = *cands[i];
            std::vector<bool> vbInliers;
            int nInliers;
            bool bNoMore;
            Sim3Solver* pSolver = vpSim3Solvers[i].get();
            cv::Mat Scm = pSolver->iterate(5, bNoMore, vbInliers, nInliers);
            if (bNoMore) {
                vbDiscarded[i] = true;
                nCandidates--;
                printf("candidate%d discarded iterations %d\n", i, pSolver->Iterations());
            }
            if (!Scm.empty()) {
                std::vector<MapPoint*> vpMapPointMatches(c.matches.size(), static_cast<MapPoint*>(nullptr));
                for (size_t j = 0, jend = vbInliers.size(); j < jend; j++)
                    if (vbInliers[j]) vpMapPointMatches[j] = c.matches[j];
                const cv::Mat R = pSolver->GetEstimatedRotation();
                const cv::Mat t = pSolver->GetEstimatedTranslation();
                const float s = pSolver->GetEstimatedScale();
                Sim3 gScm(quat_of(R), Vector3d(t.at<float>(0), t.at<float>(1), t.at<float>(2)), s);
                const int nOpt = eaofusion::OptimizeSim3<MapPoint>(&c.kf1, &c.kf2, vpMapPointMatches, gScm, 10, c.fix != 0);
                if (nOpt >= 20) {
                    bMatch = true;
                    printf("candidate%d match ransac %d optimized %d iterations %d scale %.9g\n", i, nInliers, nOpt, pSolver->Iterations(), gScm.scale());
                    break;
                }
            }
        }
    }
    printf("matched %d draws %ld\n", bMatch ? 1 : 0, Random::calls);
    return 0;
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "surface";
    return mode == "loop" ? loop() : surface();
}
