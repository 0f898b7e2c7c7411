// Stand-ins of the reference's Frame / MapPoint / DUtils::Random members that include/eaofusion/PnPsolver.h reads, and a driver over them.
//   pnp_solver_driver surface < candidate+script   one candidate; runs the script (params P MIN MAX SET EPS TH2 | iterate N | find) and prints what each call gave
//                                                  back and how many draws it consumed.  Linked with pnp_solver_stub.cpp (records the library calls) in the CPU suite.
//   pnp_solver_driver loop    < candidates         Tracking::Relocalization's loop (src/Tracking.cc:2847-2940, without the matcher steps) over the candidates with a
//                                                  seeded generator; a returned pose goes on to PoseOptimization over its inliers.  Links libeaofusion_hip.so.
// Candidate block (whitespace text): nMatches / fx fy cx cy / 8 level sigma^2 / per match: kind (-1 no map point, 0 good, 1 bad) x y z  u v octave.
#include <cstdio>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

#include <eaofusion/PnPsolver.h>

namespace standin {

// DUtils::Random::RandomInt(min, max), counting its calls: a 64-bit LCG (tests/test_pnp_solver_class_cpu.py restates it)
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

struct MapPoint {
    cv::Mat pos;
    bool bad = false;
    cv::Mat GetWorldPos() { return pos.clone(); }
    bool isBad() { return bad; }
};
struct Frame {
    float fx, fy, cx, cy;
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvLevelSigma2;
};
struct Candidate {
    Frame F;
    std::vector<MapPoint> pool;
    std::vector<MapPoint*> matches;
};

inline void read_candidate(std::istream& in, Candidate& c) {
    int n;
    in >> n >> c.F.fx >> c.F.fy >> c.F.cx >> c.F.cy;
    c.F.mvLevelSigma2.resize(8);
    for (float& s : c.F.mvLevelSigma2) in >> s;
    c.pool.resize(n);
    c.matches.assign(n, nullptr);
    c.F.mvKeysUn.resize(n);
    for (int i = 0; i < n; i++) {
        int kind, octave;
        float x, y, z, u, v;
        in >> kind >> x >> y >> z >> u >> v >> octave;
        c.pool[i].pos = cv::Mat(3, 1, CV_32F);
        c.pool[i].pos.at<float>(0) = x; c.pool[i].pos.at<float>(1) = y; c.pool[i].pos.at<float>(2) = z;
        c.pool[i].bad = kind == 1;
        if (kind >= 0) c.matches[i] = &c.pool[i];
        c.F.mvKeysUn[i] = cv::KeyPoint(u, v, 1.f, -1, 0, octave);
    }
}

}  // namespace standin

using Solver = eaofusion::PnPsolverT<standin::Frame, standin::MapPoint, standin::Random>;

static void print_outcome(const char* what, const cv::Mat& T, bool noMore, const std::vector<bool>& inl, int nInliers, long draws) {
    printf("%s draws %ld nomore %d ninl %d size %zu mat", what, draws, noMore ? 1 : 0, nInliers, inl.size());
    if (T.empty()) printf(" empty");
    else
        for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) printf(" %.9g", T.at<float>(r, c));
    printf(" inliers");
    for (size_t i = 0; i < inl.size(); i++) if (inl[i]) printf(" %zu", i);
    printf("\n");
}

static int surface() {
    standin::Candidate c;
    standin::read_candidate(std::cin, c);
    unsigned long long seed;
    std::cin >> seed;
    standin::Random::Seed(seed);
    Solver s(c.F, c.matches);
    auto header = [&](const char* what) {
        printf("%s n %d min %d maxits %d set %d eps %.9g indices", what, s.Correspondences(), s.MinInliers(), s.MaxIterations(), s.MinSet(), s.Epsilon());
        for (size_t i : s.KeyPointIndices()) printf(" %zu", i);
        printf("\n");
    };
    header("constructed");
    std::string cmd;
    while (std::cin >> cmd) {
        std::vector<bool> inl(3, true);      // (iterate clears it)
        int nInliers = -1;
        bool noMore = false;
        const long before = standin::Random::calls;
        if (cmd == "params") {
            double p; int mi, mx, set; float eps, th2;
            std::cin >> p >> mi >> mx >> set >> eps >> th2;
            s.SetRansacParameters(p, mi, mx, set, eps, th2);
            header("params");
        } else if (cmd == "iterate") {
            int n;
            std::cin >> n;
            const cv::Mat T = s.iterate(n, noMore, inl, nInliers);
            print_outcome("iterate", T, noMore, inl, nInliers, standin::Random::calls - before);
        } else if (cmd == "find") {
            const cv::Mat T = s.find(inl, nInliers);
            print_outcome("find", T, false, inl, nInliers, standin::Random::calls - before);
        }
    }
    return 0;
}

// Relocalization's loop over its candidates (src/Tracking.cc:2816-2940) without the matcher steps: SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991), rounds of
// iterate(5), a candidate with bNoMore is discarded, a returned pose goes to PoseOptimization over its inliers, nGood >= 50 ends the search.
static int loop() {
    int nc;
    unsigned long long seed;
    std::cin >> nc >> seed;
    std::vector<standin::Candidate> cs(nc);
    for (auto& c : cs) standin::read_candidate(std::cin, c);
    standin::Random::Seed(seed);
    std::vector<std::unique_ptr<Solver>> solvers;
    std::vector<bool> discarded(nc, false);
    int nCandidates = 0;
    for (int i = 0; i < nc; i++) {
        solvers.emplace_back(new Solver(cs[i].F, cs[i].matches));
        solvers[i]->SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991);
        nCandidates++;
    }
    bool bMatch = false;
    int round = 0;
    while (nCandidates > 0 && !bMatch && round < 100) {
        round++;
        for (int i = 0; i < nc; i++) {
            if (discarded[i]) continue;
            std::vector<bool> vbInliers;
            int nInliers;
            bool bNoMore;
            const long before = standin::Random::calls;
            const cv::Mat Tcw = solvers[i]->iterate(5, bNoMore, vbInliers, nInliers);
            printf("round %d candidate %d ", round, i);
            print_outcome("iterate", Tcw, bNoMore, vbInliers, nInliers, standin::Random::calls - before);
            if (bNoMore) { discarded[i] = true; nCandidates--; }
            if (!Tcw.empty()) {
                std::vector<float> T(16), Xw, obs, inv;
                for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) T[r * 4 + c] = Tcw.at<float>(r, c);
                for (size_t j = 0; j < vbInliers.size(); j++)
                    if (vbInliers[j]) {
                        for (int k = 0; k < 3; k++) Xw.push_back(cs[i].pool[j].pos.at<float>(k));
                        const cv::KeyPoint& kp = cs[i].F.mvKeysUn[j];
                        obs.push_back(kp.pt.x); obs.push_back(kp.pt.y); obs.push_back(-1.f);
                        inv.push_back(1.0f / cs[i].F.mvLevelSigma2[kp.octave]);
                    }
                eao_pose_problem p = eao_pose_problem();
                p.n = (int)inv.size(); p.Tcw = T.data(); p.Xw = Xw.data(); p.obs = obs.data(); p.inv_sigma2 = inv.data();
                p.fx = cs[i].F.fx; p.fy = cs[i].F.fy; p.cx = cs[i].F.cx; p.cy = cs[i].F.cy; p.bf = 40.f;
                std::vector<uint8_t> outlier(inv.size() + 1, 0);
                eao_pose_result r = eao_pose_result();
                r.outlier = outlier.data();
                if (eao_pose_optimization(&p, &r) != EAO_OK) { fprintf(stderr, "eao_pose_optimization: %s\n", eao_last_error()); return 2; }
                printf("pose candidate %d ngood %d T", i, r.n_inliers);
                for (int k = 0; k < 16; k++) printf(" %.9g", r.Tcw[k]);
                printf("\n");
                if (r.n_inliers < 10) continue;
                if (r.n_inliers >= 50) { bMatch = true; printf("match candidate %d\n", i); break; }
            }
        }
    }
    printf("done match %d rounds %d\n", bMatch ? 1 : 0, round);
    return 0;
}

int main(int argc, char** argv) {
    try {
        if (argc > 1 && std::string(argv[1]) == "loop") return loop();
        return surface();
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
