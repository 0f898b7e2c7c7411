// Initializer.h -- Initializer (reference include/Initializer.h, src/Initializer.cc) on top of the C-ABI (eao_initializer_initialize).
//
// The pair list (src/Initializer.cc:49-63), DUtils::Random::SeedRandOnce(0) and the draw loop with its swap-with-back removal (:78-97) stay on the host, restated
// over the reference's member names so that the template instantiates against the real Frame / cv::Mat in a checkout; FindHomography,
// FindFundamental, the choice of the model and ReconstructH / ReconstructF with CheckRT (:99-121 and everything they call) are one call into libeaofusion_hip.so.
//
//   // include/Initializer.h in an EAO-Fusion checkout: the class becomes a using-declaration, src/Tracking.cc compiles unchanged
//   #include <eaofusion/Initializer.h>
//   #include "Thirdparty/DBoW2/DUtils/Random.h"
//   namespace ORB_SLAM2 { using Initializer = eaofusion::InitializerT<Frame, DUtils::Random>; }
//
// The draw stream.  Initialize has no early exit: it always draws 8 * mMaxIterations indices before anything is computed, upstream and here, so the global rand()
// stream equals upstream's always.
//
// What differs from upstream (include/eao_fusion.h states the three deviations of the call): when the model of the branch taken has no hypothesis with a score above
// zero, upstream throws from a product with an empty cv::Mat; here Initialize returns false and leaves its outputs alone.  Fewer than eight matches make upstream's
// draw loop index an empty vector; here the library refuses the problem and Initialize throws std::runtime_error.
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "adapter_detail.h"

namespace eaofusion {

// the arguments upstream passes to ReconstructH / ReconstructF (src/Initializer.cc:116, :118; tests/golden/initializer_constants.json)
constexpr float kInitializerMinParallax = 1.0;
constexpr int kInitializerMinTriangulated = 50;

// RandomT: a class with `static void SeedRandOnce(int)` and `static int RandomInt(int min, int max)` (DUtils::Random in a checkout).
template <class FrameT, class RandomT>
class InitializerT {
    typedef std::pair<int, int> Match;

public:
    // Fix the reference frame
    InitializerT(const FrameT& ReferenceFrame, float sigma = 1.0, int iterations = 200) {
        mK = ReferenceFrame.mK.clone();
        mvKeys1 = ReferenceFrame.mvKeysUn;
        mSigma = sigma;
        mSigma2 = sigma * sigma;
        mMaxIterations = iterations;
    }

    // Computes in parallel a fundamental matrix and a homography; selects a model and tries to recover the motion and the structure from motion
    bool Initialize(const FrameT& CurrentFrame, const std::vector<int>& vMatches12, cv::Mat& R21, cv::Mat& t21, std::vector<cv::Point3f>& vP3D,
                    std::vector<bool>& vbTriangulated) {
        // Reference Frame: 1, Current Frame: 2
        mvKeys2 = CurrentFrame.mvKeysUn;
        mvMatches12.clear();
        mvMatches12.reserve(mvKeys2.size());
        mvbMatched1.resize(mvKeys1.size());
        for (size_t i = 0, iend = vMatches12.size(); i < iend; i++) {
            if (vMatches12[i] >= 0) {
                mvMatches12.push_back(std::make_pair((int)i, vMatches12[i]));
                mvbMatched1[i] = true;
            } else
                mvbMatched1[i] = false;
        }
        const int N = (int)mvMatches12.size();
        if (N < 8) throw std::runtime_error("eaofusion::Initializer: fewer than eight matches");      // (upstream: RandomInt over an empty vector)
        // Generate sets of 8 points for each RANSAC iteration
        std::vector<size_t> vAllIndices;
        vAllIndices.reserve(N);
        std::vector<size_t> vAvailableIndices;
        for (int i = 0; i < N; i++) vAllIndices.push_back(i);
        mvSets = std::vector<std::vector<size_t> >(mMaxIterations, std::vector<size_t>(8, 0));
        RandomT::SeedRandOnce(0);
        for (int it = 0; it < mMaxIterations; it++) {
            vAvailableIndices = vAllIndices;
            // Select a minimum set (the drawn POSITION is overwritten and popped: no repeats -- not the draw of PnPsolver / Sim3Solver, detail::draw_sets)
            for (size_t j = 0; j < 8; j++) {
                int randi = RandomT::RandomInt(0, (int)vAvailableIndices.size() - 1);
                int idx = (int)vAvailableIndices[randi];
                mvSets[it][j] = idx;
                vAvailableIndices[randi] = vAvailableIndices.back();
                vAvailableIndices.pop_back();
            }
        }
        // everything from the two threads of :104-105 to the return of ReconstructH / ReconstructF: one call
        std::vector<float> k1(2 * mvKeys1.size()), k2(2 * mvKeys2.size());
        for (size_t i = 0; i < mvKeys1.size(); i++) { k1[2 * i] = mvKeys1[i].pt.x; k1[2 * i + 1] = mvKeys1[i].pt.y; }
        for (size_t i = 0; i < mvKeys2.size(); i++) { k2[2 * i] = mvKeys2[i].pt.x; k2[2 * i + 1] = mvKeys2[i].pt.y; }
        std::vector<int32_t> m12(2 * (size_t)N), sets(8 * (size_t)mMaxIterations);
        for (int i = 0; i < N; i++) { m12[2 * i] = mvMatches12[i].first; m12[2 * i + 1] = mvMatches12[i].second; }
        for (int it = 0; it < mMaxIterations; it++)
            for (int j = 0; j < 8; j++) sets[8 * (size_t)it + j] = (int32_t)mvSets[it][j];
        eao_initializer_problem p = eao_initializer_problem();
        p.n1 = (int32_t)mvKeys1.size(); p.n2 = (int32_t)mvKeys2.size();
        p.keys1_xy = k1.data(); p.keys2_xy = k2.data();
        p.n_matches = N; p.matches12 = m12.data();
        float K[4];
        detail::read_intrinsics(mK, K);
        p.fx = K[0]; p.fy = K[1]; p.cx = K[2]; p.cy = K[3];
        p.sigma = mSigma;
        p.min_parallax = kInitializerMinParallax;
        p.min_triangulated = kInitializerMinTriangulated;
        std::vector<float> p3d(3 * mvKeys1.size() + 3, 0.f);
        std::vector<uint8_t> tri(mvKeys1.size() + 1, 0);
        eao_initializer_result r = eao_initializer_result();
        r.p3d = p3d.data();
        r.triangulated = tri.data();
        detail::check(eao_initializer_initialize(&p, sets.data(), mMaxIterations, &r), "eao_initializer_initialize");
        mResult = r;
        mResult.p3d = nullptr;
        mResult.triangulated = nullptr;
        if (r.no_model) return false;                                          // (upstream throws here)
        if (r.branch == EAO_INIT_BRANCH_F) { R21 = cv::Mat(); t21 = cv::Mat(); }     // ReconstructF :501-502; ReconstructH leaves them alone unless it returns true
        if (!r.returned) return false;
        detail::mat_of(r.R21, 3, 3).copyTo(R21);
        detail::mat_of(r.t21, 3, 1).copyTo(t21);
        vP3D.resize(mvKeys1.size());
        vbTriangulated = std::vector<bool>(mvKeys1.size(), false);
        for (size_t i = 0; i < mvKeys1.size(); i++) {
            vP3D[i] = cv::Point3f(p3d[3 * i], p3d[3 * i + 1], p3d[3 * i + 2]);
            vbTriangulated[i] = tri[i] != 0;
        }
        return true;
    }

    // what the last call found (not part of the reference's interface; the array pointers are null)
    const eao_initializer_result& LastResult() const { return mResult; }
    const std::vector<Match>& Matches12() const { return mvMatches12; }
    const std::vector<std::vector<size_t> >& Sets() const { return mvSets; }

private:
    std::vector<cv::KeyPoint> mvKeys1;      // Keypoints from Reference Frame (Frame 1)
    std::vector<cv::KeyPoint> mvKeys2;      // Keypoints from Current Frame (Frame 2)
    std::vector<Match> mvMatches12;         // Current Matches from Reference to Current
    std::vector<bool> mvbMatched1;
    cv::Mat mK;                             // Calibration
    float mSigma, mSigma2;                  // Standard Deviation and Variance
    int mMaxIterations;                     // Ransac max iterations
    std::vector<std::vector<size_t> > mvSets;      // Ransac sets
    eao_initializer_result mResult = eao_initializer_result();
};

}  // namespace eaofusion
