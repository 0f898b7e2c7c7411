// PnPsolver.h -- PnPsolver (reference include/PnPsolver.h, src/PnPsolver.cc) on top of the C-ABI (eao_pnp_solver_iterate).
//
// The constructor's walk over the frame's matches with its two filters (src/PnPsolver.cc:67-110), SetRansacParameters (:121-157) and the sampling loop
// (:188-201) stay on the host, restated over the reference's member names so that the template instantiates against the real Frame / MapPoint / cv::Mat in a
// checkout; compute_pose and CheckInliers of every hypothesis of an iterate call, Refine of every record and the sequential part of
// the loop are one call into libeaofusion_hip.so.
//
//   // include/PnPsolver.h in an EAO-Fusion checkout: the class becomes a using-declaration, src/Tracking.cc compiles unchanged
//   #include <eaofusion/PnPsolver.h>
//   #include "Thirdparty/DBoW2/DUtils/Random.h"
//   namespace ORB_SLAM2 { using PnPsolver = eaofusion::PnPsolverT<Frame, MapPoint, DUtils::Random>; }
//
// The loop count.  Upstream's loop is `while(mnIterations<mRansacMaxIts || nCurrentIterations<nIterations)` (:182) -- note the ||: iterate(n) makes
// max(n, mRansacMaxIts - mnIterations) passes, so the first iterate(5) of Relocalization runs all of its mRansacMaxIts hypotheses.  Kept.
//
// The draw stream.  iterate draws all min_set * passes indices FIRST, through the draw source Sim3SolverT uses, and makes one library call.  When that call
// returns at chunk position k, the draws of the rest of the chunk have been consumed; upstream would not have made them (Sim3Solver.h).
//
// The sampling loop is restated WITH its quirk (detail::draw_sets, adapter_detail.h): vAvailableIndices[idx] = vAvailableIndices.back() uses the drawn VALUE
// idx, not the drawn position randi (:199), so a set with a repeated index is reachable upstream and here.
//
// SetRansacParameters is restated as written, with the float / int conversions of :134-152.  One guard: with N < mRansacMinInliers the epsilon exceeds 1, the
// logarithm is a NaN and its conversion to int is undefined upstream; iterate leaves through N < mRansacMinInliers before the value matters.  Here a value
// that does not fit an int becomes INT_MIN (what x86 produces), so mRansacMaxIts becomes 1.
#pragma once

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "adapter_detail.h"

namespace eaofusion {

// RandomT: a class with `static int RandomInt(int min, int max)` (DUtils::Random in a checkout).
template <class FrameT, class MapPointT, class RandomT>
class PnPsolverT {
public:
    PnPsolverT(const FrameT& F, const std::vector<MapPointT*>& vpMapPointMatches) {
        mState = eao_pnp_solver_state();      // mnIterations(0), mnBestInliers(0)
        mnMatches = vpMapPointMatches.size();
        for (size_t i = 0, iend = vpMapPointMatches.size(); i < iend; i++) {
            MapPointT* pMP = vpMapPointMatches[i];
            if (pMP) {
                if (!pMP->isBad()) {
                    const auto& kp = F.mvKeysUn[i];
                    mvP2D.push_back(kp.pt.x);
                    mvP2D.push_back(kp.pt.y);
                    mvSigma2.push_back(F.mvLevelSigma2[kp.octave]);
                    detail::push3(pMP->GetWorldPos(), mvP3Dw);
                    mvKeyPointIndices.push_back(i);
                }
            }
        }
        fu = F.fx;
        fv = F.fy;
        uc = F.cx;
        vc = F.cy;
        SetRansacParameters();
    }

    void SetRansacParameters(double probability = 0.99, int minInliers = 8, int maxIterations = 300, int minSet = 4, float epsilon = 0.4, float th2 = 5.991) {
        mRansacProb = probability;
        mRansacMinInliers = minInliers;
        mRansacMaxIts = maxIterations;
        mRansacEpsilon = epsilon;
        mRansacMinSet = minSet;
        N = (int)mvSigma2.size();      // number of correspondences
        // Adjust Parameters according to number of correspondences
        int nMinInliers = N * mRansacEpsilon;
        if (nMinInliers < mRansacMinInliers) nMinInliers = mRansacMinInliers;
        if (nMinInliers < minSet) nMinInliers = minSet;
        mRansacMinInliers = nMinInliers;
        if (mRansacEpsilon < (float)mRansacMinInliers / N) mRansacEpsilon = (float)mRansacMinInliers / N;
        // Set RANSAC iterations according to probability, epsilon, and max iterations
        int nIterations;
        if (mRansacMinInliers == N) nIterations = 1;
        else {
            const double v = std::ceil(std::log(1 - mRansacProb) / std::log(1 - std::pow(mRansacEpsilon, 3)));
            nIterations = (v >= -2147483648.0 && v <= 2147483647.0) ? (int)v : INT_MIN;      // (the guard of the header comment; a NaN fails both comparisons)
        }
        mRansacMaxIts = std::max(1, std::min(nIterations, mRansacMaxIts));
        mRansacTh2 = th2;      // mvMaxError[i] = mvSigma2[i]*th2 is formed inside the library call, in float
    }

    cv::Mat find(std::vector<bool>& vbInliers, int& nInliers) {
        bool bFlag;
        return iterate(mRansacMaxIts, bFlag, vbInliers, nInliers);
    }

    cv::Mat iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers) {
        bNoMore = false;
        vbInliers.clear();
        nInliers = 0;
        if (N < mRansacMinInliers) {
            bNoMore = true;
            return cv::Mat();
        }
        std::vector<int32_t> sets;
        const int nHyp = draw(nIterations, sets);
        if (mBestInlier.size() != (size_t)N + 1) mBestInlier.assign((size_t)N + 1, 0);
        mState.best_inlier = mBestInlier.data();
        const eao_pnp_solver_problem p = problem();
        std::vector<uint8_t> inlier((size_t)N + 1, 0);
        eao_pnp_solver_result r = eao_pnp_solver_result();
        r.inlier = inlier.data();
        detail::check(eao_pnp_solver_iterate(&p, mRansacMinInliers, mRansacMaxIts, mRansacMinSet, &mState, sets.data(), nHyp, &r), "eao_pnp_solver_iterate");
        return collect(r, inlier, bNoMore, vbInliers, nInliers);
    }

    // ---- not part of the reference's interface: the pieces of iterate, for a caller that batches Relocalization's candidates
    // the passes of the loop of :182 and their draws; returns the number of passes
    int draw(int nIterations, std::vector<int32_t>& sets) {
        const int nHyp = std::max(nIterations, mRansacMaxIts - mState.iterations);      // the || of :182
        sets.assign((size_t)std::max(nHyp, 0) * mRansacMinSet, 0);
        detail::draw_sets<RandomT>(N, mRansacMinSet, nHyp, sets.data());
        return std::max(nHyp, 0);
    }
    cv::Mat collect(const eao_pnp_solver_result& r, const std::vector<uint8_t>& inlier, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers) {
        bNoMore = r.no_more != 0;
        vbInliers.clear();
        nInliers = 0;
        if (r.returned < 0) return cv::Mat();
        nInliers = r.n_inliers;
        vbInliers = std::vector<bool>(mnMatches, false);
        for (int i = 0; i < N; i++)
            if (inlier[i]) vbInliers[mvKeyPointIndices[i]] = true;
        return detail::mat_of(r.Tcw, 4, 4);
    }
    eao_pnp_solver_problem problem() const {
        eao_pnp_solver_problem p;
        p.n = N;
        p.p3d_w = mvP3Dw.data(); p.p2d = mvP2D.data(); p.sigma2 = mvSigma2.data();
        p.fx = fu; p.fy = fv; p.cx = uc; p.cy = vc;
        p.th2 = mRansacTh2;
        return p;
    }
    eao_pnp_solver_state* State() {
        if (mBestInlier.size() != (size_t)N + 1) mBestInlier.assign((size_t)N + 1, 0);
        mState.best_inlier = mBestInlier.data();
        return &mState;
    }
    const std::vector<size_t>& KeyPointIndices() const { return mvKeyPointIndices; }
    int Correspondences() const { return N; }
    int MinInliers() const { return mRansacMinInliers; }
    int MaxIterations() const { return mRansacMaxIts; }
    int MinSet() const { return mRansacMinSet; }
    float Epsilon() const { return mRansacEpsilon; }
    int Iterations() const { return mState.iterations; }

protected:
    std::vector<float> mvP2D, mvP3Dw, mvSigma2;
    std::vector<size_t> mvKeyPointIndices;
    size_t mnMatches = 0;      // mvpMapPointMatches.size()
    float fu, fv, uc, vc;      // F.fx .. F.cy (floats there; the library widens them as upstream's double members do)
    int N = 0;
    eao_pnp_solver_state mState;      // mnIterations, mnBestInliers, mBestTcw, mvbBestInliers
    std::vector<uint8_t> mBestInlier;
    double mRansacProb = 0.99;
    int mRansacMinInliers = 8;
    int mRansacMaxIts = 300;
    float mRansacEpsilon = 0.4f;
    float mRansacTh2 = 5.991f;
    int mRansacMinSet = 4;
};

}  // namespace eaofusion
