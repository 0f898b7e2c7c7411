// Sim3Solver.h -- Sim3Solver (reference include/Sim3Solver.h, src/Sim3Solver.cc) on top of the C-ABI (eao_sim3_solver_iterate).
//
// The constructor's walk over the two keyframes (src/Sim3Solver.cc:62-102), SetRansacParameters (:114-138) and the sampling loop (:163-177)
// stay on the host, restated over the reference's member names so that the template instantiates against the real KeyFrame / MapPoint /
// cv::Mat in a checkout; ComputeSim3 and CheckInliers of every hypothesis of an iterate call, and the sequential
// part of its loop, are one call into libeaofusion_hip.so.
//
//   // include/Sim3Solver.h in an EAO-Fusion checkout: the class becomes a using-declaration, src/LoopClosing.cc compiles unchanged
//   #include <eaofusion/Sim3Solver.h>
//   #include "Thirdparty/DBoW2/DUtils/Random.h"
//   namespace ORB_SLAM2 { using Sim3Solver = eaofusion::Sim3SolverT<KeyFrame, MapPoint, DUtils::Random>; }
//
// The draw stream.  iterate(n) draws all 3 * min(n, mRansacMaxIts - mnIterations) indices FIRST and makes one library call.  When that call
// returns a Sim3 at chunk position k, the draws of the rest of the chunk have been consumed; upstream would not have made them.  The global
// rand() stream therefore equals upstream's up to the first successful iterate of the process and may differ afterwards.  (Upstream's stream
// is already shared, unsynchronised, with Tracking's PnPsolver.)  Drawing one iteration per launch would keep the stream and give the launch
// count of the host loop back; it is not offered.  The note of OptimizerSim3.h on running ComputeSim3's candidates together stays true: the
// round-robin over candidates is the caller's (src/LoopClosing.cc:286-311), one iterate(5) per candidate and round.
//
// The sampling loop is restated WITH its quirk (detail::draw_sets, adapter_detail.h): upstream writes vAvailableIndices[idx] = back() with
// idx the drawn VALUE, not the drawn position randi.  After the first draw position a holds N-1; drawing position a again yields N-1, and
// a third time N-1 again -- triples with a repeated index are reachable upstream and here.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "adapter_detail.h"

namespace eaofusion {

// RandomT: a class with `static int RandomInt(int min, int max)` (DUtils::Random in a checkout).
template <class KeyFrameT, class MapPointT, class RandomT>
class Sim3SolverT {
public:
    Sim3SolverT(KeyFrameT* pKF1, KeyFrameT* pKF2, const std::vector<MapPointT*>& vpMatched12, const bool bFixScale = true)
        : mbFixScale(bFixScale) {
        mState = eao_sim3_solver_state();      // mnIterations(0), mnBestInliers(0)
        mpKF1 = pKF1;
        mpKF2 = pKF2;
        const std::vector<MapPointT*> vpKeyFrameMP1 = pKF1->GetMapPointMatches();
        mN1 = (int)vpMatched12.size();
        mT1w.resize(16); mT2w.resize(16);
        detail::read_pose(pKF1->GetRotation(), pKF1->GetTranslation(), mT1w.data());
        detail::read_pose(pKF2->GetRotation(), pKF2->GetTranslation(), mT2w.data());
        for (int i1 = 0; i1 < mN1; i1++) {
            if (!vpMatched12[i1]) continue;
            MapPointT* pMP1 = vpKeyFrameMP1[i1];
            MapPointT* pMP2 = vpMatched12[i1];
            if (!pMP1) continue;
            if (pMP1->isBad() || pMP2->isBad()) continue;
            const int indexKF1 = pMP1->GetIndexInKeyFrame(pKF1);
            const int indexKF2 = pMP2->GetIndexInKeyFrame(pKF2);
            if (indexKF1 < 0 || indexKF2 < 0) continue;
            const auto& kp1 = pKF1->mvKeysUn[indexKF1];
            const auto& kp2 = pKF2->mvKeysUn[indexKF2];
            mvSigma2_1.push_back(pKF1->mvLevelSigma2[kp1.octave]);
            mvSigma2_2.push_back(pKF2->mvLevelSigma2[kp2.octave]);
            mvnIndices1.push_back((size_t)i1);
            detail::push3(pMP1->GetWorldPos(), mvXw1);
            detail::push3(pMP2->GetWorldPos(), mvXw2);
        }
        detail::read_intrinsics(pKF1->mK, mK1);
        detail::read_intrinsics(pKF2->mK, mK2);
        SetRansacParameters();
    }

    void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300) {
        mRansacProb = probability;
        mRansacMinInliers = minInliers;
        mRansacMaxIts = maxIterations;
        N = (int)mvnIndices1.size();
        // N < minInliers: iterate returns before it reads mRansacMaxIts (:146-150), and the formula would convert a NaN or an infinity to int
        if (N >= mRansacMinInliers) {
            const float epsilon = (float)mRansacMinInliers / N;
            int nIterations;
            if (mRansacMinInliers == N) nIterations = 1;
            else nIterations = (int)std::ceil(std::log(1 - mRansacProb) / std::log(1 - std::pow(epsilon, 3)));
            mRansacMaxIts = std::max(1, std::min(nIterations, mRansacMaxIts));
        }
        mState.iterations = 0;
    }

    cv::Mat find(std::vector<bool>& vbInliers12, int& nInliers) {
        bool bFlag;
        return iterate(mRansacMaxIts, bFlag, vbInliers12, nInliers);
    }

    cv::Mat iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers) {
        bNoMore = false;
        vbInliers = std::vector<bool>(mN1, false);
        nInliers = 0;
        if (N < mRansacMinInliers) {
            bNoMore = true;
            return cv::Mat();
        }
        // every draw of the chunk first (see the header comment), then one call
        const int nHyp = std::max(0, std::min(nIterations, mRansacMaxIts - mState.iterations));
        std::vector<int32_t> triples((size_t)nHyp * 3);
        detail::draw_sets<RandomT>(N, 3, nHyp, triples.data());
        const eao_sim3_solver_problem p = problem();
        std::vector<uint8_t> inlier((size_t)N + 1, 0);
        eao_sim3_solver_result r = eao_sim3_solver_result();
        r.inlier = inlier.data();
        detail::check(eao_sim3_solver_iterate(&p, mRansacMinInliers, mRansacMaxIts, &mState, triples.data(), nHyp, &r), "eao_sim3_solver_iterate");
        bNoMore = r.no_more != 0;
        if (r.returned < 0) return cv::Mat();
        nInliers = r.n_inliers;
        for (int i = 0; i < N; i++)
            if (inlier[i]) vbInliers[mvnIndices1[i]] = true;
        return detail::mat_of(r.T12, 4, 4);
    }

    cv::Mat GetEstimatedRotation() { return detail::mat_of(mState.best_R, 3, 3); }
    cv::Mat GetEstimatedTranslation() { return detail::mat_of(mState.best_t, 3, 1); }
    float GetEstimatedScale() { return mState.best_s; }

    // what the flattened problem holds (not part of the reference's interface)
    eao_sim3_solver_problem problem() const {
        eao_sim3_solver_problem p;
        p.n = N;
        p.T1w = mT1w.data(); p.T2w = mT2w.data(); p.Xw1 = mvXw1.data(); p.Xw2 = mvXw2.data();
        p.sigma2_1 = mvSigma2_1.data(); p.sigma2_2 = mvSigma2_2.data();
        p.fx1 = mK1[0]; p.fy1 = mK1[1]; p.cx1 = mK1[2]; p.cy1 = mK1[3];
        p.fx2 = mK2[0]; p.fy2 = mK2[1]; p.cx2 = mK2[2]; p.cy2 = mK2[3];
        p.fix_scale = mbFixScale ? 1 : 0;
        return p;
    }
    const std::vector<size_t>& Indices1() const { return mvnIndices1; }
    int MaxIterations() const { return mRansacMaxIts; }
    int Iterations() const { return mState.iterations; }

protected:
    KeyFrameT* mpKF1;
    KeyFrameT* mpKF2;
    std::vector<float> mT1w, mT2w, mvXw1, mvXw2, mvSigma2_1, mvSigma2_2;
    std::vector<size_t> mvnIndices1;
    float mK1[4], mK2[4];
    int N = 0;          // number of correspondences
    int mN1 = 0;
    bool mbFixScale;
    eao_sim3_solver_state mState;      // mnIterations, mnBestInliers, mBestT12, mBestRotation, mBestTranslation, mBestScale
    double mRansacProb = 0.99;
    int mRansacMinInliers = 6;
    int mRansacMaxIts = 300;
};

}  // namespace eaofusion
