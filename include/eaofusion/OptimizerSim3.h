// OptimizerSim3.h -- Optimizer::OptimizeSim3 (reference src/Optimizer.cc:1437-1632) on top of the C-ABI (eao_optimize_sim3).
//
// The walk over the two keyframes (src/Optimizer.cc:1486-1561) stays on the host, restated over the reference's member names so that the
// template instantiates against the real KeyFrame / MapPoint / g2o::Sim3 in a checkout; the two optimize() calls and
// the inlier passes are one call into libeaofusion_hip.so.  The header needs no Eigen: g2o::Sim3 is read through rotation().x() .. w(),
// translation()[i] and scale(), and written back through Sim3T(QuatT(w, x, y, z), VecT(t0, t1, t2), s) -- the device's quaternion bit
// for bit, not a re-derivation from a rotation matrix.
//
//   // src/Optimizer_hip_sim3.cc in an EAO-Fusion checkout (replaces the function body in src/Optimizer.cc):
//   #include <eaofusion/OptimizerSim3.h>
//   int ORB_SLAM2::Optimizer::OptimizeSim3(KeyFrame* pKF1, KeyFrame* pKF2, std::vector<MapPoint*>& vpMatches1, g2o::Sim3& g2oS12, const float th2, const bool bFixScale)
//   { return eaofusion::OptimizeSim3<MapPoint>(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale); }
//
// No batching at this level: LoopClosing::ComputeSim3 stops at the first candidate that reaches 20 inliers, and each candidate's
// Sim3Solver::iterate draws from the global rand() stream -- running the candidates together would change the draws later loop
// detections see.  eao_optimize_sim3_batch is there for offline replays.
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "adapter_detail.h"

namespace eaofusion {

// The flattened problem and where each of its correspondences came from.
struct Sim3Walk {
    std::vector<float> T1w, T2w, Xw1, Xw2, obs1, obs2, inv1, inv2;
    std::vector<int> index;        // correspondence k -> i of vpMatches1
    float K1[4] = {0, 0, 0, 0}, K2[4] = {0, 0, 0, 0};
    double q[4] = {0, 0, 0, 1}, t[3] = {0, 0, 0}, s = 1;
    float th2 = 0;
    int fix_scale = 0;
    eao_sim3_problem problem() const {
        eao_sim3_problem p;
        p.n = (int32_t)index.size();
        p.T1w = T1w.data(); p.T2w = T2w.data(); p.Xw1 = Xw1.data(); p.Xw2 = Xw2.data();
        p.obs1 = obs1.data(); p.obs2 = obs2.data(); p.inv_sigma2_1 = inv1.data(); p.inv_sigma2_2 = inv2.data();
        p.fx1 = K1[0]; p.fy1 = K1[1]; p.cx1 = K1[2]; p.cy1 = K1[3];
        p.fx2 = K2[0]; p.fy2 = K2[1]; p.cx2 = K2[2]; p.cy2 = K2[3];
        for (int k = 0; k < 4; k++) p.q[k] = q[k];
        for (int k = 0; k < 3; k++) p.t[k] = t[k];
        p.s = s;
        p.th2 = th2;
        p.fix_scale = fix_scale;
        return p;
    }
};

// The host walk of src/Optimizer.cc:1486-1561: a correspondence gets an edge pair when vpMatches1[i] and GetMapPointMatches()[i] are both
// set, neither isBad(), and pMP2->GetIndexInKeyFrame(pKF2) >= 0; every other entry is skipped and left as it is.
template <class MapPointT, class KeyFrameT, class Sim3T>
Sim3Walk WalkSim3(KeyFrameT* pKF1, KeyFrameT* pKF2, const std::vector<MapPointT*>& vpMatches1, const Sim3T& g2oS12, float th2, bool bFixScale) {
    Sim3Walk w;
    detail::read_intrinsics(pKF1->mK, w.K1);
    detail::read_intrinsics(pKF2->mK, w.K2);
    w.T1w.resize(16); w.T2w.resize(16);
    detail::read_pose(pKF1->GetRotation(), pKF1->GetTranslation(), w.T1w.data());
    detail::read_pose(pKF2->GetRotation(), pKF2->GetTranslation(), w.T2w.data());
    w.q[0] = g2oS12.rotation().x(); w.q[1] = g2oS12.rotation().y(); w.q[2] = g2oS12.rotation().z(); w.q[3] = g2oS12.rotation().w();
    for (int k = 0; k < 3; k++) w.t[k] = g2oS12.translation()[k];
    w.s = g2oS12.scale();
    w.th2 = th2;
    w.fix_scale = bFixScale ? 1 : 0;
    const int N = (int)vpMatches1.size();
    const std::vector<MapPointT*> vpMapPoints1 = pKF1->GetMapPointMatches();
    for (int i = 0; i < N; i++) {
        if (!vpMatches1[i]) continue;
        MapPointT* pMP1 = vpMapPoints1[i];
        MapPointT* pMP2 = vpMatches1[i];
        const int i2 = pMP2->GetIndexInKeyFrame(pKF2);
        if (!pMP1 || !pMP2) continue;
        if (pMP1->isBad() || pMP2->isBad() || i2 < 0) continue;
        detail::push3(pMP1->GetWorldPos(), w.Xw1);
        detail::push3(pMP2->GetWorldPos(), w.Xw2);
        const auto& kp1 = pKF1->mvKeysUn[i];
        const auto& kp2 = pKF2->mvKeysUn[i2];
        w.obs1.push_back(kp1.pt.x); w.obs1.push_back(kp1.pt.y);
        w.obs2.push_back(kp2.pt.x); w.obs2.push_back(kp2.pt.y);
        w.inv1.push_back(pKF1->mvInvLevelSigma2[kp1.octave]);
        w.inv2.push_back(pKF2->mvInvLevelSigma2[kp2.octave]);
        w.index.push_back(i);
    }
    return w;
}

// g2oS12 = g2o::Sim3(Quaterniond(w, x, y, z), Vector3d(t0, t1, t2), s): the quaternion and vector types are those of the accessors
template <class Sim3T> void WriteSim3(Sim3T& S, const double q[4], const double t[3], double s) {
    using QuatT = typename std::decay<decltype(S.rotation())>::type;
    using VecT = typename std::decay<decltype(S.translation())>::type;
    S = Sim3T(QuatT(q[3], q[0], q[1], q[2]), VecT(t[0], t[1], t[2]), s);
}

// Optimizer::OptimizeSim3: nulls vpMatches1 where the reference does (either inlier pass), writes g2oS12 back unless fewer than 10
// correspondences survived the first pass, returns the inlier count.
template <class MapPointT, class KeyFrameT, class Sim3T>
int OptimizeSim3(KeyFrameT* pKF1, KeyFrameT* pKF2, std::vector<MapPointT*>& vpMatches1, Sim3T& g2oS12, float th2, bool bFixScale) {
    const Sim3Walk w = WalkSim3<MapPointT>(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale);
    const eao_sim3_problem p = w.problem();
    std::vector<uint8_t> removed(w.index.size() + 1, 0);
    eao_sim3_result r;
    r.removed = removed.data();
    detail::check(eao_optimize_sim3(&p, &r), "eao_optimize_sim3");
    for (size_t k = 0; k < w.index.size(); k++)
        if (removed[k]) vpMatches1[w.index[k]] = static_cast<MapPointT*>(nullptr);
    if (r.early_exit) return 0;
    WriteSim3(g2oS12, r.q, r.t, r.s);
    return r.n_inliers;
}

}  // namespace eaofusion
