// LocalMapping.h -- the triangulation half of LocalMapping::CreateNewMapPoints (reference src/LocalMapping.cc:288-454) over the library's C-ABI.
//
// Upstream runs, per neighbour keyframe, SearchForTriangulation and then a loop over the matched pairs that triangulates and gates each one.  The searches are
// ORBmatcher::SearchForTriangulationBatch (include/eaofusion/ORBmatcher.h); this header adds the loop:
//   TriangulateMatches(pKF1, vpNeighKFs, vvMatchedPairs)                          host arrays, over the pairs a batch search returned
//   CreateNewMapPointsBatch(h1, pKF1, h2s, vpNeighKFs, vF12, bOnlyStereo)         keyframe handles: search and triangulation in one library call
// Both return, per neighbour and in pair order, {idx1, idx2, x3D} of the ACCEPTED pairs.  Creating the MapPoint, its observations, descriptor and normal
// (:437-453) stays on the caller's side of the ABI, as with Fuse.
//
// The hoisted arrangement and what it changes: upstream interleaves search and triangulation, so a keypoint of the current keyframe that received a point from
// neighbour k is occupied when neighbour k + 1 is searched and is not offered again.  Here every search sees the occupancy at entry.  Both functions therefore
// drop an accepted pair when an earlier neighbour of the same call already produced a point for the same idx1 -- exactly the pairs upstream's loop would not have
// offered (`dropped` counts them).  What remains different is documented in INTEGRATION.md (a neighbour's own keypoint is never offered twice: each neighbour is
// searched once).
#ifndef EAOFUSION_LOCALMAPPING_H
#define EAOFUSION_LOCALMAPPING_H
#include <utility>
#include <vector>

#include "ORBmatcher.h"
#include "adapter_detail.h"

namespace eaofusion {

struct NewMapPoint {
    size_t idx1, idx2;      // keypoint of the current keyframe, keypoint of the neighbour
    cv::Mat x3D;            // 3 x 1 CV_32F, world coordinates
    int verdict;            // EAO_TRI_TRIANGULATED / EAO_TRI_UNPROJECTED_1 / EAO_TRI_UNPROJECTED_2: which branch made the point
};

class NewMapPoints : public ORBmatcher {
public:
    static constexpr float RATIO_FACTOR_BASE = 1.5f;      // src/LocalMapping.cc:236  ratioFactor = 1.5f*mpCurrentKeyFrame->mfScaleFactor
    // `ORBmatcher matcher(0.6,false)` of :219
    NewMapPoints(float nnratio = 0.6f, bool checkOri = false) : ORBmatcher(nnratio, checkOri) {}

    size_t dropped = 0;      // accepted pairs of the last call whose idx1 an earlier neighbour of that call had already given a point

    // the loop of :288-454 over vvMatchedPairs[k] (what SearchForTriangulationBatch returned for vpNeighKFs[k])
    template <class KeyFrameT>
    std::vector<std::vector<NewMapPoint> > TriangulateMatches(KeyFrameT* pKF1, const std::vector<KeyFrameT*>& vpNeighKFs,
                                                              const std::vector<std::vector<std::pair<size_t, size_t> > >& vvMatchedPairs) {
        const size_t nb = vpNeighKFs.size();
        dropped = 0;
        if (!nb) return std::vector<std::vector<NewMapPoint> >();
        FrameArrays fa1;
        DepthArrays da1;
        eao_frame_view v1 = kfview(*pKF1, fa1);
        depth_of(*pKF1, da1);
        const eao_tri_camera c1 = camera_of(*pKF1);
        std::vector<FrameArrays> fa2(nb);
        std::vector<DepthArrays> da2(nb);
        std::vector<eao_frame_view> v2(nb);
        std::vector<const eao_frame_view*> pv(nb);
        std::vector<eao_tri_camera> c2(nb);
        std::vector<const float*> dp(nb), rx(nb), ry(nb);
        std::vector<int32_t> m12(nb * (size_t)v1.n, -1);
        for (size_t q = 0; q < nb; q++) {
            v2[q] = kfview(*vpNeighKFs[q], fa2[q]);
            depth_of(*vpNeighKFs[q], da2[q]);
            pv[q] = &v2[q]; c2[q] = camera_of(*vpNeighKFs[q]);
            dp[q] = da2[q].depth.data(); rx[q] = da2[q].rx.data(); ry[q] = da2[q].ry.data();
            for (size_t j = 0; j < vvMatchedPairs[q].size(); j++) m12[q * v1.n + vvMatchedPairs[q][j].first] = (int32_t)vvMatchedPairs[q][j].second;
        }
        std::vector<int32_t> verdict(nb * (size_t)v1.n, 0);
        std::vector<float> x3d(3 * nb * (size_t)v1.n, 0.f);
        detail::check(eao_triangulate_matches_batch(&v1, &c1, da1.depth.data(), da1.rx.data(), da1.ry.data(), (int)nb, pv.data(), c2.data(), dp.data(), rx.data(), ry.data(),
                                                    m12.data(), RATIO_FACTOR_BASE * pKF1->mfScaleFactor, verdict.data(), x3d.data()), "eao_triangulate_matches_batch");
        return accepted(nb, v1.n, m12, verdict, x3d);
    }

    // search and triangulation over KEYFRAME HANDLES in one library call (eao_kf_create_new_map_points): vF12[k] = ComputeF12(pKF1, vpNeighKFs[k]) (:268);
    // the handles carry their depth (KeyFrameHandles::of sends it with the upload).  vvMatchedPairs, when given, receives what SearchForTriangulationBatch would.
    template <class KeyFrameT>
    std::vector<std::vector<NewMapPoint> > CreateNewMapPointsBatch(const eao_keyframe* h1, KeyFrameT* pKF1, const std::vector<const eao_keyframe*>& h2s,
                                                                   const std::vector<KeyFrameT*>& vpNeighKFs, const std::vector<cv::Mat>& vF12, const bool bOnlyStereo,
                                                                   std::vector<std::vector<std::pair<size_t, size_t> > >* vvMatchedPairs = nullptr) {
        const size_t nb = vpNeighKFs.size();
        dropped = 0;
        if (vvMatchedPairs) vvMatchedPairs->assign(nb, std::vector<std::pair<size_t, size_t> >());
        if (!nb) return std::vector<std::vector<NewMapPoint> >();
        std::vector<float> Fm(9 * nb), ex(nb), ey(nb);
        std::vector<eao_tri_camera> c2(nb);
        const eao_tri_camera c1 = camera_of(*pKF1);
        const cv::Mat Cw = pKF1->GetCameraCenter();
        for (size_t q = 0; q < nb; q++) {
            KeyFrameT* pKF2 = vpNeighKFs[q];
            detail::epipole(Cw, pKF2->GetRotation(), pKF2->GetTranslation(), pKF2->fx, pKF2->fy, pKF2->cx, pKF2->cy, ex[q], ey[q]);      // as in the single call (src/ORBmatcher.cc:663-670)
            detail::read33(vF12[q], &Fm[9 * q]);
            c2[q] = camera_of(*pKF2);
        }
        const int n1 = eao_keyframe_size(h1);
        std::vector<int32_t> m12(nb * (size_t)n1, -1), nm(nb, 0), verdict(nb * (size_t)n1, 0);
        std::vector<float> x3d(3 * nb * (size_t)n1, 0.f);
        detail::check(eao_kf_create_new_map_points(h1, &c1, (int)nb, h2s.data(), c2.data(), Fm.data(), ex.data(), ey.data(), bOnlyStereo ? 1 : 0, mbCheckOrientation ? 1 : 0,
                                                   RATIO_FACTOR_BASE * pKF1->mfScaleFactor, m12.data(), nm.data(), verdict.data(), x3d.data()), "eao_kf_create_new_map_points");
        if (vvMatchedPairs)
            for (size_t q = 0; q < nb; q++) {
                (*vvMatchedPairs)[q].reserve(nm[q]);
                for (int i = 0; i < n1; i++) if (m12[q * n1 + i] >= 0) (*vvMatchedPairs)[q].push_back(std::make_pair((size_t)i, (size_t)m12[q * n1 + i]));
            }
        return accepted(nb, n1, m12, verdict, x3d);
    }

    // GetRotation / GetTranslation / GetCameraCenter and the intrinsics as :221-234, :274-286 read them
    template <class KeyFrameT>
    static eao_tri_camera camera_of(KeyFrameT& K) {
        eao_tri_camera c;
        const cv::Mat R = K.GetRotation(), t = K.GetTranslation(), O = K.GetCameraCenter();
        detail::read33(R, c.Rcw); detail::read3(t, c.tcw); detail::read3(O, c.Ow);
        c.fx = K.fx; c.fy = K.fy; c.cx = K.cx; c.cy = K.cy; c.invfx = K.invfx; c.invfy = K.invfy; c.mb = K.mb; c.mbf = K.mbf;
        return c;
    }

private:
    struct DepthArrays { std::vector<float> depth, rx, ry; };
    template <class KeyFrameT>
    static void depth_of(KeyFrameT& K, DepthArrays& a) {      // mvDepth and mvKeys[i].pt (what KeyFrame::UnprojectStereo reads, src/KeyFrame.cc:654-670)
        const int N = K.N;
        a.depth.assign(K.mvDepth.begin(), K.mvDepth.end());
        a.rx.resize(N); a.ry.resize(N);
        for (int i = 0; i < N; i++) { a.rx[i] = K.mvKeys[i].pt.x; a.ry[i] = K.mvKeys[i].pt.y; }
    }
    // the accepted pairs per neighbour in pair (= idx1) order, less those whose idx1 an earlier neighbour already served
    std::vector<std::vector<NewMapPoint> > accepted(size_t nb, int n1, const std::vector<int32_t>& m12, const std::vector<int32_t>& verdict, const std::vector<float>& x3d) {
        std::vector<std::vector<NewMapPoint> > out(nb);
        std::vector<uint8_t> served(n1 > 0 ? n1 : 1, 0);
        for (size_t q = 0; q < nb; q++)
            for (int i = 0; i < n1; i++) {
                const int32_t v = verdict[q * n1 + i];
                if (v != EAO_TRI_TRIANGULATED && v != EAO_TRI_UNPROJECTED_1 && v != EAO_TRI_UNPROJECTED_2) continue;
                if (served[i]) { dropped++; continue; }
                served[i] = 1;
                NewMapPoint p;
                p.idx1 = (size_t)i; p.idx2 = (size_t)m12[q * n1 + i]; p.verdict = v;
                p.x3D = detail::mat_of(&x3d[3 * (q * n1 + i)], 3, 1);
                out[q].push_back(p);
            }
        return out;
    }
};

}  // namespace eaofusion
#endif  // EAOFUSION_LOCALMAPPING_H
