// MapPlanes.h -- the plane association of Map (reference include/Map.h:93-97, src/Map.cc:155-292) and the four places a MapPlane's boundary cloud or
// position changes (src/MapPlane.cc:23-39, :137-153, :161-192; src/Map.cc:147-153) on top of the C-ABI (eao_plane_map_*).
//
// The boundary clouds of the map's planes are resident on the device.  Map::AssociatePlanesByBoundary and Map::SearchMatchedPlanes become one library call
// each: the frame's plane coefficients go up, one index per frame plane comes back; what the association is written into (Frame::mvpMapPlanes,
// Frame::mbNewPlane, vpMatched) is written exactly as upstream's loops write it.  Nothing here prints: upstream's `out` flag only selects cout lines.
//
//   // include/Map.h in an EAO-Fusion checkout: one member, and the two bodies in src/Map.cc become forwards
//   #include <eaofusion/MapPlanes.h>
//   eaofusion::MapPlanesT<MapPlane, Frame, KeyFrame> mPlanes;
//   void Map::AssociatePlanesByBoundary(Frame &pF, bool out) { unique_lock<mutex> lock(mMutexMap); mPlanes.AssociatePlanesByBoundary(*this, pF, out); }
//   void Map::SearchMatchedPlanes(KeyFrame *pKF, cv::Mat Scw, const vector<MapPlane *> &vpPlanes, vector<MapPlane *> &vpMatched, bool out)
//   { unique_lock<mutex> lock(mMutexMap); mPlanes.SearchMatchedPlanes(pKF, Scw, vpPlanes, vpMatched, out); }
//
// The hooks (INTEGRATION.md says where each goes):
//   Constructed(pMP, pRefKF, idx)   end of MapPlane::MapPlane           the cloud of pRefKF->mvBoundaryPoints[idx] with pRefKF->GetPose(), and Pos
//   BoundaryUpdated(pMP, F, id)     MapPlane::UpdateBoundary            the cloud of F.mvBoundaryPoints[id] with F.mTcw
//   WorldPosSet(pMP)                end of MapPlane::SetWorldPos        pMP->GetWorldPos()
//   Erased(pMP)                     Map::EraseMapPlane (which the losing side of MapPlane::Replace calls), Map::clear -> Cleared()
// The device does the transform of the cloud (pcl::transformPointCloud with T.inverse()); pMP->mvBoundaryPoints may be kept for the viewer or dropped.
//
// MapPlaneT: mnId, GetWorldPos() -> cv::Mat 4x1 CV_32F.  FrameT: mnPlaneNum, mvPlaneCoefficients (cv::Mat 4x1 CV_32F each), mvBoundaryPoints (clouds with
// .points of .x .y .z), mTcw, mvpMapPlanes, mbNewPlane.  KeyFrameT: mnPlaneNum, mvPlaneCoefficients, mvBoundaryPoints, GetPose().  MapT: mspMapPlanes.
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "adapter_detail.h"

namespace eaofusion {

template <class MapPlaneT, class FrameT, class KeyFrameT>
class MapPlanesT {
public:
    float mfDisTh = EAO_PLANE_MAP_DIS_TH;        // Map::Map, src/Map.cc:22
    float mfAngleTh = EAO_PLANE_MAP_ANGLE_TH;    // :23

    MapPlanesT() { detail::check(eao_plane_map_create(&mHandle), "eao_plane_map_create"); }
    ~MapPlanesT() {
        if (mHandle) eao_plane_map_destroy(mHandle);
    }
    MapPlanesT(const MapPlanesT&) = delete;
    MapPlanesT& operator=(const MapPlanesT&) = delete;
    eao_plane_map* handle() const { return mHandle; }

    // ---------------------------------------------------------------------------------------- the hooks
    void Constructed(MapPlaneT* pMP, KeyFrameT* pRefKF, int idx) {      // src/MapPlane.cc:34-37
        std::vector<float> xyz;
        pack(pRefKF->mvBoundaryPoints[idx], xyz);
        float w[4], T[16];
        detail::read4(pMP->GetWorldPos(), w);
        detail::read44(pRefKF->GetPose(), T);
        detail::check(eao_plane_map_add(mHandle, (uint64_t)pMP->mnId, w, (int32_t)(xyz.size() / 3), xyz.data(), T), "eao_plane_map_add");
    }
    void BoundaryUpdated(MapPlaneT* pMP, const FrameT& pF, int id) {      // src/MapPlane.cc:150-153
        std::vector<float> xyz;
        pack(pF.mvBoundaryPoints[id], xyz);
        float T[16];
        detail::read44(pF.mTcw, T);
        detail::check(eao_plane_map_update_boundary(mHandle, (uint64_t)pMP->mnId, (int32_t)(xyz.size() / 3), xyz.data(), T), "eao_plane_map_update_boundary");
    }
    void WorldPosSet(MapPlaneT* pMP) {      // src/MapPlane.cc:137-142
        float w[4];
        detail::read4(pMP->GetWorldPos(), w);
        detail::check(eao_plane_map_set_world_pos(mHandle, (uint64_t)pMP->mnId, w), "eao_plane_map_set_world_pos");
    }
    void Erased(MapPlaneT* pMP) { detail::check(eao_plane_map_erase(mHandle, (uint64_t)pMP->mnId), "eao_plane_map_erase"); }      // src/Map.cc:147-153
    void Cleared() { detail::check(eao_plane_map_clear(mHandle), "eao_plane_map_clear"); }                                         // src/Map.cc:131-133

            // ---------------------------------------------------------------------------------------- Map::AssociatePlanesByBoundary, src/Map.cc:155-215
            template <class MapT>
            void AssociatePlanesByBoundary(MapT& map, FrameT& pF, bool /*out*/ = false) {
                pF.mbNewPlane = false;      // :160
        std::vector<MapPlaneT*> cand(map.mspMapPlanes.begin(), map.mspMapPlanes.end());      // the std::set's order, :175
        std::vector<int32_t> match;
        float M[16];
        detail::read44(pF.mTcw, M);
        const int32_t start[2] = {0, pF.mnPlaneNum};
        associate(1, M, start, pF.mvPlaneCoefficients, cand, match);
        for (int i = 0; i < pF.mnPlaneNum; ++i)
            if (match[i] >= 0) pF.mvpMapPlanes[i] = cand[match[i]];      // :200 (a plane without a match keeps what the slot held)
        for (auto p : pF.mvpMapPlanes)      // :210-214
            if (p == nullptr) pF.mbNewPlane = true;
    }

    // ---------------------------------------------------------------------------------------- Map::SearchMatchedPlanes, src/Map.cc:245-292
    void SearchMatchedPlanes(KeyFrameT* pKF, cv::Mat Scw, const std::vector<MapPlaneT*>& vpPlanes, std::vector<MapPlaneT*>& vpMatched, bool /*out*/ = false) {
        vpMatched = std::vector<MapPlaneT*>(pKF->mnPlaneNum, static_cast<MapPlaneT*>(nullptr));      // :253
        std::vector<int32_t> match;
        float M[16];
        detail::read44(Scw, M);
        const int32_t start[2] = {0, pKF->mnPlaneNum};
        associate(1, M, start, pKF->mvPlaneCoefficients, vpPlanes, match);
        for (int i = 0; i < pKF->mnPlaneNum; ++i)
            if (match[i] >= 0) vpMatched[i] = vpPlanes[match[i]];      // :286
    }

    // The same for every keyframe of LoopClosing::SearchAndFuse (src/LoopClosing.cc:608-620) against the one list mvpLoopMapPlanes, in ONE call.  Upstream
    // interleaves the searches with MapPlane::Replace (:645); Replace changes neither a candidate's cloud nor its mWorldPos, so searching first gives the same
    // matches.  vvpMatched[k] is what SearchMatchedPlanes(vpKFs[k], vScw[k], vpPlanes, ...) returns.
    void SearchMatchedPlanes(const std::vector<KeyFrameT*>& vpKFs, const std::vector<cv::Mat>& vScw, const std::vector<MapPlaneT*>& vpPlanes,
                             std::vector<std::vector<MapPlaneT*>>& vvpMatched) {
        if (vpKFs.size() != vScw.size()) throw std::runtime_error("MapPlanes::SearchMatchedPlanes: one Scw per keyframe");
        const int n = (int)vpKFs.size();
        std::vector<float> M((size_t)n * 16);
        std::vector<int32_t> start(1, 0);
        std::vector<cv::Mat> coef;
        for (int k = 0; k < n; k++) {
            detail::read44(vScw[k], &M[16 * (size_t)k]);
            for (int i = 0; i < vpKFs[k]->mnPlaneNum; ++i) coef.push_back(vpKFs[k]->mvPlaneCoefficients[i]);
            start.push_back((int32_t)coef.size());
        }
        std::vector<int32_t> match;
        associate(n, M.data(), start.data(), coef, vpPlanes, match);
        vvpMatched.assign((size_t)n, std::vector<MapPlaneT*>());
        for (int k = 0; k < n; k++) {
            vvpMatched[k].assign((size_t)vpKFs[k]->mnPlaneNum, static_cast<MapPlaneT*>(nullptr));
            for (int i = 0; i < vpKFs[k]->mnPlaneNum; ++i)
                if (match[start[k] + i] >= 0) vvpMatched[k][i] = vpPlanes[match[start[k] + i]];
        }
    }

private:
    template <class CloudT>
    static void pack(const CloudT& cloud, std::vector<float>& xyz) {
        xyz.clear();
        xyz.reserve(cloud.points.size() * 3);
        for (const auto& p : cloud.points) {
            xyz.push_back(p.x);
            xyz.push_back(p.y);
            xyz.push_back(p.z);
        }
    }
    // rows = start[nSets] coefficient vectors against the candidates in the order given
    void associate(int32_t nSets, const float* M, const int32_t* start, const std::vector<cv::Mat>& coefficients, const std::vector<MapPlaneT*>& cand,
                   std::vector<int32_t>& match) {
        const int32_t rows = start[nSets];
        std::vector<float> coef((size_t)rows * 4);
        for (int32_t i = 0; i < rows; i++) detail::read4(coefficients[i], &coef[4 * (size_t)i]);
        std::vector<uint64_t> ids;
        ids.reserve(cand.size());
        for (MapPlaneT* p : cand) ids.push_back((uint64_t)p->mnId);
        match.assign((size_t)rows, -1);
        std::vector<float> dis((size_t)rows);
        detail::check(eao_plane_map_associate(mHandle, nSets, M, start, coef.data(), (int32_t)ids.size(), ids.data(), mfDisTh, mfAngleTh, match.data(), dis.data(), nullptr,
                                              nullptr, nullptr),
                      "eao_plane_map_associate");
    }

    eao_plane_map* mHandle = nullptr;
};

}  // namespace eaofusion
