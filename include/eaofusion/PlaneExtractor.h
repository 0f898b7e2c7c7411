// PlaneExtractor.h -- Frame::ComputePlanesFromPEAC (reference src/Frame.cc:381-460, called from the RGB-D constructor at :240) on top of the C-ABI
// (eao_plane_seg_*): the depth image goes up, PEAC's segmentation, the per-plane voxel grids and PlaneNotSeen run in the library, and
// the frame's members are filled as upstream fills them.
//
//   // src/Frame.cc in an EAO-Fusion checkout: the body of the member becomes a forward
//   #include <eaofusion/PlaneExtractor.h>
//   void Frame::ComputePlanesFromPEAC(const cv::Mat &imDepth) { eaofusion::ComputePlanesFromPEAC(*this, imDepth); }
//
// What is written (src/Frame.cc:410, :453-455): plane_num_ = the number of planes PEAC extracted (kept or not, as upstream's plane_vertices_.size()); for every
// plane that PlaneNotSeen keeps, in order, its coefficients (cv::Mat 4x1 CV_32F, d >= 0) are appended to mvPlaneCoefficients and its voxel cloud to
// mvBoundaryPoints and to mvPlanePoints.  The vectors are appended to, not cleared, as upstream's push_backs.
//
// The clouds also stay on the device in the extractor's handle until its next frame.  A MapPlane built from plane idx of that frame can take its boundary from
// there instead of from the host copy: the hooks below stand where MapPlanesT::Constructed / BoundaryUpdated stand (include/eaofusion/MapPlanes.h,
// src/MapPlane.cc:34-37, :150-153) and append the cloud device to device (eao_plane_map_add_from_seg / eao_plane_map_update_boundary_from_seg).  They throw when
// the extractor has moved on to another frame.
//
// FrameT: fx, fy, cx, cy (floats, static or not), mnId, plane_num_, mvPlaneCoefficients (std::vector<cv::Mat>), mvBoundaryPoints and mvPlanePoints (vectors of
// clouds with .points of .x .y .z).  imDepth: CV_32F, the frame's size.
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "adapter_detail.h"

namespace eaofusion {

class PlaneExtractor {
public:
    PlaneExtractor() {}
    ~PlaneExtractor() {
        if (mHandle) eao_plane_seg_destroy(mHandle);
    }
    PlaneExtractor(const PlaneExtractor&) = delete;
    PlaneExtractor& operator=(const PlaneExtractor&) = delete;
    eao_plane_seg* handle() const { return mHandle; }

    template <class FrameT>
    void ComputePlanesFromPEAC(FrameT& F, const cv::Mat& imDepth) {
        if (imDepth.empty() || imDepth.type() != CV_32F) throw std::runtime_error("PlaneExtractor: imDepth must be a CV_32F image");
        ready(imDepth.cols, imDepth.rows, F.fx, F.fy, F.cx, F.cy);
        mHaveFrame = false;
        detail::check(eao_plane_seg_run(mHandle, imDepth.ptr<float>(0), (int32_t)(imDepth.step / sizeof(float))), "eao_plane_seg_run");
        int32_t n = 0;
        detail::check(eao_plane_seg_planes(mHandle, 0, nullptr, &n), "eao_plane_seg_planes");
        std::vector<eao_plane_seg_plane> planes((size_t)n);
        if (n > 0) detail::check(eao_plane_seg_planes(mHandle, n, planes.data(), &n), "eao_plane_seg_planes");
        F.plane_num_ = (int)n;      // :410
        mKept.clear();
        std::vector<float> xyz;
        for (int32_t i = 0; i < n; i++) {
            if (!planes[i].kept) continue;      // :447-450
            xyz.resize((size_t)planes[i].cloud_count * 3);
            int32_t m = 0;
            detail::check(eao_plane_seg_cloud(mHandle, i, planes[i].cloud_count, xyz.data(), &m), "eao_plane_seg_cloud");
            typename std::remove_reference<decltype(F.mvBoundaryPoints)>::type::value_type cloud;
            for (int32_t k = 0; k < m; k++) {
                typename std::remove_reference<decltype(cloud.points)>::type::value_type p = {};
                p.x = xyz[3 * (size_t)k]; p.y = xyz[3 * (size_t)k + 1]; p.z = xyz[3 * (size_t)k + 2];
                cloud.points.push_back(p);
            }
            const cv::Mat coef = detail::mat_of(planes[i].coef, 4, 1);
            F.mvBoundaryPoints.push_back(cloud);      // :453-455
            F.mvPlanePoints.push_back(cloud);
            F.mvPlaneCoefficients.push_back(coef);
            mKept.push_back(i);
        }
        mFrameId = (uint64_t)F.mnId;
        mHaveFrame = true;
    }

    // ---------------------------------------------------------------------------------------- the MapPlanesT hooks, device to device
    // MapPlane::MapPlane (src/MapPlane.cc:34-37) for plane idx of the frame this extractor ran last: in place of planes.Constructed(pMP, pRefKF, idx)
    template <class MapPlanesT_, class MapPlaneT>
    void Constructed(MapPlanesT_& planes, MapPlaneT* pMP, uint64_t frameId, int idx, const cv::Mat& Tcw) {
        float w[4], T[16];
        detail::read4(pMP->GetWorldPos(), w);
        detail::read44(Tcw, T);
        detail::check(eao_plane_map_add_from_seg(planes.handle(), (uint64_t)pMP->mnId, w, mHandle, segPlane(frameId, idx), T), "eao_plane_map_add_from_seg");
    }
    // MapPlane::UpdateBoundary (src/MapPlane.cc:150-153): in place of planes.BoundaryUpdated(pMP, F, id)
    template <class MapPlanesT_, class MapPlaneT>
    void BoundaryUpdated(MapPlanesT_& planes, MapPlaneT* pMP, uint64_t frameId, int idx, const cv::Mat& Tcw) {
        float T[16];
        detail::read44(Tcw, T);
        detail::check(eao_plane_map_update_boundary_from_seg(planes.handle(), (uint64_t)pMP->mnId, mHandle, segPlane(frameId, idx), T), "eao_plane_map_update_boundary_from_seg");
    }
    // true while the handle still holds the clouds of frame frameId
    bool Holds(uint64_t frameId) const { return mHaveFrame && mFrameId == frameId; }

private:
    // frame plane idx (an index into the frame's mvBoundaryPoints as this extractor filled it) -> the plane of the handle's table
    int32_t segPlane(uint64_t frameId, int idx) const {
        if (!Holds(frameId)) throw std::runtime_error("PlaneExtractor: the handle no longer holds that frame's clouds");
        if (idx < 0 || idx >= (int)mKept.size()) throw std::runtime_error("PlaneExtractor: no such frame plane");
        return mKept[(size_t)idx];
    }
    // one handle per geometry; a frame of another size or camera replaces it
    void ready(int width, int height, float fx, float fy, float cx, float cy) {
        if (mHandle && mCfg.width == width && mCfg.height == height && mCfg.fx == fx && mCfg.fy == fy && mCfg.cx == cx && mCfg.cy == cy) return;
        eao_plane_seg_cfg cfg;
        eao_plane_seg_cfg_default(&cfg, width, height, fx, fy, cx, cy);      // PlaneFitter() and ParamSet() as written: plane_filter is never configured upstream
        eao_plane_seg* h = nullptr;
        detail::check(eao_plane_seg_create(&cfg, &h), "eao_plane_seg_create");
        if (mHandle) eao_plane_seg_destroy(mHandle);
        mHandle = h;
        mCfg = cfg;
        mHaveFrame = false;
    }

    eao_plane_seg* mHandle = nullptr;
    eao_plane_seg_cfg mCfg = eao_plane_seg_cfg();
    std::vector<int32_t> mKept;
    uint64_t mFrameId = 0;
    bool mHaveFrame = false;
};

// The extractor of the calling thread (upstream's plane_filter is a Frame member that is copied with the frame and used by the Tracking thread alone).
inline PlaneExtractor& ThreadPlaneExtractor() {
    thread_local PlaneExtractor ex;
    return ex;
}

// Frame::ComputePlanesFromPEAC(imDepth), src/Frame.cc:381-460
template <class FrameT>
void ComputePlanesFromPEAC(FrameT& F, const cv::Mat& imDepth) {
    ThreadPlaneExtractor().ComputePlanesFromPEAC(F, imDepth);
}

}  // namespace eaofusion
