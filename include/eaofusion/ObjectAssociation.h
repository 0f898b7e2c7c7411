// ObjectAssociation.h -- the data-parallel parts of Tracking's object association (reference src/Tracking.cc:2036-2069) on top of the C-ABI:
// Object_2D::NoParaDataAssociation (include/Object.h:97, src/Object.cc:728-962) through eao_object_np_association_batch and Object_Map::ComputeProjectRectFrame
// (include/Object.h:246, src/Object.cc:1606-1651) through eao_object_project_rects_batch.  Both run on the device and return exactly what upstream computes; the
// gathering of the points and the loops around the calls stay here, written as upstream writes them.
//
//   // src/Object.cc in an EAO-Fusion checkout: the bodies become forwards
//   #include <eaofusion/ObjectAssociation.h>
//   int Object_2D::NoParaDataAssociation(Object_Map* ObjectMapSingle, Frame&, cv::Mat&) { return eaofusion::NoParaDataAssociation(*this, *ObjectMapSingle); }
//   void Object_Map::ComputeProjectRectFrame(cv::Mat& image, Frame& f) { eaofusion::ComputeProjectRectFrame(*this, f, image.cols, image.rows); }
//
// A caller that restructures the loops hands a whole loop to one library call: NoParaCandidates is the loop of src/Object.cc:260-277 (one detection against every
// map object of its class), ComputeProjectRectFrames the loop of src/Tracking.cc:2041-2055 (every object under the frame's pose).  There is no form that takes
// several detections of a frame at once: upstream's DataAssociateUpdate adds points to map objects between two detections (:287-:330), so only one detection
// against all objects is a snapshot upstream also sees.
//
// Two places where this differs from upstream's text, both where upstream's behaviour is undefined:
//   - where the int product m * n * (m + n + 1) of :942 overflows, the library answers EAO_OBJECT_NP_UNDEFINED; here that is 2 (association failed);
//   - where a projection is a NaN (std::sort's contract at :1634) or the box lies outside int (cv::Rect's float -> int conversion), mRectProject is left
//     unchanged.
//
// Obj2dT: _class_id, Obj_c_MapPonits (std::vector<MapPointT*>).  ObjMapT: mnClass, bBadErase, mvpMapObjectMappoints, mnLastAddID, mRectProject (constructible
// from four ints, cv::Rect upstream).  MapPointT: isBad(), out_point, GetWorldPos() returning a value with at<float>(0..2).  FrameT: mTcw with at<float>(r, c),
// fx, fy, cx, cy, mnId.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "adapter_detail.h"

namespace eaofusion {

namespace object_association_detail {

// the points upstream counts and compares: not isBad() and not out_point (:737, :751, :787, :815, :846), in vector order
template <class VecT>
void gather_good(const VecT& points, std::vector<float>& xyz) {
    for (size_t i = 0; i < points.size(); i++) {
        if (points[i]->isBad() || points[i]->out_point) continue;
        detail::push3(points[i]->GetWorldPos(), xyz);
    }
}

// One detection against the map objects `cand`, in that order: one library call.  verdict[k] as upstream returns it; false when the library refused the call.
template <class Obj2dT, class ObjMapT>
bool associate(const Obj2dT& obj2d, const std::vector<const ObjMapT*>& cand, std::vector<int32_t>& verdict) {
    std::vector<float> det, map;
    gather_good(obj2d.Obj_c_MapPonits, det);
    const int32_t detStart[2] = {0, (int32_t)(det.size() / 3)};
    std::vector<int32_t> mapStart(1, 0), mapTotal, pairDet(cand.size(), 0), pairMap;
    for (size_t k = 0; k < cand.size(); k++) {
        gather_good(cand[k]->mvpMapObjectMappoints, map);
        mapStart.push_back((int32_t)(map.size() / 3));
        mapTotal.push_back((int32_t)cand[k]->mvpMapObjectMappoints.size());
        pairMap.push_back((int32_t)k);
    }
    verdict.assign(cand.size(), 0);
    if (eao_object_np_association_batch(1, detStart, det.data(), (int32_t)cand.size(), mapStart.data(), map.data(), mapTotal.data(), (int32_t)cand.size(),
                                        pairDet.data(), pairMap.data(), verdict.data(), nullptr, nullptr) != EAO_OK)
        return false;
    for (int32_t& v : verdict)
        if (v == EAO_OBJECT_NP_UNDEFINED) v = 2;
    return true;
}

// m of :732-743
template <class Obj2dT>
int good_points(const Obj2dT& obj2d) {
    int m = 0;
    for (size_t i = 0; i < obj2d.Obj_c_MapPonits.size(); i++)
        if (!(obj2d.Obj_c_MapPonits[i]->isBad() || obj2d.Obj_c_MapPonits[i]->out_point)) m++;
    return m;
}

// Object_Map::ComputeProjectRectFrame for the objects of `objs` under the frame's pose in ONE library call.  Returns the number of objects whose mRectProject was
// written, or -1 when the library refused the call (every object is left unchanged).
template <class ObjMapT, class FrameT>
int project(const std::vector<ObjMapT*>& objs, const FrameT& frame, int cols, int rows) {
    if (objs.empty()) return 0;
    std::vector<float> xyz;
    std::vector<int32_t> start(1, 0);
    for (ObjMapT* obj : objs) {
        for (size_t j = 0; j < obj->mvpMapObjectMappoints.size(); j++)      // (:1612: every point, bad ones included)
            detail::push3(obj->mvpMapObjectMappoints[j]->GetWorldPos(), xyz);
        start.push_back((int32_t)(xyz.size() / 3));
    }
    float Tcw[16];
    detail::read44(frame.mTcw, Tcw);
    std::vector<int32_t> rect(4 * objs.size(), 0);
    std::vector<uint8_t> status(objs.size(), 0);
    if (eao_object_project_rects_batch((int32_t)objs.size(), start.data(), xyz.data(), Tcw, frame.fx, frame.fy, frame.cx, frame.cy, (int32_t)cols, (int32_t)rows,
                                       rect.data(), status.data(), nullptr) != EAO_OK)
        return -1;
    int written = 0;
    for (size_t k = 0; k < objs.size(); k++)
        if (status[k] == 1) {      // 0: no points, upstream returns at :1631; 2: undefined upstream
            objs[k]->mRectProject = decltype(objs[k]->mRectProject)(rect[4 * k], rect[4 * k + 1], rect[4 * k + 2], rect[4 * k + 3]);
            written++;
        }
    return written;
}

}  // namespace object_association_detail

// Object_2D::NoParaDataAssociation: 0, 1 or 2 as upstream, or -1 when the library refused the call (eao_last_error() says why).  m < 20 returns 0 without a call.
template <class Obj2dT, class ObjMapT>
int NoParaDataAssociation(const Obj2dT& obj2d, const ObjMapT& mapObj) {
    if (object_association_detail::good_points(obj2d) < EAO_OBJECT_NP_MIN_DET_POINTS) return 0;      // :760
    std::vector<int32_t> verdict;
    if (!object_association_detail::associate(obj2d, std::vector<const ObjMapT*>(1, &mapObj), verdict)) return -1;
    return (int)verdict[0];
}

// The loop of src/Object.cc:260-277 (run it where upstream's condition `old == false` holds) in ONE library call: vObjByNPId receives the indices upstream pushes,
// in its descending order.  Returns the number pushed, or -1 when the library refused the call (vObjByNPId is left as it was).
template <class Obj2dT, class ObjMapT>
int NoParaCandidates(const Obj2dT& obj2d, const std::vector<ObjMapT*>& mvObjectMap, std::vector<int>& vObjByNPId) {
    // nFlag == 0 (:271) does not depend on i: m < 20 ends the loop at the first object that passes the two filters, before anything is pushed
    if (object_association_detail::good_points(obj2d) < EAO_OBJECT_NP_MIN_DET_POINTS) return 0;
    std::vector<const ObjMapT*> cand;
    std::vector<int> index;
    for (int i = (int)mvObjectMap.size() - 1; i >= 0; i--) {
        if (obj2d._class_id != mvObjectMap[i]->mnClass) continue;
        if (mvObjectMap[i]->bBadErase) continue;
        cand.push_back(mvObjectMap[i]);
        index.push_back(i);
    }
    if (cand.empty()) return 0;
    std::vector<int32_t> verdict;
    if (!object_association_detail::associate(obj2d, cand, verdict)) return -1;
    int pushed = 0;
    for (size_t k = 0; k < cand.size(); k++)
        if (verdict[k] == 1) {      // :275
            vObjByNPId.push_back(index[k]);
            pushed++;
        }
    return pushed;
}

// Object_Map::ComputeProjectRectFrame.  Returns 1 when mRectProject was written, 0 when it was left (no points, or undefined upstream), -1 on a refused call.
template <class ObjMapT, class FrameT>
int ComputeProjectRectFrame(ObjMapT& obj, const FrameT& frame, int cols, int rows) {
    return object_association_detail::project(std::vector<ObjMapT*>(1, &obj), frame, cols, rows);
}

// Step 10.1 of Tracking (src/Tracking.cc:2041-2055) in ONE library call: an object seen in the last 30 frames gets its projected box, any other Rect(0, 0, 0, 0);
// objects marked bBadErase are left alone.  Returns the number of objects whose projected box was written, or -1 when the library refused the call (the objects seen
// in the last 30 frames are then left unchanged).
template <class ObjMapT, class FrameT>
int ComputeProjectRectFrames(const std::vector<ObjMapT*>& mvObjectMap, const FrameT& frame, int cols, int rows) {
    std::vector<ObjMapT*> recent;
    for (int i = 0; i < (int)mvObjectMap.size(); i++) {
        if (mvObjectMap[i]->bBadErase) continue;
        if (mvObjectMap[i]->mnLastAddID > frame.mnId - 30)      // upstream's expression with upstream's types (:2047): int against long unsigned
            recent.push_back(mvObjectMap[i]);
        else
            mvObjectMap[i]->mRectProject = decltype(mvObjectMap[i]->mRectProject)(0, 0, 0, 0);
    }
    return object_association_detail::project(recent, frame, cols, rows);
}

}  // namespace eaofusion
