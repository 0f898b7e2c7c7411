// ObjectMap.h -- Object_Map::IsolationForestDeleteOutliers (reference include/Object.h:260, src/Object.cc:1239-1348) on top of the C-ABI
// (eao_object_iforest_outliers_batch): the 50-tree isolation forest over the object's map points runs on the device, bit for bit what
// include/isolation_forest.h computes; the early returns, the erase loop and the mSumPointsPos update stay here, written as upstream writes them.
//
//   // src/Object.cc in an EAO-Fusion checkout: the body becomes a forward
//   #include <eaofusion/ObjectMap.h>
//   void Object_Map::IsolationForestDeleteOutliers() { eaofusion::IsolationForestDeleteOutliers(*this, biForest); }
//
// A caller that restructures the loop of Tracking's object association (the call sites :718, :1596, :1692, :1699 run once per associated object per frame) hands
// all of a frame's objects to the overload over std::vector<ObjT*>: one library call, one launch for all their forests.
//
// Two places where this differs from upstream's text, both where upstream's behaviour is undefined:
//   - after the last outlier is erased upstream's loop reads outliernum[numMOutpoint] one past the end (:1336); here the list is walked with a bound and
//     exactly the flagged points are erased;
//   - a NaN or infinite coordinate breaks std::sort's ordering contract inside Node::Build; the library refuses such an object and it is left unchanged
//     (the return value is -1 and eao_last_error() says why).
//
// ObjT: mnClass, mvpMapObjectMappoints (std::vector<MapPointT*>), mMutexMapPoints, mSumPointsPos (-= the position type).  MapPointT: GetWorldPos() returning a
// value with at<float>(0..2) (cv::Mat 3x1 CV_32F upstream).
#pragma once

#include <cstddef>
#include <cstdint>
#include <mutex>
#include <vector>

#include "adapter_detail.h"

namespace eaofusion {

namespace object_map_detail {

// :1241-1257 without the forest: does upstream's function go on to build one?
template <class ObjT>
bool runs(const ObjT& obj, bool biForest) {
    if (!biForest) return false;
    if ((obj.mnClass == EAO_OBJECT_IFOREST_EXEMPT_CLASS_A) || (obj.mnClass == EAO_OBJECT_IFOREST_EXEMPT_CLASS_B) || (obj.mnClass == EAO_OBJECT_IFOREST_EXEMPT_CLASS_C))
        return false;
    return obj.mvpMapObjectMappoints.size() >= (size_t)EAO_OBJECT_IFOREST_MIN_POINTS;
}

// :1259-1269: GetWorldPos() of the points in vector order
template <class ObjT>
void gather(const ObjT& obj, std::vector<float>& xyz) {
    for (size_t i = 0; i < obj.mvpMapObjectMappoints.size(); i++) detail::push3(obj.mvpMapObjectMappoints[i]->GetWorldPos(), xyz);
}

// :1311-1347 with the flags the library returned for the points gathered above
template <class ObjT>
int erase(ObjT& obj, const uint8_t* flags, size_t n) {
    std::vector<int> outliernum;
    for (size_t i = 0; i < n; i++)
        if (flags[i]) outliernum.push_back((int)i);
    if (outliernum.empty()) return 0;
    int numMappoint = -1;
    size_t numMOutpoint = 0;
    {
        std::unique_lock<std::mutex> lock(obj.mMutexMapPoints);
        for (auto pMP = obj.mvpMapObjectMappoints.begin(); pMP != obj.mvpMapObjectMappoints.end();) {
            numMappoint++;
            const auto pos = (*pMP)->GetWorldPos();
            if (numMOutpoint < outliernum.size() && numMappoint == outliernum[numMOutpoint]) {
                numMOutpoint++;
                pMP = obj.mvpMapObjectMappoints.erase(pMP);
                obj.mSumPointsPos -= pos;
            } else {
                ++pMP;
            }
        }
    }
    return (int)numMOutpoint;
}

}  // namespace object_map_detail

// Object_Map::IsolationForestDeleteOutliers for every object of `objs` in ONE library call.  Returns the number of points erased over all objects, or -1 when the
// library refused the call (every object is left unchanged).
template <class ObjT>
int IsolationForestDeleteOutliers(const std::vector<ObjT*>& objs, bool biForest) {
    std::vector<ObjT*> run;
    std::vector<int32_t> start(1, 0), classId;
    std::vector<float> xyz;
    for (ObjT* obj : objs) {
        if (!object_map_detail::runs(*obj, biForest)) continue;
        object_map_detail::gather(*obj, xyz);
        run.push_back(obj);
        start.push_back((int32_t)(xyz.size() / 3));
        classId.push_back((int32_t)obj->mnClass);
    }
    if (run.empty()) return 0;
    std::vector<uint8_t> flags(xyz.size() / 3);
    std::vector<int32_t> removed(run.size());
    if (eao_object_iforest_outliers_batch((int32_t)run.size(), start.data(), xyz.data(), classId.data(), 1, flags.data(), removed.data(), nullptr) != EAO_OK) return -1;
    int erased = 0;
    for (size_t j = 0; j < run.size(); j++) erased += object_map_detail::erase(*run[j], flags.data() + start[j], (size_t)(start[j + 1] - start[j]));
    return erased;
}

template <class ObjT>
int IsolationForestDeleteOutliers(std::vector<ObjT*>& objs, bool biForest) {      // (a non-const vector must not bind to the single-object form below)
    return IsolationForestDeleteOutliers(static_cast<const std::vector<ObjT*>&>(objs), biForest);
}

// Object_Map::IsolationForestDeleteOutliers.  Returns the number of points erased, or -1 when the library refused the object (it is left unchanged).
template <class ObjT>
int IsolationForestDeleteOutliers(ObjT& obj, bool biForest) {
    return IsolationForestDeleteOutliers(std::vector<ObjT*>(1, &obj), biForest);
}

}  // namespace eaofusion
