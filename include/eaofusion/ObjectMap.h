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

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <mutex>
#include <unordered_map>
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

// ---- Object_Map::ComputeMeanAndStandard (src/Object.cc:999-1235) with both of its calls of Object_Map::UpdateObjPose (:2243-2303) on top of
// eao_object_cuboids_batch: the sums, deviations, extrema, corners and poses come from the device, bit for bit what upstream's loops compute; the erase of the bad
// points (:1003-1024), the evaluation of Ryaw (:2250-2260, so that the caller's own cos(float) / sin(float) decide its bits) and the member writes stay here.
//
//   // src/Object.cc in an EAO-Fusion checkout: the bodies become forwards
//   void Object_Map::ComputeMeanAndStandard() { eaofusion::ComputeMeanAndStandard<Converter>(*this); }
//   // and, where the loop of :718-719 is restructured: eaofusion::RefineObjects<Converter>(objs, biForest) -- two library calls for all of a frame's objects
//
// ConvT is the conversion policy: ConvT::toSE3Quat(cv::Mat 4x4 CV_32F) builds mCuboid3D.pose and pose_without_yaw from the two matrices the library returns.  In a
// checkout it is upstream's own Converter, so both members are upstream's by construction and this header names no Eigen or g2o type; the vector members are
// assigned through their own type (deduced), constructed from three doubles as upstream constructs them.
//
// Every member is written on the path upstream takes: nothing past mStandar_* when the list is empty (:1050), the bounds only on the few-frames path of :1071 (the
// record says which).  One difference: upstream reads GetWorldPos() of a point three times (:1012, :1034, :1134) and another thread may move it in between; here
// it is read once, under mMutexMapPoints.  A refused call (a non-finite position; the return value is -1) leaves every member as it was; the bad points are
// erased by then, as upstream erases them before it computes anything.
//
// ObjT in addition to the above: mCenter3D, mStandar_x / y / z, mCenterStandar_x / y / z, mCenterStandar, mObjectFrame (pointers to objects with _Pos), mMutex,
// mCuboid3D (rotP, rotR, rotY, cuboidCenter, x_min .. z_max, lenth, width, height, corner_1 .. corner_8, corner_1_w .. corner_8_w, pose, pose_without_yaw,
// mfRMax).  MapPointT in addition: isBad().
namespace object_map_detail {

// :1003-1024: the bad points leave the list under the mutex; the positions of the others in list order
template <class ObjT>
void gather_good(ObjT& obj, std::vector<float>& xyz) {
    std::unique_lock<std::mutex> lock(obj.mMutexMapPoints);
    for (auto pMP = obj.mvpMapObjectMappoints.begin(); pMP != obj.mvpMapObjectMappoints.end();) {
        const auto pos = (*pMP)->GetWorldPos();
        if ((*pMP)->isBad()) {
            pMP = obj.mvpMapObjectMappoints.erase(pMP);
        } else {
            detail::push3(pos, xyz);
            ++pMP;
        }
    }
}

// :2250-2260: upstream's expression, evaluated in float by the caller's own overloads; REigen widens each entry and Converter::toCvMat narrows it back unchanged
template <class CuboidT>
void ryaw(const CuboidT& c, float* R) {
    using std::cos;
    using std::sin;
    float cp = cos(c.rotP);
    float sp = sin(c.rotP);
    float sr = sin(c.rotR);
    float cr = cos(c.rotR);
    float sy = sin(c.rotY);
    float cy = cos(c.rotY);
    R[0] = cp * cy; R[1] = (sr * sp * cy) - (cr * sy); R[2] = (cr * sp * cy) + (sr * sy);
    R[3] = cp * sy; R[4] = (sr * sp * sy) + (cr * cy); R[5] = (cr * sp * sy) - (sr * cy);
    R[6] = -sp; R[7] = sr * cp; R[8] = cr * cp;
}

template <class VecT>
void set3(VecT& dst, const double* v) {
    dst = VecT(v[0], v[1], v[2]);
}

template <class ConvT, class ObjT>
void write_members(ObjT& obj, const eao_object_cuboid_rec& r) {
    obj.mSumPointsPos = detail::mat_of(r.sum_pos, 3, 1);
    obj.mCenter3D = detail::mat_of(r.center, 3, 1);
    obj.mStandar_x = r.standar[0];
    obj.mStandar_y = r.standar[1];
    obj.mStandar_z = r.standar[2];
    if (r.status == EAO_OBJECT_CUBOID_EMPTY) return;      // :1050
    obj.mCenterStandar_x = r.center_standar[0];
    obj.mCenterStandar_y = r.center_standar[1];
    obj.mCenterStandar_z = r.center_standar[2];
    auto& C = obj.mCuboid3D;
    if (r.bounds_written) {      // :1095-1100
        C.x_min = r.bounds[0]; C.x_max = r.bounds[1];
        C.y_min = r.bounds[2]; C.y_max = r.bounds[3];
        C.z_min = r.bounds[4]; C.z_max = r.bounds[5];
    }
    set3(C.corner_1, r.corners[0]); set3(C.corner_2, r.corners[1]); set3(C.corner_3, r.corners[2]); set3(C.corner_4, r.corners[3]);
    set3(C.corner_5, r.corners[4]); set3(C.corner_6, r.corners[5]); set3(C.corner_7, r.corners[6]); set3(C.corner_8, r.corners[7]);
    set3(C.corner_1_w, r.corners_w[0]); set3(C.corner_2_w, r.corners_w[1]); set3(C.corner_3_w, r.corners_w[2]); set3(C.corner_4_w, r.corners_w[3]);
    set3(C.corner_5_w, r.corners_w[4]); set3(C.corner_6_w, r.corners_w[5]); set3(C.corner_7_w, r.corners_w[6]); set3(C.corner_8_w, r.corners_w[7]);
    C.lenth = r.lenth;
    C.width = r.width;
    C.height = r.height;
    set3(C.cuboidCenter, r.cuboid_center);
    {
        std::unique_lock<std::mutex> lock(obj.mMutex);      // UpdateObjPose's (:2245)
        C.pose = ConvT::toSE3Quat(detail::mat_of(r.Twobj, 4, 4));
        C.pose_without_yaw = ConvT::toSE3Quat(detail::mat_of(r.Twobj_without_yaw, 4, 4));
    }
    C.mfRMax = r.rmax;
    obj.mCenterStandar = r.center_standar_dis;
}

}  // namespace object_map_detail

// Object_Map::ComputeMeanAndStandard for every object of `objs` in ONE library call.  Returns 0, or -1 when the library refused the call.
template <class ConvT, class ObjT>
int ComputeMeanAndStandard(const std::vector<ObjT*>& objs) {
    if (objs.empty()) return 0;
    std::vector<std::vector<float>> points(objs.size()), centroids(objs.size());
    std::vector<eao_object_cuboid_desc> descs(objs.size());
    for (size_t j = 0; j < objs.size(); j++) {
        ObjT& obj = *objs[j];
        object_map_detail::gather_good(obj, points[j]);
        for (size_t i = 0; i < obj.mObjectFrame.size(); i++) detail::push3(obj.mObjectFrame[i]->_Pos, centroids[j]);
        eao_object_cuboid_desc& d = descs[j];
        d.n_points = (int32_t)(points[j].size() / 3);
        d.points = points[j].empty() ? nullptr : points[j].data();
        d.n_centroids = (int32_t)(centroids[j].size() / 3);
        d.centroids = centroids[j].empty() ? nullptr : centroids[j].data();
        object_map_detail::ryaw(obj.mCuboid3D, d.Ryaw);
        for (int k = 0; k < 3; k++) d.prev_cuboid_center[k] = obj.mCuboid3D.cuboidCenter[k];
    }
    std::vector<eao_object_cuboid_rec> recs(objs.size());
    if (eao_object_cuboids_batch((int32_t)objs.size(), descs.data(), recs.data()) != EAO_OK) return -1;
    for (size_t j = 0; j < objs.size(); j++) object_map_detail::write_members<ConvT>(*objs[j], recs[j]);
    return 0;
}

template <class ConvT, class ObjT>
int ComputeMeanAndStandard(std::vector<ObjT*>& objs) {      // (a non-const vector must not bind to the single-object form below)
    return ComputeMeanAndStandard<ConvT>(static_cast<const std::vector<ObjT*>&>(objs));
}

// Object_Map::ComputeMeanAndStandard.
template <class ConvT, class ObjT>
int ComputeMeanAndStandard(ObjT& obj) {
    return ComputeMeanAndStandard<ConvT>(std::vector<ObjT*>(1, &obj));
}

// The pair of :718-719 for all of a frame's objects: the forest and its erase, then the cuboids -- two library calls.  Returns the number of points the forest
// erased, or -1 when either call was refused (the cuboids are asked for even behind a refused forest, as upstream's second line runs whatever the first did).
template <class ConvT, class ObjT>
int RefineObjects(const std::vector<ObjT*>& objs, bool biForest) {
    const int erased = IsolationForestDeleteOutliers(objs, biForest);
    const int done = ComputeMeanAndStandard<ConvT>(objs);
    return (erased < 0 || done < 0) ? -1 : erased;
}

// Object_Map::WhetherOverlap (:1954-1970) over every ordered pair of `objs` in one library call: verdict[i * M + j], and where `extents` is given the three overlap
// extents of src/LocalMapping.cc:873-875 at 3 * (i * M + j) (zero where the verdict is 0).  eligible[i] == 0 takes object i out of every pair (the callers' own
// `continue`s: bad_3d, another class, ...).  DealTwoOverlapObjs' decisions and the loops' early `break` stay with the caller; the point erases behind them (BigToSmall,
// DivideEquallyTwoObjs) are BigToSmall and DivideEquallyTwoObjs below.  Returns the number of verdicts set, or -1.
template <class ObjT>
int OverlapMatrix(const std::vector<ObjT*>& objs, const std::vector<uint8_t>& eligible, std::vector<uint8_t>& verdict, std::vector<float>* extents = nullptr) {
    const size_t M = objs.size();
    verdict.assign(M * M, 0);
    if (extents) extents->assign(3 * M * M, 0.0f);
    if (M == 0) return 0;
    if (eligible.size() != M) return -1;
    std::vector<eao_object_overlap_row> rows(M);
    for (size_t j = 0; j < M; j++) {
        rows[j] = eao_object_overlap_row();
        for (int k = 0; k < 3; k++) rows[j].cuboid_center[k] = objs[j]->mCuboid3D.cuboidCenter[k];
        rows[j].lenth = objs[j]->mCuboid3D.lenth;
        rows[j].width = objs[j]->mCuboid3D.width;
        rows[j].height = objs[j]->mCuboid3D.height;
    }
    if (eao_object_overlaps((int32_t)M, rows.data(), eligible.data(), verdict.data(), extents ? extents->data() : nullptr) != EAO_OK) return -1;
    int set = 0;
    for (uint8_t v : verdict) set += v;
    return set;
}

// ---- The update of mvpMapObjectMappoints on top of eao_object_points_update: Object_Map::DataAssociateUpdate (src/Object.cc:1352-1601), step 1 of
// MergeTwoMapObjs (:1766-1821), BigToSmall (:2043-2090) and DivideEquallyTwoObjs (:2094-2121).  The change gate, the gates of the candidates, the comparison of
// every candidate with the growing list, the erase rules and the float sums come from the device, bit for bit what upstream's loops compute (DESIGN.md section
// 4r); the writes into the map points and the object stay here, in upstream's order.
//
//   // src/Object.cc in an EAO-Fusion checkout
//   bool Object_Map::DataAssociateUpdate(Object_2D* ObjectFrame, Frame& mCurrentFrame, cv::Mat& image, int Flag) {
//       if ((Flag != 1) && (Flag != 4)) this->ComputeProjectRectFrame(image, mCurrentFrame);      // :1371, as before
//       return eaofusion::DataAssociateUpdate<Converter>(*this, ObjectFrame, mCurrentFrame, image, Flag, biForest, [&] { /* step 2, :1439-1457; false = :1454 */ }) > 0;
//   }
//
// What stays the caller's: step 2 of DataAssociateUpdate (mnLastAddID, mLastRect, mnConfidence, mObjectFrame; handed in as `step2`, which runs where upstream runs
// it: behind the change gate, before the first write), the cv::circle debug draw, mAssMapObjCenter and mvObjectFrame (:1598-1599), steps 2 to 5 of MergeTwoMapObjs,
// the corner members BigToSmall reads for nothing.  One difference: GetWorldPos() of a point is read once per call, not once per comparison.
//
// ObjT in addition to the above: mnId, mvpMapCurrentNewMappoints, mRectProject, mCuboid3D.pose with rotation().x() .. w() and translation()[k].  MapPointT in
// addition: object_id, object_class, object_id_vector (std::map<int, int>), have_feature, feature.  Obj2DT: _class_id, Obj_c_MapPonits, mBox, mBoxRect.  FrameT:
// mTcw, fx, fy, cx, cy.  ImageT: cols, rows.  Every function returns -1 when the library refused the call; nothing is written then.
namespace object_map_detail {

template <class MapPointT>
int32_t id_count(const MapPointT& mp, int id) {
    const auto sit = mp.object_id_vector.find(id);
    return sit == mp.object_id_vector.end() ? 0 : (int32_t)sit->second;
}

// one call of the entry for one object: the lists as gathered, the outputs sized for them
struct PointsCall {
    eao_object_points_desc d = eao_object_points_desc();
    eao_object_points_rec rec = eao_object_points_rec();
    std::vector<float> map_points, cand_points, survivors_xyz;
    std::vector<int32_t> map_count, cand_count, target, count, list, survivors;
    std::vector<uint8_t> gate, erased;

    template <class ObjT>
    void gather_list(const ObjT& obj) {
        for (size_t i = 0; i < obj.mvpMapObjectMappoints.size(); i++) {
            detail::push3(obj.mvpMapObjectMappoints[i]->GetWorldPos(), map_points);
            map_count.push_back(id_count(*obj.mvpMapObjectMappoints[i], obj.mnId));
        }
        for (int k = 0; k < 3; k++) d.sum_pos[k] = obj.mSumPointsPos.template at<float>(k);
    }
    template <class ObjT, class MapPointT>
    void gather_candidates(const ObjT& obj, const std::vector<MapPointT*>& cand) {
        for (size_t j = 0; j < cand.size(); j++) {
            detail::push3(cand[j]->GetWorldPos(), cand_points);
            cand_count.push_back(id_count(*cand[j], obj.mnId));
        }
    }
    bool run() {
        const size_t M = map_count.size(), C = cand_count.size();
        d.n_map = (int32_t)M;
        d.n_cand = (int32_t)C;
        d.map_points = M ? map_points.data() : nullptr;
        d.map_count = M ? map_count.data() : nullptr;
        d.cand_points = C ? cand_points.data() : nullptr;
        d.cand_count = C ? cand_count.data() : nullptr;
        gate.assign(C + 1, 0); target.assign(C + 1, -1); count.assign(C + 1, 0);
        list.assign(2 * (M + C) + 2, 0); erased.assign(M + C + 1, 0); survivors.assign(2 * (M + C) + 2, 0); survivors_xyz.assign(3 * (M + C) + 3, 0.0f);
        d.survivors = survivors_xyz.data();
        eao_object_points_out o = eao_object_points_out();
        o.rec = &rec; o.gate = gate.data(); o.target = target.data(); o.count = count.data();
        o.list = list.data(); o.erased = erased.data(); o.survivors = survivors.data();
        return eao_object_points_update(&d, &o) == EAO_OK;
    }
};

// :1484-1535 / :1779-1820 with the device's answers: the writes of the candidate loop in candidate order, then the appended points in append order
template <class ObjT, class MapPointT>
void apply_append(ObjT& obj, const std::vector<MapPointT*>& cand, const PointsCall& c, bool current_new) {
    const size_t M = c.map_count.size();
    auto source = [&](int32_t at) -> MapPointT* { return c.list[2 * at] == 0 ? obj.mvpMapObjectMappoints[(size_t)c.list[2 * at + 1]] : cand[(size_t)c.list[2 * at + 1]]; };
    std::vector<MapPointT*> final_list((size_t)c.rec.n_list);
    for (int32_t k = 0; k < c.rec.n_list; k++) final_list[(size_t)k] = source(k);
    std::unique_lock<std::mutex> lock(obj.mMutexMapPoints);
    for (size_t j = 0; j < cand.size(); j++) {
        if (!c.gate[j]) continue;
        MapPointT* pMP = cand[j];
        pMP->object_id = obj.mnId;
        pMP->object_class = obj.mnClass;
        pMP->object_id_vector[pMP->object_id] = c.count[j];      // erase + insert of sit_sec + 1, or insert of 1
        if (c.target[j] >= 0) {
            MapPointT* old = final_list[(size_t)c.target[j]];
            old->have_feature = pMP->have_feature;
            old->feature = pMP->feature;
        }
    }
    for (size_t k = M; k < final_list.size(); k++) {
        obj.mvpMapObjectMappoints.push_back(final_list[k]);
        if (current_new) obj.mvpMapCurrentNewMappoints.push_back(final_list[k]);
    }
}

// the erases of :1543-1588, :2070-2087, :2096-2120 with the device's flags over the list as apply_append left it, and mSumPointsPos
template <class ObjT>
void apply_erase(ObjT& obj, const PointsCall& c) {
    std::unique_lock<std::mutex> lock(obj.mMutexMapPoints);
    size_t at = 0;
    for (auto pMP = obj.mvpMapObjectMappoints.begin(); pMP != obj.mvpMapObjectMappoints.end(); at++) {
        if (at < (size_t)c.rec.n_list && c.erased[at]) pMP = obj.mvpMapObjectMappoints.erase(pMP);
        else ++pMP;
    }
    for (int k = 0; k < 3; k++) obj.mSumPointsPos.template at<float>(k) = c.rec.sum_pos[k];
}

// A list entry that is itself a gated-in candidate shares its object_id_vector with it: step 3 has raised the count that step 4 reads (:1550-1559).  The library
// knows positions, not identities, and was given the count of before; an entry it erased whose raised count exceeds the bound stays.  (mSumPointsPos then holds one
// subtraction too many until ComputeMeanAndStandard, which follows at once, sums it anew.)
template <class ObjT, class MapPointT>
void keep_recounted(const ObjT& obj, const std::vector<MapPointT*>& cand, PointsCall& c) {
    std::unordered_map<const MapPointT*, int32_t> raised;
    for (size_t j = 0; j < cand.size(); j++)
        if (c.gate[j]) raised[cand[j]]++;
    for (size_t k = 0; k < c.map_count.size(); k++) {
        if (!c.erased[k]) continue;
        const auto it = raised.find(obj.mvpMapObjectMappoints[k]);
        if (it != raised.end() && c.map_count[k] + it->second > EAO_OBJECT_POINTS_KEEP_COUNT) {
            c.erased[k] = 0;
            c.rec.n_erased--;
            c.rec.n_survivors++;
        }
    }
}

template <class CuboidT>
void read_cuboid_pose(const CuboidT& C, eao_object_points_desc& d) {
    d.pose_q[0] = C.pose.rotation().x(); d.pose_q[1] = C.pose.rotation().y(); d.pose_q[2] = C.pose.rotation().z(); d.pose_q[3] = C.pose.rotation().w();
    for (int k = 0; k < 3; k++) d.pose_t[k] = C.pose.translation()[k];
    d.lenth = C.lenth; d.width = C.width; d.height = C.height;
}

}  // namespace object_map_detail

// Object_Map::DataAssociateUpdate.  1: associated (upstream's true); 0: upstream's `return false` (another class, the change gate, or step2() said so); -1: refused.
template <class ConvT, class ObjT, class Obj2DT, class FrameT, class ImageT, class Step2T>
int DataAssociateUpdate(ObjT& obj, Obj2DT* ObjectFrame, FrameT& mCurrentFrame, const ImageT& image, int Flag, bool biForest, Step2T step2) {
    if (ObjectFrame->_class_id != obj.mnClass) return 0;      // :1357
    object_map_detail::PointsCall c;
    eao_object_points_desc& d = c.d;
    d.change_gate = ((Flag != 1) && (Flag != 4)) ? 1 : 0;      // :1364
    d.gate = EAO_OBJECT_POINTS_GATE_RADIUS;
    d.erase = EAO_OBJECT_POINTS_ERASE_PROJECTION;
    d.box_off_edge = ((ObjectFrame->mBox.x > EAO_OBJECT_POINTS_EDGE_PIXELS) && (ObjectFrame->mBox.y > EAO_OBJECT_POINTS_EDGE_PIXELS) && (ObjectFrame->mBox.x + ObjectFrame->mBox.width < image.cols - EAO_OBJECT_POINTS_EDGE_PIXELS) &&
                      (ObjectFrame->mBox.y + ObjectFrame->mBox.height < image.rows - EAO_OBJECT_POINTS_EDGE_PIXELS)) ? 1 : 0;      // :1538-1541
    detail::read44(mCurrentFrame.mTcw, d.Tcw);
    d.fx = mCurrentFrame.fx; d.fy = mCurrentFrame.fy; d.cx = mCurrentFrame.cx; d.cy = mCurrentFrame.cy;
    d.cols = image.cols; d.rows = image.rows;
    d.project_rect1[0] = obj.mRectProject.x; d.project_rect1[1] = obj.mRectProject.y; d.project_rect1[2] = obj.mRectProject.width; d.project_rect1[3] = obj.mRectProject.height;
    d.box_rect[0] = ObjectFrame->mBoxRect.x; d.box_rect[1] = ObjectFrame->mBoxRect.y; d.box_rect[2] = ObjectFrame->mBoxRect.width; d.box_rect[3] = ObjectFrame->mBoxRect.height;
    for (int k = 0; k < 3; k++) d.center[k] = obj.mCenter3D.template at<float>(k);
    d.rmax = obj.mCuboid3D.mfRMax;
    d.n_frames_after_push = (int32_t)obj.mObjectFrame.size() + 1;      // step 2 pushes before step 3 reads the size (:1451, :1469)
    c.gather_list(obj);
    c.gather_candidates(obj, ObjectFrame->Obj_c_MapPonits);
    if (!c.run()) return -1;
    if (c.rec.status != EAO_OBJECT_POINTS_DONE) return 0;      // :1435 (an undefined projection associates nothing either)
    if (!step2()) return 0;                                    // :1454
    object_map_detail::keep_recounted(obj, ObjectFrame->Obj_c_MapPonits, c);
    object_map_detail::apply_append(obj, ObjectFrame->Obj_c_MapPonits, c, true);
    object_map_detail::apply_erase(obj, c);
    if (ComputeMeanAndStandard<ConvT>(obj) < 0) return -1;              // :1593 (it sums mSumPointsPos anew, :1001)
    if (IsolationForestDeleteOutliers(obj, biForest) < 0) return -1;    // :1596
    return 1;
}

namespace object_map_detail {

// one call of eao_object_update_chain for one object: the points call's lists, gathered once, and what the stages behind it need
struct ChainCall {
    PointsCall p;
    std::vector<uint8_t> map_bad, cand_bad, forest_flags;
    std::vector<int32_t> cand_alias, final_list;
    std::vector<float> centroids;
    eao_object_chain_desc d = eao_object_chain_desc();
    eao_object_chain_rec rec = eao_object_chain_rec();
    eao_object_cuboid_rec cuboid = eao_object_cuboid_rec();

    // isBad() of every point, and per candidate the list position of the entry that is the very same MapPoint (-1: none)
    template <class ObjT, class MapPointT>
    void gather_flags(const ObjT& obj, const std::vector<MapPointT*>& cand) {
        std::unordered_map<const MapPointT*, int32_t> at;
        for (size_t k = obj.mvpMapObjectMappoints.size(); k-- > 0;) at[obj.mvpMapObjectMappoints[k]] = (int32_t)k;      // (the first of equal pointers)
        for (size_t k = 0; k < obj.mvpMapObjectMappoints.size(); k++) map_bad.push_back(obj.mvpMapObjectMappoints[k]->isBad() ? 1 : 0);
        for (size_t j = 0; j < cand.size(); j++) {
            cand_bad.push_back(cand[j]->isBad() ? 1 : 0);
            const auto it = at.find(cand[j]);
            cand_alias.push_back(it == at.end() ? -1 : it->second);
        }
    }
    bool run() {
        const size_t M = p.map_count.size(), C = p.cand_count.size();
        eao_object_points_desc& q = p.d;
        q.n_map = (int32_t)M;
        q.n_cand = (int32_t)C;
        q.map_points = M ? p.map_points.data() : nullptr;
        q.map_count = M ? p.map_count.data() : nullptr;
        q.cand_points = C ? p.cand_points.data() : nullptr;
        q.cand_count = C ? p.cand_count.data() : nullptr;
        p.gate.assign(C + 1, 0); p.target.assign(C + 1, -1); p.count.assign(C + 1, 0);
        p.list.assign(2 * (M + C) + 2, 0); p.erased.assign(M + C + 1, 0); p.survivors.assign(2 * (M + C) + 2, 0);
        final_list.assign(2 * (M + C) + 2, 0);
        forest_flags.assign(M + C + 1, 0);
        d.points = q;
        d.map_bad = M ? map_bad.data() : nullptr;
        d.cand_bad = C ? cand_bad.data() : nullptr;
        d.cand_alias = C ? cand_alias.data() : nullptr;
        d.n_centroids = (int32_t)(centroids.size() / 3);
        d.centroids = centroids.empty() ? nullptr : centroids.data();
        eao_object_chain_out o = eao_object_chain_out();
        o.points.rec = &p.rec; o.points.gate = p.gate.data(); o.points.target = p.target.data(); o.points.count = p.count.data();
        o.points.list = p.list.data(); o.points.erased = p.erased.data(); o.points.survivors = p.survivors.data();
        o.rec = &rec; o.final = final_list.data(); o.cuboid = &cuboid; o.forest_flags = forest_flags.data();
        return eao_object_update_chain(&d, &o) == EAO_OK;
    }
};

// :1003-1024 with the flags the chain was given: over the list as apply_erase left it (the survivors, in order), the bad points leave under the mutex
template <class ObjT>
void apply_bad(ObjT& obj, const ChainCall& c) {
    std::unique_lock<std::mutex> lock(obj.mMutexMapPoints);
    size_t at = 0;
    for (auto pMP = obj.mvpMapObjectMappoints.begin(); pMP != obj.mvpMapObjectMappoints.end(); at++) {
        bool bad = false;
        if (at < (size_t)c.p.rec.n_survivors) {
            const int32_t src = c.p.survivors[2 * at], idx = c.p.survivors[2 * at + 1];
            bad = (src ? c.cand_bad[(size_t)idx] : c.map_bad[(size_t)idx]) != 0;
        }
        if (bad) pMP = obj.mvpMapObjectMappoints.erase(pMP);
        else ++pMP;
    }
}

}  // namespace object_map_detail

// Object_Map::DataAssociateUpdate over ONE library call (eao_object_update_chain): the positions are gathered once, and the point update, the erase of the bad
// points, the cuboid and the isolation forest run chained on the device.  The same three return values and the same members afterwards as DataAssociateUpdate
// above.  The chain is pure, so a false step2() discards it, as the order above discards the points call.  Two differences: isBad() of a point is read when the
// lists are gathered, not when ComputeMeanAndStandard would reach it; and a list that holds the same MapPoint twice hands the raised count of :1550-1559 to the
// first of the two entries only.
template <class ConvT, class ObjT, class Obj2DT, class FrameT, class ImageT, class Step2T>
int DataAssociateUpdateChained(ObjT& obj, Obj2DT* ObjectFrame, FrameT& mCurrentFrame, const ImageT& image, int Flag, bool biForest, Step2T step2) {
    if (ObjectFrame->_class_id != obj.mnClass) return 0;      // :1357
    object_map_detail::ChainCall c;
    eao_object_points_desc& d = c.p.d;
    d.change_gate = ((Flag != 1) && (Flag != 4)) ? 1 : 0;      // :1364
    d.gate = EAO_OBJECT_POINTS_GATE_RADIUS;
    d.erase = EAO_OBJECT_POINTS_ERASE_PROJECTION;
    d.box_off_edge = ((ObjectFrame->mBox.x > EAO_OBJECT_POINTS_EDGE_PIXELS) && (ObjectFrame->mBox.y > EAO_OBJECT_POINTS_EDGE_PIXELS) && (ObjectFrame->mBox.x + ObjectFrame->mBox.width < image.cols - EAO_OBJECT_POINTS_EDGE_PIXELS) &&
                      (ObjectFrame->mBox.y + ObjectFrame->mBox.height < image.rows - EAO_OBJECT_POINTS_EDGE_PIXELS)) ? 1 : 0;      // :1538-1541
    detail::read44(mCurrentFrame.mTcw, d.Tcw);
    d.fx = mCurrentFrame.fx; d.fy = mCurrentFrame.fy; d.cx = mCurrentFrame.cx; d.cy = mCurrentFrame.cy;
    d.cols = image.cols; d.rows = image.rows;
    d.project_rect1[0] = obj.mRectProject.x; d.project_rect1[1] = obj.mRectProject.y; d.project_rect1[2] = obj.mRectProject.width; d.project_rect1[3] = obj.mRectProject.height;
    d.box_rect[0] = ObjectFrame->mBoxRect.x; d.box_rect[1] = ObjectFrame->mBoxRect.y; d.box_rect[2] = ObjectFrame->mBoxRect.width; d.box_rect[3] = ObjectFrame->mBoxRect.height;
    for (int k = 0; k < 3; k++) d.center[k] = obj.mCenter3D.template at<float>(k);
    d.rmax = obj.mCuboid3D.mfRMax;
    d.n_frames_after_push = (int32_t)obj.mObjectFrame.size() + 1;      // step 2 pushes before step 3 reads the size (:1451, :1469)
    c.p.gather_list(obj);
    c.p.gather_candidates(obj, ObjectFrame->Obj_c_MapPonits);
    c.gather_flags(obj, ObjectFrame->Obj_c_MapPonits);
    for (size_t i = 0; i < obj.mObjectFrame.size(); i++) detail::push3(obj.mObjectFrame[i]->_Pos, c.centroids);
    detail::push3(ObjectFrame->_Pos, c.centroids);      // step 2 pushes the detection before the cuboid reads the centroids (:1451, :1054)
    object_map_detail::ryaw(obj.mCuboid3D, c.d.Ryaw);
    for (int k = 0; k < 3; k++) c.d.prev_cuboid_center[k] = obj.mCuboid3D.cuboidCenter[k];
    c.d.class_id = (int32_t)obj.mnClass;
    c.d.bi_forest = biForest ? 1 : 0;
    if (!c.run()) return -1;
    if (c.p.rec.status != EAO_OBJECT_POINTS_DONE) return 0;      // :1435 (an undefined projection associates nothing either)
    if (!step2()) return 0;                                      // :1454
    object_map_detail::apply_append(obj, ObjectFrame->Obj_c_MapPonits, c.p, true);
    object_map_detail::apply_erase(obj, c.p);
    object_map_detail::apply_bad(obj, c);
    object_map_detail::write_members<ConvT>(obj, c.cuboid);      // :1593 (it sums mSumPointsPos anew, :1001)
    object_map_detail::erase(obj, c.forest_flags.data(), (size_t)c.rec.n_final);      // :1596
    return 1;
}

// Step 1 of Object_Map::MergeTwoMapObjs (:1766-1821): RepeatObj's points into obj.  Returns the number of points appended, or -1.
template <class ObjT>
int MergeTwoMapObjsPoints(ObjT& obj, ObjT& RepeatObj) {
    object_map_detail::PointsCall c;
    c.d.gate = EAO_OBJECT_POINTS_GATE_CUBOID;
    object_map_detail::read_cuboid_pose(obj.mCuboid3D, c.d);
    c.gather_list(obj);
    c.gather_candidates(obj, RepeatObj.mvpMapObjectMappoints);
    if (!c.run()) return -1;
    object_map_detail::apply_append(obj, RepeatObj.mvpMapObjectMappoints, c, false);
    for (int k = 0; k < 3; k++) obj.mSumPointsPos.template at<float>(k) = c.rec.sum_pos[k];
    return c.rec.n_appended;
}

// Object_Map::BigToSmall (:2043-2090): the points of obj strictly inside SmallObj's bounds leave it, then ComputeMeanAndStandard.  Returns the number erased, or -1.
template <class ConvT, class ObjT>
int BigToSmall(ObjT& obj, const ObjT& SmallObj) {
    object_map_detail::PointsCall c;
    c.d.erase = EAO_OBJECT_POINTS_ERASE_BOX;
    const auto& S = SmallObj.mCuboid3D;
    c.d.bounds[0] = S.x_min; c.d.bounds[1] = S.x_max; c.d.bounds[2] = S.y_min; c.d.bounds[3] = S.y_max; c.d.bounds[4] = S.z_min; c.d.bounds[5] = S.z_max;
    c.gather_list(obj);
    if (!c.run()) return -1;
    object_map_detail::apply_erase(obj, c);
    if (ComputeMeanAndStandard<ConvT>(obj) < 0) return -1;      // :2089
    return c.rec.n_erased;
}

// Object_Map::DivideEquallyTwoObjs (:2094-2121).  Returns the number erased, or -1.
template <class ObjT>
int DivideEquallyTwoObjs(ObjT& obj, const ObjT& AnotherObj, float overlap_x, float overlap_y, float overlap_z) {
    object_map_detail::PointsCall c;
    c.d.erase = EAO_OBJECT_POINTS_ERASE_SHRUNK;
    const auto& A = AnotherObj.mCuboid3D;
    for (int k = 0; k < 3; k++) c.d.cuboid_center[k] = A.cuboidCenter[k];
    c.d.lenth = A.lenth; c.d.width = A.width; c.d.height = A.height;
    c.d.overlap[0] = overlap_x; c.d.overlap[1] = overlap_y; c.d.overlap[2] = overlap_z;
    c.gather_list(obj);
    if (!c.run()) return -1;
    object_map_detail::apply_erase(obj, c);
    return c.rec.n_erased;
}

}  // namespace eaofusion
