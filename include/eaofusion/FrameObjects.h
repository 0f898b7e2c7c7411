// FrameObjects.h -- steps 2, 4, 5 and 6 of Tracking's object layer (reference src/Tracking.cc:1768-1973) in one call on top of the C-ABI
// (eao_frame_objects_batch): Tracking::AssociateObjAndPoints (:3031-3065), Object_2D::ComputeMeanAndStandardFrame and RemoveOutliersByBoxPlot
// (src/Object.cc:61-157) per box, the projected centre and the box of the feature points (:1801-1854), the removal of bad boxes (:1868-1973).  The device
// returns exactly what upstream's loops compute; this header gathers the frame and writes the results where upstream writes them.
//
//   // src/Tracking.cc in an EAO-Fusion checkout: :1768-1973 become
//   #include <eaofusion/FrameObjects.h>
//   eaofusion::BuildFrameObjects(objs_2d, mCurrentFrame, image.cols, image.rows);
//
// What it writes, in upstream's order: per keypoint with a good map point and per box that contains it, pMP->object_view = true,
// pMP->frame_id.insert(mCurrentFrame.mnId) and pMP->feature = mvKeysUn[i] (:3051-3053); per object Obj_c_MapPonits (the list after the boxplot), sum_pos_3d,
// _Pos, mStandar_x / y / z, mCountMappoint, point_center_2d, mRectFeaturePoints (where upstream assigns it: at least 4 points), bad, and bOnEdge where upstream
// sets it; then the bad objects leave the vector, without delete, as upstream (:1949-1973).
//
// One deviation: isBad() is read ONCE per keypoint, in front of the call.  Upstream reads it again in ComputeMeanAndStandardFrame (src/Object.cc:70, :87) while
// LocalMapping may be culling points; a point that turns bad between those reads leaves upstream's list (and its sum) and stays in this one for the frame.
// (sum_pos_3d is assigned, not added to: upstream's objects come to step 2 with a zero sum, src/Tracking.cc:1737-1741.)
//
// Obj2dT: mBoxRect (x, y, width, height), mScore, Obj_c_MapPonits (std::vector<MapPointT*>), sum_pos_3d and _Pos (assignable from cv::Mat), mStandar_x/y/z,
// mCountMappoint, point_center_2d and mRectFeaturePoints (constructible from two floats / four ints), bad, bOnEdge.  FrameT: N, mvpMapPoints, mvKeysUn
// (cv::KeyPoint), mTcw with at<float>(r, c), fx, fy, cx, cy, mnId.  MapPointT: isBad(), GetWorldPos() with at<float>(0..2), object_view, frame_id, feature.
#pragma once

#include <cstddef>
#include <cstdint>
#include <unordered_map>
#include <vector>

#include "adapter_detail.h"

namespace eaofusion {

namespace frame_objects_detail {

// one frame's arrays, alive for the call
struct Gathered {
    std::vector<float> kp_x, kp_y, xyz, score;
    std::vector<int32_t> mp_id, boxes;
};

template <class Obj2dT, class FrameT>
void gather(const std::vector<Obj2dT*>& objs, const FrameT& frame, int cols, int rows, Gathered& g, eao_frame_objects_desc& d) {
    const int N = (int)frame.N;
    g.kp_x.resize((size_t)N); g.kp_y.resize((size_t)N); g.mp_id.assign((size_t)N, -1); g.xyz.assign(3 * (size_t)N, 0.f);
    std::unordered_map<const void*, int32_t> id;      // equal ids = one MapPoint
    for (int i = 0; i < N; i++) {
        g.kp_x[(size_t)i] = frame.mvKeysUn[(size_t)i].pt.x;
        g.kp_y[(size_t)i] = frame.mvKeysUn[(size_t)i].pt.y;
        const auto* pMP = frame.mvpMapPoints[(size_t)i];
        if (!pMP || pMP->isBad()) continue;      // (:3038, :3042: the one snapshot)
        g.mp_id[(size_t)i] = id.emplace((const void*)pMP, (int32_t)id.size()).first->second;
        float p[3];
        detail::read3(pMP->GetWorldPos(), p);
        for (int a = 0; a < 3; a++) g.xyz[3 * (size_t)i + a] = p[a];
    }
    for (const Obj2dT* o : objs) {
        g.boxes.push_back((int32_t)o->mBoxRect.x); g.boxes.push_back((int32_t)o->mBoxRect.y);
        g.boxes.push_back((int32_t)o->mBoxRect.width); g.boxes.push_back((int32_t)o->mBoxRect.height);
        g.score.push_back((float)o->mScore);
    }
    d.n_kp = N; d.kp_x = g.kp_x.data(); d.kp_y = g.kp_y.data(); d.mp_id = g.mp_id.data(); d.mp_xyz = g.xyz.data();
    d.n_box = (int32_t)objs.size(); d.boxes = g.boxes.data(); d.score = g.score.data();
    detail::read44(frame.mTcw, d.Tcw);
    d.fx = frame.fx; d.fy = frame.fy; d.cx = frame.cx; d.cy = frame.cy;
    d.cols = (int32_t)cols; d.rows = (int32_t)rows;
}

// the list capacity no frame can exceed: every box holds every keypoint with a map point
inline int64_t worst_case(const Gathered& g) {
    int64_t valid = 0;
    for (int32_t v : g.mp_id) valid += v >= 0 ? 1 : 0;
    return valid * (int64_t)g.score.size();
}

template <class Obj2dT, class FrameT>
void scatter(std::vector<Obj2dT*>& objs, FrameT& frame, const eao_frame_object_record* rec, const int32_t* aStart, const int32_t* assigned, const int32_t* kStart,
             const int32_t* kept) {
    const size_t M = objs.size();
    // step 2's writes on the map points, keypoint by keypoint and box by box (:3044-3053): the lists ascend, so a cursor per box finds the hits of keypoint i
    std::vector<int32_t> cursor(aStart, aStart + M);
    for (int32_t i = 0; i < (int32_t)frame.N; i++)
        for (size_t k = 0; k < M; k++)
            if (cursor[k] < aStart[k + 1] && assigned[cursor[k]] == i) {
                cursor[k]++;
                auto* pMP = frame.mvpMapPoints[(size_t)i];
                pMP->object_view = true;
                pMP->frame_id.insert(frame.mnId);
                pMP->feature = frame.mvKeysUn[(size_t)i];
            }
    for (size_t k = 0; k < M; k++) {
        Obj2dT& o = *objs[k];
        const eao_frame_object_record& r = rec[k];
        o.Obj_c_MapPonits.clear();
        for (int32_t p = kStart[k]; p < kStart[k + 1]; p++) o.Obj_c_MapPonits.push_back(frame.mvpMapPoints[(size_t)kept[p]]);
        o.sum_pos_3d = detail::mat_of(r.sum_pos, 3, 1);
        o._Pos = detail::mat_of(r.pos, 3, 1);
        o.mStandar_x = r.std[0]; o.mStandar_y = r.std[1]; o.mStandar_z = r.std[2];
        o.mCountMappoint = (int)r.n;
        o.point_center_2d = decltype(o.point_center_2d)(r.center_2d[0], r.center_2d[1]);
        if (r.has_feature_rect) o.mRectFeaturePoints = decltype(o.mRectFeaturePoints)(r.feature_rect[0], r.feature_rect[1], r.feature_rect[2], r.feature_rect[3]);
        if (r.bad) o.bad = true;
        if (r.on_edge) o.bOnEdge = true;
    }
    // :1949-1973: the bad objects leave the vector (no delete, as upstream)
    size_t keep = 0;
    for (size_t k = 0; k < M; k++)
        if (!objs[k]->bad) objs[keep++] = objs[k];
    objs.resize(keep);
}

}  // namespace frame_objects_detail

// Offline replay: frames[f] with its detections objs[f], all frames in ONE library call.  Returns the number of objects left over all frames, or -1 when the
// library refused the call (eao_last_error() says why; nothing is written).
template <class Obj2dT, class FrameT>
int BuildFrameObjects(std::vector<std::vector<Obj2dT*>*>& objs, std::vector<FrameT*>& frames, int cols, int rows) {
    namespace fd = frame_objects_detail;
    if (objs.size() != frames.size()) return -1;
    const size_t F = frames.size();
    std::vector<fd::Gathered> g(F);
    std::vector<eao_frame_objects_desc> d(F);
    int64_t cap = 0;
    size_t boxes = 0;
    for (size_t f = 0; f < F; f++) {
        fd::gather(*objs[f], *frames[f], cols, rows, g[f], d[f]);
        cap += fd::worst_case(g[f]);
        boxes += objs[f]->size();
    }
    std::vector<eao_frame_object_record> rec(boxes);
    std::vector<int32_t> aStart(boxes + 1), kStart(boxes + 1), assigned((size_t)cap), kept((size_t)cap);
    const eao_frame_objects_out out = {rec.data(), aStart.data(), assigned.data(), cap, kStart.data(), kept.data(), cap};
    if (eao_frame_objects_batch((int32_t)F, d.data(), &out) != EAO_OK) return -1;
    int left = 0;
    size_t b = 0;
    for (size_t f = 0; f < F; f++) {
        const size_t M = objs[f]->size();
        fd::scatter(*objs[f], *frames[f], rec.data() + b, aStart.data() + b, assigned.data(), kStart.data() + b, kept.data());
        left += (int)objs[f]->size();
        b += M;
    }
    return left;
}

// src/Tracking.cc:1768-1973 for the current frame.  Returns the number of objects left in objs_2d, or -1 when the library refused the call.
template <class Obj2dT, class FrameT>
int BuildFrameObjects(std::vector<Obj2dT*>& objs_2d, FrameT& frame, int cols, int rows) {
    std::vector<std::vector<Obj2dT*>*> objs(1, &objs_2d);
    std::vector<FrameT*> frames(1, &frame);
    return BuildFrameObjects(objs, frames, cols, rows);      // (the overload above: the more specialised of the two)
}

}  // namespace eaofusion
