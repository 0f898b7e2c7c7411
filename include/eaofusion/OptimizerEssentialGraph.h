// OptimizerEssentialGraph.h -- Optimizer::OptimizeEssentialGraph (reference src/Optimizer.cc:1141-1435) on top of the C-ABI
// (eao_optimize_essential_graph).
//
// The walk over the map (src/Optimizer.cc:1157-1344) stays on the host, restated over the reference's member names so that the template
// instantiates against the real Map / KeyFrame / MapPoint / MapPlane / g2o::Sim3 in a checkout; optimize(20), the
// SE3 recovery and the point correction are one call into libeaofusion_hip.so; the write-back (:1350-1434) happens here under
// pMap->mMutexMapUpdate.  The header needs no Eigen: a g2o::Sim3 is read through rotation().x() .. w(), translation()[i] and scale(),
// and g2o::Sim3(Rcw, tcw, 1.0) of a keyframe outside CorrectedSim3 is formed by Eigen's Quaterniond(Matrix3d) rule written out below.
//
//   // src/Optimizer_hip_essential_graph.cc in an EAO-Fusion checkout (replaces the function body in src/Optimizer.cc):
//   #include <eaofusion/OptimizerEssentialGraph.h>
//   void ORB_SLAM2::Optimizer::OptimizeEssentialGraph(Map* pMap, KeyFrame* pLoopKF, KeyFrame* pCurKF, const LoopClosing::KeyFrameAndPose& NonCorrectedSim3,
//           const LoopClosing::KeyFrameAndPose& CorrectedSim3, const map<KeyFrame*, set<KeyFrame*> >& LoopConnections, const bool& bFixScale)
//   { eaofusion::OptimizeEssentialGraph<MapPoint, MapPlane>(pMap, pLoopKF, pCurKF, NonCorrectedSim3, CorrectedSim3, LoopConnections, bFixScale); }
//
// Bad keyframes: a keyframe with isBad() gets no vertex (as upstream, :1173), and an edge that would touch one is skipped; a map point or
// plane whose reference keyframe has no vertex comes back as it is.  Upstream never meets either case -- Map::EraseKeyFrame removes a bad
// keyframe from GetAllKeyFrames(), SetBadFlag() takes it out of the spanning tree, the loop edges and the covisibility graph, and the
// SE3 recovery loop (:1353-1371) would dereference a null vertex if it did.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <map>
#include <mutex>
#include <set>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "adapter_detail.h"

namespace eaofusion {

// The flattened graph and where each of its rows came from.
struct EssentialGraphWalk {
    std::vector<double> Scw, Snc;          // 8 per vertex
    std::vector<uint8_t> has_nc;
    std::vector<int32_t> edges;            // (i, j, kind) in the order upstream adds them
    std::vector<float> Xw;                 // the good map points, then the good map planes' first three coefficients
    std::vector<int32_t> ref;
    std::vector<int> kf_index;             // vertex -> index in vpKFs
    std::vector<int> point_index;          // point row -> index in vpMPs
    std::vector<int> plane_index;          // plane row (behind the points) -> index in vpMPlanes
    std::vector<unsigned long> ids;        // vertex -> mnId
    int fixed = -1, fix_scale = 0;
    eao_essential_graph_problem problem() const {
        eao_essential_graph_problem p;
        p.n = (int32_t)ids.size(); p.fixed = fixed; p.fix_scale = fix_scale;
        p.Scw = Scw.data(); p.has_nc = has_nc.data(); p.Snc = Snc.data();
        p.n_edges = (int32_t)(edges.size() / 3); p.edges = edges.data();
        p.n_points = (int32_t)ref.size(); p.Xw = Xw.data(); p.ref = ref.data();
        return p;
    }
};

namespace essential_graph_detail {
// Eigen::Quaterniond(const Matrix3d&): the trace branch, else the largest diagonal (a strict > moves to the later index)
inline void quat_of_rotation(const double m[9], double q[4]) {      // q: x, y, z, w
    double t = m[0] + m[4] + m[8];
    if (t > 0) {
        t = std::sqrt(t + 1.0);
        q[3] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (m[7] - m[5]) * t; q[1] = (m[2] - m[6]) * t; q[2] = (m[3] - m[1]) * t;
        return;
    }
    int i = 0;
    if (m[4] > m[0]) i = 1;
    if (m[8] > m[i * 4]) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    t = std::sqrt(m[i * 4] - m[j * 4] - m[k * 4] + 1.0);
    q[i] = 0.5 * t;
    t = 0.5 / t;
    q[3] = (m[k * 3 + j] - m[j * 3 + k]) * t;
    q[j] = (m[j * 3 + i] + m[i * 3 + j]) * t;
    q[k] = (m[k * 3 + i] + m[i * 3 + k]) * t;
}
template <class Sim3T> inline void push_sim3(const Sim3T& S, std::vector<double>& out) {
    out.push_back(S.rotation().x()); out.push_back(S.rotation().y()); out.push_back(S.rotation().z()); out.push_back(S.rotation().w());
    for (int k = 0; k < 3; k++) out.push_back(S.translation()[k]);
    out.push_back(S.scale());
}
template <class M> inline void push_pose(const M& R, const M& t, std::vector<double>& out) {      // g2o::Sim3(toMatrix3d(R), toVector3d(t), 1.0)
    double m[9], q[4];
    for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) m[r * 3 + c] = R.template at<float>(r, c);
    quat_of_rotation(m, q);
    for (int k = 0; k < 4; k++) out.push_back(q[k]);
    for (int k = 0; k < 3; k++) out.push_back(t.template at<float>(k));
    out.push_back(1.0);
}
}  // namespace essential_graph_detail

// The host walk of src/Optimizer.cc:1157-1344: the vertices, then the loop-connection edges (kind 0), then per keyframe its spanning-tree
// edge, its loop edges and its covisibility edges (kind 1), with the filters as upstream writes them; then the good map points and planes
// with the keyframe each is corrected through (:1381-1390, :1414-1423).  vpKFs / vpMPs / vpMPlanes: the map's GetAllKeyFrames() / GetAllMapPoints() /
// GetAllMapPlanes(), taken ONCE by the caller as upstream takes them (:1157-1159) -- the walk's indices point into these vectors, and so does the write-back.
template <class MapPointT, class MapPlaneT, class KeyFrameT, class PoseMapT, class LoopMapT>
EssentialGraphWalk WalkEssentialGraph(const std::vector<KeyFrameT*>& vpKFs, const std::vector<MapPointT*>& vpMPs, const std::vector<MapPlaneT*>& vpMPlanes,
                                      KeyFrameT* pLoopKF, KeyFrameT* pCurKF, const PoseMapT& NonCorrectedSim3, const PoseMapT& CorrectedSim3,
                                      const LoopMapT& LoopConnections, bool bFixScale) {
    namespace D = essential_graph_detail;
    EssentialGraphWalk w;
    w.fix_scale = bFixScale ? 1 : 0;
    const int minFeat = 100;
    std::map<unsigned long, int> vertexOf;      // mnId -> vertex (upstream: vectors of nMaxKFid + 1 entries indexed by mnId)
    // Set KeyFrame vertices
    for (size_t i = 0, iend = vpKFs.size(); i < iend; i++) {
        KeyFrameT* pKF = vpKFs[i];
        if (pKF->isBad()) continue;
        const int v = (int)w.ids.size();
        vertexOf[pKF->mnId] = v;
        w.ids.push_back(pKF->mnId);
        w.kf_index.push_back((int)i);
        typename PoseMapT::const_iterator it = CorrectedSim3.find(pKF);
        if (it != CorrectedSim3.end()) D::push_sim3(it->second, w.Scw);
        else D::push_pose(pKF->GetRotation(), pKF->GetTranslation(), w.Scw);
        typename PoseMapT::const_iterator itn = NonCorrectedSim3.find(pKF);
        w.has_nc.push_back(itn != NonCorrectedSim3.end() ? 1 : 0);
        if (itn != NonCorrectedSim3.end()) D::push_sim3(itn->second, w.Snc);
        else w.Snc.insert(w.Snc.end(), w.Scw.end() - 8, w.Scw.end());
        if (pKF == pLoopKF) w.fixed = v;
    }
    auto vertex = [&](KeyFrameT* pKF) -> int {
        if (!pKF || pKF->isBad()) return -1;
        std::map<unsigned long, int>::const_iterator it = vertexOf.find(pKF->mnId);
        return it == vertexOf.end() ? -1 : it->second;
    };
    auto add_edge = [&](int i, int j, int kind) { w.edges.push_back(i); w.edges.push_back(j); w.edges.push_back(kind); };
    std::set<std::pair<unsigned long, unsigned long> > sInsertedEdges;
    // Set Loop edges
    for (typename LoopMapT::const_iterator mit = LoopConnections.begin(), mend = LoopConnections.end(); mit != mend; mit++) {
        KeyFrameT* pKF = mit->first;
        const unsigned long nIDi = pKF->mnId;
        const std::set<KeyFrameT*>& spConnections = mit->second;
        for (typename std::set<KeyFrameT*>::const_iterator sit = spConnections.begin(), send = spConnections.end(); sit != send; sit++) {
            const unsigned long nIDj = (*sit)->mnId;
            if ((nIDi != pCurKF->mnId || nIDj != pLoopKF->mnId) && pKF->GetWeight(*sit) < minFeat) continue;
            const int vi = vertex(pKF), vj = vertex(*sit);
            if (vi < 0 || vj < 0) continue;      // (a bad keyframe: see the head of this file)
            add_edge(vi, vj, 0);
            sInsertedEdges.insert(std::make_pair(std::min(nIDi, nIDj), std::max(nIDi, nIDj)));
        }
    }
    // Set normal edges
    for (size_t i = 0, iend = vpKFs.size(); i < iend; i++) {
        KeyFrameT* pKF = vpKFs[i];
        const int vi = vertex(pKF);
        if (vi < 0) continue;
        KeyFrameT* pParentKF = pKF->GetParent();
        // Spanning tree edge
        if (pParentKF) {
            const int vj = vertex(pParentKF);
            if (vj >= 0) add_edge(vi, vj, 1);
        }
        // Loop edges
        const std::set<KeyFrameT*> sLoopEdges = pKF->GetLoopEdges();
        for (typename std::set<KeyFrameT*>::const_iterator sit = sLoopEdges.begin(), send = sLoopEdges.end(); sit != send; sit++) {
            KeyFrameT* pLKF = *sit;
            if (pLKF->mnId < pKF->mnId) {
                const int vl = vertex(pLKF);
                if (vl >= 0) add_edge(vi, vl, 1);
            }
        }
        // Covisibility graph edges
        const std::vector<KeyFrameT*> vpConnectedKFs = pKF->GetCovisiblesByWeight(minFeat);
        for (typename std::vector<KeyFrameT*>::const_iterator vit = vpConnectedKFs.begin(); vit != vpConnectedKFs.end(); vit++) {
            KeyFrameT* pKFn = *vit;
            if (pKFn && pKFn != pParentKF && !pKF->hasChild(pKFn) && !sLoopEdges.count(pKFn)) {
                if (!pKFn->isBad() && pKFn->mnId < pKF->mnId) {
                    if (sInsertedEdges.count(std::make_pair(std::min(pKF->mnId, pKFn->mnId), std::max(pKF->mnId, pKFn->mnId)))) continue;
                    const int vn = vertex(pKFn);
                    if (vn >= 0) add_edge(vi, vn, 1);
                }
            }
        }
    }
    // the points and planes the correction pass visits, each with the vertex of the keyframe it goes through
    auto reference_of = [&](auto* pMP) -> int {
        unsigned long nIDr;
        if (pMP->mnCorrectedByKF == pCurKF->mnId) nIDr = pMP->mnCorrectedReference;
        else nIDr = pMP->GetReferenceKeyFrame()->mnId;
        std::map<unsigned long, int>::const_iterator it = vertexOf.find(nIDr);
        return it == vertexOf.end() ? -1 : it->second;
    };
    for (size_t i = 0, iend = vpMPs.size(); i < iend; i++) {
        MapPointT* pMP = vpMPs[i];
        if (pMP->isBad()) continue;
        detail::push3(pMP->GetWorldPos(), w.Xw);
        w.ref.push_back(reference_of(pMP));
        w.point_index.push_back((int)i);
    }
    for (size_t i = 0, iend = vpMPlanes.size(); i < iend; i++) {
        MapPlaneT* pMP = vpMPlanes[i];
        if (pMP->isBad()) continue;
        detail::push3(pMP->GetWorldPos(), w.Xw);      // (four coefficients; the fork's loop reads the first three through Converter::toVector3d)
        w.ref.push_back(reference_of(pMP));
        w.plane_index.push_back((int)i);
    }
    return w;
}

// Optimizer::OptimizeEssentialGraph: SetPose(Tiw) on every keyframe with a vertex, SetWorldPos + UpdateNormalAndDepth on every good map
// point, SetWorldPos (a 3 x 1 matrix, as the fork wrote it; no UpdateNormalAndDepth) on every good map plane.
template <class MapPointT, class MapPlaneT, class MapT, class KeyFrameT, class PoseMapT, class LoopMapT>
void OptimizeEssentialGraph(MapT* pMap, KeyFrameT* pLoopKF, KeyFrameT* pCurKF, const PoseMapT& NonCorrectedSim3, const PoseMapT& CorrectedSim3,
                            const LoopMapT& LoopConnections, const bool& bFixScale) {
    const std::vector<KeyFrameT*> vpKFs = pMap->GetAllKeyFrames();
    const std::vector<MapPointT*> vpMPs = pMap->GetAllMapPoints();
    const std::vector<MapPlaneT*> vpMPlanes = pMap->GetAllMapPlanes();
    const EssentialGraphWalk w = WalkEssentialGraph<MapPointT, MapPlaneT>(vpKFs, vpMPs, vpMPlanes, pLoopKF, pCurKF, NonCorrectedSim3, CorrectedSim3, LoopConnections, bFixScale);
    if (w.fixed < 0) throw std::runtime_error("OptimizeEssentialGraph: pLoopKF is not a good keyframe of the map");
    const eao_essential_graph_problem p = w.problem();
    std::vector<double> Scw(w.ids.size() * 8);
    std::vector<float> Tiw(w.ids.size() * 16), Xc(w.ref.size() * 3 + 3);
    eao_essential_graph_result r = eao_essential_graph_result();
    r.Scw = Scw.data(); r.Tiw = Tiw.data(); r.Xw_corrected = Xc.data();
    detail::check(eao_optimize_essential_graph(&p, &r), "eao_optimize_essential_graph");
    std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);
    // SE3 Pose Recovering. Sim3:[sR t;0 1] -> SE3:[R t/s;0 1]
    for (size_t v = 0; v < w.ids.size(); v++) {
        vpKFs[w.kf_index[v]]->SetPose(detail::mat_of(&Tiw[v * 16], 4, 4));
    }
    // Correct points
    for (size_t k = 0; k < w.point_index.size(); k++) {
        MapPointT* pMP = vpMPs[w.point_index[k]];
        pMP->SetWorldPos(detail::mat_of(&Xc[k * 3], 3, 1));
        pMP->UpdateNormalAndDepth();
    }
    // Correct planes
    const size_t base = w.point_index.size();
    for (size_t k = 0; k < w.plane_index.size(); k++) {
        MapPlaneT* pMP = vpMPlanes[w.plane_index[k]];
        pMP->SetWorldPos(detail::mat_of(&Xc[(base + k) * 3], 3, 1));
    }
}

}  // namespace eaofusion
