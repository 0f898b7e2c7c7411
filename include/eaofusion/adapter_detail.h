// adapter_detail.h -- what the class-surface headers of this directory share: the status check, the reads and writes between cv::Mat and the flat
// float arrays of the C-ABI, the epipole of SearchForTriangulation, the DBoW2 FeatureVector flattening and the RANSAC index draw of PnPsolver / Sim3Solver.
// Header-only, no state.  It travels with the adapters (and with cv_compat.h) into a checkout; nothing outside this directory includes it.
//
// Every matrix helper is a template on the matrix type and reads through m.template at<float>(...): cv::Mat, the stand-in of cv_compat.h and the `auto`
// results of a stand-in's accessors all fit.  A vector is read with the single index at<float>(k), which is right for n x 1 and for 1 x n.
#pragma once

#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../eao_fusion.h"
#include "cv_compat.h"

namespace eaofusion {
namespace detail {

inline void check(eao_status st, const char* what) {
    if (st != EAO_OK) throw std::runtime_error(std::string(what) + ": " + eao_last_error());
}

// ---- matrix -> floats (row-major)
template <class M> inline void read44(const M& m, float* out) {
    for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) out[r * 4 + c] = m.template at<float>(r, c);
}
template <class M> inline void read33(const M& m, float* out) {
    for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) out[r * 3 + c] = m.template at<float>(r, c);
}
template <class M> inline void read3(const M& v, float* out) {
    for (int k = 0; k < 3; k++) out[k] = v.template at<float>(k);
}
template <class M> inline void read4(const M& v, float* out) {
    for (int k = 0; k < 4; k++) out[k] = v.template at<float>(k);
}
template <class M> inline void push3(const M& v, std::vector<float>& out) {
    for (int k = 0; k < 3; k++) out.push_back(v.template at<float>(k));
}
template <class M> inline void push4(const M& v, std::vector<float>& out) {
    for (int k = 0; k < 4; k++) out.push_back(v.template at<float>(k));
}
// GetRotation() / GetTranslation() -> [R t; 0 0 0 1]
template <class MR, class Mt> inline void read_pose(const MR& R, const Mt& t, float* out) {
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) out[r * 4 + c] = R.template at<float>(r, c);
        out[r * 4 + 3] = t.template at<float>(r);
    }
    out[12] = out[13] = out[14] = 0.f; out[15] = 1.f;
}
// mK -> fx, fy, cx, cy
template <class M> inline void read_intrinsics(const M& K, float* out) {
    out[0] = K.template at<float>(0, 0); out[1] = K.template at<float>(1, 1);
    out[2] = K.template at<float>(0, 2); out[3] = K.template at<float>(1, 2);
}

// ---- floats -> matrix
inline cv::Mat mat_of(const float* v, int rows, int cols) {
    cv::Mat m(rows, cols, CV_32F);
    for (int r = 0; r < rows; r++)
        for (int c = 0; c < cols; c++) m.at<float>(r, c) = v[r * cols + c];
    return m;
}
template <class M> inline void write44(M& m, const float* v) {
    for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) m.template at<float>(r, c) = v[r * 4 + c];
}
template <class M> inline void write_vec(M& m, const float* v, int n) {
    for (int k = 0; k < n; k++) m.template at<float>(k) = v[k];
}

// The epipole of the first camera in the second image (reference src/ORBmatcher.cc:663-670): C2 = R2w * Cw + t2w as cv::gemm forms it -- a double
// accumulator over k = 0, 1, 2, the translation added in double, ONE rounding to float -- then the projection in float.  The searches behind it are held
// to the reference bit for bit, so the order of these operations is part of the interface.
template <class MC, class MR, class Mt>
inline void epipole(const MC& Cw, const MR& R2w, const Mt& t2w, float fx, float fy, float cx, float cy, float& ex, float& ey) {
    float C2[3];
    for (int r = 0; r < 3; r++) {
        double acc = 0;
        for (int k = 0; k < 3; k++) acc += (double)R2w.template at<float>(r, k) * (double)Cw.template at<float>(k);
        C2[r] = (float)(acc + (double)t2w.template at<float>(r));
    }
    const float invz = 1.0f / C2[2];
    ex = fx * C2[0] * invz + cx; ey = fy * C2[1] * invz + cy;
}

// DBoW2::FeatureVector (std::map<node id, std::vector<keypoint index>>) as the C-ABI takes it; the view points into the caller's arrays
struct FeatVecArrays { std::vector<uint32_t> id, index; std::vector<int32_t> start; };
template <class FeatVecT>
inline eao_feature_vector flatten(const FeatVecT& fv, FeatVecArrays& a) {
    a.id.clear(); a.index.clear(); a.start.assign(1, 0);
    for (typename FeatVecT::const_iterator it = fv.begin(); it != fv.end(); ++it) {
        a.id.push_back((uint32_t)it->first);
        for (size_t k = 0; k < it->second.size(); k++) a.index.push_back((uint32_t)it->second[k]);
        a.start.push_back((int32_t)a.index.size());
    }
    eao_feature_vector f;
    f.n_nodes = (int32_t)a.id.size(); f.node_id = a.id.data(); f.node_start = a.start.data(); f.index = a.index.data();
    return f;
}

// The sampling loop of PnPsolver::iterate (reference src/PnPsolver.cc:188-201) and Sim3Solver::iterate (src/Sim3Solver.cc:163-177): k indices out of
// 0 .. N-1 for each of nHyp hypotheses, sets[h * k + i] the i-th of hypothesis h.  Restated WITH upstream's quirk: the slot that is overwritten with the last
// available index is vAvailableIndices[idx], idx being the drawn VALUE, not the drawn position randi -- so a set with a repeated index is reachable, upstream
// and here.  (Initializer's loop, src/Initializer.cc:78-97, overwrites the position and has no such repeat: it is a different draw and stays in Initializer.h.)
// Where idx is past the shrunken size upstream's write lands in the vector's spare capacity and is never read; the buffer here keeps its size N.
template <class RandomT>
inline void draw_sets(int N, int k, int nHyp, int32_t* sets) {
    std::vector<size_t> vAvailableIndices((size_t)N);
    for (int h = 0; h < nHyp; h++) {
        for (int i = 0; i < N; i++) vAvailableIndices[i] = (size_t)i;      // = mvAllIndices
        size_t size = (size_t)N;
        for (short i = 0; i < k; ++i) {
            const int randi = RandomT::RandomInt(0, (int)size - 1);
            const int idx = (int)vAvailableIndices[randi];
            sets[(size_t)h * k + i] = idx;
            vAvailableIndices[idx] = vAvailableIndices[size - 1];           // the drawn VALUE as position: upstream's quirk, kept
            size--;
        }
    }
}

}  // namespace detail
}  // namespace eaofusion
