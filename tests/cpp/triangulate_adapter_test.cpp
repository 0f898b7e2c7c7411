// Drives include/eaofusion/LocalMapping.h (NewMapPoints::TriangulateMatches over host arrays, NewMapPoints::CreateNewMapPointsBatch over keyframe handles) against
// stand-ins of the reference's KeyFrame with the member names src/LocalMapping.cc:211-454 and src/KeyFrame.cc:654-670 use.  Reads a scene written by
// tests/test_gpu_triangulation.py, asserts what the two forms owe each other and the dropped duplicates, and writes every accepted pair; the Python side compares
// them with the C-ABI called directly.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <map>
#include <set>
#include <vector>

#include <eaofusion/LocalMapping.h>

struct MapPoint { int dummy = 0; };
static MapPoint g_some_point;

struct KeyFrame {
    int N = 0;
    float fx, fy, cx, cy, invfx, invfy, mb, mbf, mfScaleFactor = 1.2f;
    std::vector<cv::KeyPoint> mvKeys, mvKeysUn;
    std::vector<float> mvuRight, mvDepth, mvScaleFactors, mvLevelSigma2, mvInvLevelSigma2;
    cv::Mat mDescriptors;
    int mnMinX = 0, mnMinY = 0, mnMaxX = 640, mnMaxY = 480, mnGridCols = 64, mnGridRows = 48;
    float mfGridElementWidthInv = 64.f / 640.f, mfGridElementHeightInv = 48.f / 480.f, mfLogScaleFactor = 0;
    std::map<unsigned, std::vector<unsigned> > mFeatVec;
    std::vector<uint8_t> occupied;
    cv::Mat Rcw, tcw, Ow;
    MapPoint* GetMapPoint(size_t i) { return occupied[i] ? &g_some_point : nullptr; }
    cv::Mat GetRotation() { return Rcw.clone(); }
    cv::Mat GetTranslation() { return tcw.clone(); }
    cv::Mat GetCameraCenter() { return Ow.clone(); }
};

template <typename T> static void rd(std::ifstream& f, T* p, size_t n) { f.read(reinterpret_cast<char*>(p), n * sizeof(T)); }
template <typename T> static void wr(std::ofstream& f, const T* p, size_t n) { f.write(reinterpret_cast<const char*>(p), n * sizeof(T)); }

static void read_keyframe(std::ifstream& f, KeyFrame& K, const float* sf, const float* s2, const float* is2, float logsf) {
    int n = 0;
    rd(f, &n, 1);
    std::vector<float> x(n), y(n), ang(n), ur(n), depth(n), rx(n), ry(n);
    std::vector<int32_t> oct(n);
    std::vector<uint8_t> occ(n), desc((size_t)n * 32);
    rd(f, x.data(), n); rd(f, y.data(), n); rd(f, ang.data(), n); rd(f, ur.data(), n); rd(f, oct.data(), n); rd(f, occ.data(), n); rd(f, desc.data(), desc.size());
    rd(f, depth.data(), n); rd(f, rx.data(), n); rd(f, ry.data(), n);
    int nn = 0;
    rd(f, &nn, 1);
    std::vector<uint32_t> id(nn);
    std::vector<int32_t> st(nn + 1);
    rd(f, id.data(), nn); rd(f, st.data(), nn + 1);
    std::vector<uint32_t> idx(st[nn]);
    rd(f, idx.data(), idx.size());
    float cam[23];
    rd(f, cam, 23);
    K.N = n;
    K.mvKeys.resize(n); K.mvKeysUn.resize(n); K.mvuRight = ur; K.mvDepth = depth; K.occupied = occ;
    for (int i = 0; i < n; i++) {
        K.mvKeysUn[i].pt.x = x[i]; K.mvKeysUn[i].pt.y = y[i]; K.mvKeysUn[i].angle = ang[i]; K.mvKeysUn[i].octave = oct[i];
        K.mvKeys[i] = K.mvKeysUn[i]; K.mvKeys[i].pt.x = rx[i]; K.mvKeys[i].pt.y = ry[i];
    }
    K.mDescriptors = cv::Mat(n, 32, CV_8U);
    for (int i = 0; i < n; i++) std::memcpy(K.mDescriptors.ptr(i), &desc[(size_t)i * 32], 32);
    for (int k = 0; k < nn; k++) K.mFeatVec[id[k]] = std::vector<unsigned>(idx.begin() + st[k], idx.begin() + st[k + 1]);
    K.Rcw = cv::Mat(3, 3, CV_32F); K.tcw = cv::Mat(3, 1, CV_32F); K.Ow = cv::Mat(3, 1, CV_32F);
    for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) K.Rcw.at<float>(r, c) = cam[r * 3 + c]; K.tcw.at<float>(r) = cam[9 + r]; K.Ow.at<float>(r) = cam[12 + r]; }
    K.fx = cam[15]; K.fy = cam[16]; K.cx = cam[17]; K.cy = cam[18]; K.invfx = cam[19]; K.invfy = cam[20]; K.mb = cam[21]; K.mbf = cam[22];
    K.mvScaleFactors.assign(sf, sf + 8); K.mvLevelSigma2.assign(s2, s2 + 8); K.mvInvLevelSigma2.assign(is2, is2 + 8); K.mfLogScaleFactor = logsf;
    K.mfScaleFactor = sf[1];
}

typedef std::vector<std::vector<eaofusion::NewMapPoint> > Points;
typedef std::vector<std::vector<std::pair<size_t, size_t> > > Pairs;

static void write_points(std::ofstream& out, const Points& P, size_t dropped) {
    const int32_t d = (int32_t)dropped;
    wr(out, &d, 1);
    for (const auto& row : P) {
        const int32_t n = (int32_t)row.size();
        wr(out, &n, 1);
        for (const auto& p : row) {
            const int32_t rec[3] = {(int32_t)p.idx1, (int32_t)p.idx2, (int32_t)p.verdict};
            wr(out, rec, 3);
            const float X[3] = {p.x3D.at<float>(0), p.x3D.at<float>(1), p.x3D.at<float>(2)};
            wr(out, X, 3);
        }
    }
}

static bool same(const Points& A, const Points& B) {
    if (A.size() != B.size()) return false;
    for (size_t q = 0; q < A.size(); q++) {
        if (A[q].size() != B[q].size()) return false;
        for (size_t j = 0; j < A[q].size(); j++) {
            const auto &a = A[q][j], &b = B[q][j];
            if (a.idx1 != b.idx1 || a.idx2 != b.idx2 || a.verdict != b.verdict) return false;
            for (int k = 0; k < 3; k++) if (std::memcmp(&a.x3D.at<float>(k), &b.x3D.at<float>(k), 4)) return false;
        }
    }
    return true;
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    std::ifstream in(argv[1], std::ios::binary);
    std::ofstream out(argv[2], std::ios::binary);
    float sf[8], s2[8], is2[8], logsf;
    int nb = 0;
    rd(in, sf, 8); rd(in, s2, 8); rd(in, is2, 8); rd(in, &logsf, 1); rd(in, &nb, 1);
    KeyFrame A;
    read_keyframe(in, A, sf, s2, is2, logsf);
    std::vector<KeyFrame> store(nb);
    std::vector<KeyFrame*> nbs(nb);
    std::vector<cv::Mat> vF(nb);
    for (int q = 0; q < nb; q++) {
        read_keyframe(in, store[q], sf, s2, is2, logsf);
        nbs[q] = &store[q];
        float F[9];
        rd(in, F, 9);
        vF[q] = cv::Mat(3, 3, CV_32F);
        for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) vF[q].at<float>(r, c) = F[r * 3 + c];
    }
    if (!in) { std::fprintf(stderr, "short scene file\n"); return 3; }

    // ---- host arrays: the batch search of round 4, then the loop
    eaofusion::NewMapPoints lm(0.6f, false);
    Pairs pairs;
    lm.SearchForTriangulationBatch(&A, nbs, vF, pairs, false);
    const Points viaArrays = lm.TriangulateMatches(&A, nbs, pairs);
    const size_t droppedArrays = lm.dropped;

    // ---- keyframe handles: one call
    eaofusion::KeyFrameHandles H;
    std::vector<const eao_keyframe*> hs;
    for (int q = 0; q < nb; q++) hs.push_back(H.of(nbs[q]));
    Pairs pairsH;
    const Points viaHandles = lm.CreateNewMapPointsBatch(H.of(&A), &A, hs, nbs, vF, false, &pairsH);
    const size_t droppedHandles = lm.dropped;

    if (pairsH != pairs) { std::fprintf(stderr, "CreateNewMapPointsBatch: the matched pairs differ from SearchForTriangulationBatch's\n"); return 3; }
    if (!same(viaArrays, viaHandles) || droppedArrays != droppedHandles) { std::fprintf(stderr, "the two forms return different points\n"); return 3; }
    // the dropped duplicates: no keypoint of the current keyframe receives two points in one call, every kept pair is one the search returned, in pair order,
    // and the scene does offer keypoints twice (the neighbours are variants of one keyframe)
    std::set<size_t> served;
    size_t offered = 0;
    for (int q = 0; q < nb; q++) {
        size_t at = 0;
        for (const auto& p : viaArrays[q]) {
            if (!served.insert(p.idx1).second) { std::fprintf(stderr, "keypoint %zu of the current keyframe received two points\n", p.idx1); return 3; }
            while (at < pairs[q].size() && pairs[q][at].first != p.idx1) at++;
            if (at == pairs[q].size() || pairs[q][at].second != p.idx2) { std::fprintf(stderr, "neighbour %d: a point for a pair the search did not return, or out of pair order\n", q); return 3; }
            if (A.GetMapPoint(p.idx1) || nbs[q]->GetMapPoint(p.idx2)) { std::fprintf(stderr, "a point on an occupied keypoint\n"); return 3; }
        }
        offered += pairs[q].size();
    }
    if (droppedArrays == 0) { std::fprintf(stderr, "no duplicate was dropped: the scene does not exercise the rule\n"); return 3; }
    // a handle that never received its depth is refused (the search-only upload of a keyframe class without mvDepth / mvKeys)
    {
        eao_frame_view v;
        std::memset(&v, 0, sizeof(v));
        float one = 1.f;
        v.scale_factors = &one; v.nlevels = 1; v.grid_cols = 64; v.grid_rows = 48; v.max_x = 640; v.max_y = 480; v.grid_inv_w = 0.1f; v.grid_inv_h = 0.1f;
        eao_feature_vector f;
        std::memset(&f, 0, sizeof(f));
        int32_t zero = 0;
        f.node_start = &zero;
        eao_keyframe* bare = nullptr;
        if (eao_keyframe_create(&v, &f, &bare) != EAO_OK) { std::fprintf(stderr, "eao_keyframe_create of an empty keyframe: %s\n", eao_last_error()); return 3; }
        const eao_tri_camera c = eaofusion::NewMapPoints::camera_of(A);
        const eao_keyframe* one_nb[1] = {hs[0]};
        float F[9] = {0, 0, 0, 0, 0, 1, 0, -1, 0}, e = 0;
        int32_t m = 0, nm = 0, vd = 0;
        float X[3];
        const eao_status st = eao_kf_create_new_map_points(bare, &c, 1, one_nb, &c, F, &e, &e, 0, 0, 1.8f, &m, &nm, &vd, X);
        eao_keyframe_destroy(bare);
        if (st != EAO_ERR_INVALID) { std::fprintf(stderr, "a handle without depth was not refused (status %d)\n", (int)st); return 3; }
    }
    write_points(out, viaArrays, droppedArrays);
    std::fprintf(stderr, "%zu pairs offered, %zu points, %zu duplicates dropped\n", offered, served.size(), droppedArrays);
    return 0;
}
