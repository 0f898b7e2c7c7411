// triangulate.hip -- the second half of LocalMapping::CreateNewMapPoints for MI355X (gfx950): triangulate and gate the matched pairs.
//
// Reference src/LocalMapping.cc:288-454 runs, per neighbour keyframe, a loop over the pairs SearchForTriangulation returned: parallax between the two rays, one of
// three ways to a point (linear triangulation with a 4 x 4 cv::SVD, KeyFrame::UnprojectStereo of either side -- src/KeyFrame.cc:654-670), then depth, reprojection
// and scale gates.  Every pair is independent, reads two keypoints and two camera records and leaves a verdict and three floats: one lane per pair.
//   * About one slot in ten of a neighbour's row of the match table holds a pair.  A wavefront owns kSeg consecutive slots: it writes the empty slots' verdicts,
//     ballot-compacts the populated ones into its own piece of LDS and then walks that list 64 pairs at a time -- no atomics, no barrier, nothing shared between
//     wavefronts, so a pair's result cannot depend on its neighbours or on the launch shape.
//   * The neighbour is blockIdx.y: both camera records and the array addresses sit in the kernel arguments and come through scalar loads.
//   * Arithmetic (tests/triangulation_reference.py is the same text in numpy): a cv::Mat product, Mat::dot and cv::norm accumulate in double in
//     storage order and round once; A's rows are float expressions; the right singular vector of the smallest singular value is the eigenvector of the smallest
//     eigenvalue of A^T A (double, from the float A) after kSweeps4 cyclic Jacobi sweeps -- a fixed count, no data-dependent loop -- rounded to float before the
//     w == 0 test; x3D / w multiplies by 1. / w in double and rounds once; the comparisons are written as upstream writes them (a NaN falls through the same gates).
#include <algorithm>
#include <cstring>
#include <vector>

#include "small_dense.h"
#include "triangulate_internal.h"

namespace {

// ---- the loop's literals (tests/golden/triangulation_constants.json, read from the reference text by tools/reference_literals.py; held to it by
// tests/test_triangulation_reference_cpu.py).  Nothing else in this file spells them.
constexpr double kLowParallaxCos = 0.9998;      // src/LocalMapping.cc:323  cosParallaxRays<0.9998
constexpr double kChi2Mono = 5.991;             // :378, :404  > 5.991*sigmaSquare
constexpr double kChi2Stereo = 7.8;             // :389, :415  > 7.8*sigmaSquare
[[maybe_unused]] constexpr float kRatioFactorBase = 1.5f;      // :236  ratioFactor = 1.5f*mfScaleFactor: the caller's product (ratio_factor of the entry points; include/eaofusion/LocalMapping.h forms it)
// ----

constexpr int kSeg = 256;        // match-table slots per wavefront
using eao::dense::smallest_eigenvector;      // small_dense.h: kSweeps4 cyclic Jacobi sweeps over the 4 x 4 A^T A

struct TriArgs {
    eao::tri::Side K1;
    eao_tri_camera cam1;
    float ratioFactor;
    int* verdict;      // nProb x K1.n
    float* x3d;        // nProb x K1.n x 3
    eao::tri::Prob P[eao::tri::kMaxProb];
};

// sum of three products of floats, in double, in storage order (cv::Mat::dot / the inner loop of a small float gemm / cv::norm's sum of squares)
__device__ __forceinline__ double ddot3(float a0, float a1, float a2, float b0, float b1, float b2) {
    double s = (double)a0 * (double)b0;
    s += (double)a1 * (double)b1;
    s += (double)a2 * (double)b2;
    return s;
}

// KeyFrame::UnprojectStereo (src/KeyFrame.cc:654-670); false: !(z > 0), upstream returns an empty Mat
__device__ __forceinline__ bool unproject_stereo(const eao_tri_camera& c, float z, float u, float v, float (&X)[3]) {
    if (!(z > 0)) return false;
    const float x = (u - c.cx) * z * c.invfx;
    const float y = (v - c.cy) * z * c.invfy;
#pragma unroll
    for (int i = 0; i < 3; i++) X[i] = (float)(ddot3(c.Rcw[i], c.Rcw[3 + i], c.Rcw[6 + i], x, y, z) + (double)c.Ow[i]);      // Rwc * x3Dc + Ow
    return true;
}

__global__ __launch_bounds__(256) void k_triangulate(TriArgs A) {
    __shared__ int s_list[4][kSeg];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, pb = blockIdx.y;
    const eao::tri::Side& K1 = A.K1;
    const eao::tri::Prob& P = A.P[pb];
    const eao::tri::Side& K2 = P.K2;
    const eao_tri_camera& c1 = A.cam1;
    const eao_tri_camera& c2 = P.cam2;
    const int n1 = K1.n;
    const int base = (blockIdx.x * 4 + w) * kSeg;
    if (base >= n1) return;      // (wave-uniform; no barrier below)
    int* verdict = A.verdict + (size_t)pb * n1;
    float* x3d = A.x3d + (size_t)pb * n1 * 3;
    // the populated slots of this wave's segment, compacted in slot order
    int cnt = 0;
#pragma unroll
    for (int it = 0; it < kSeg / 64; it++) {
        const int i = base + it * 64 + lane;
        int m = -1;
        if (i < n1) {
            m = P.match[i];
            if ((unsigned)m >= (unsigned)K2.n) m = -1;      // (the entry points refuse such a table; never an address)
            if (m < 0) {
                verdict[i] = EAO_TRI_EMPTY;
                x3d[3 * (size_t)i] = 0.f; x3d[3 * (size_t)i + 1] = 0.f; x3d[3 * (size_t)i + 2] = 0.f;
            }
        }
        const unsigned long long b = __ballot(m >= 0);
        if (m >= 0) s_list[w][cnt + __popcll(b & ((1ull << lane) - 1ull))] = i;
        cnt += __popcll(b);
    }
    eao::wave_sync();
    for (int j = lane; j < cnt; j += 64) {
        const int idx1 = s_list[w][j];
        const int idx2 = P.match[idx1];
        const float kx1 = K1.kx[idx1], ky1 = K1.ky[idx1], ur1 = K1.ur[idx1];
        const float kx2 = K2.kx[idx2], ky2 = K2.ky[idx2], ur2 = K2.ur[idx2];
        const int o1 = K1.oct[idx1], o2 = K2.oct[idx2];
        const bool st1 = ur1 >= 0, st2 = ur2 >= 0;
        // :303-320 parallax between the rays, and of the stereo pair that sees the point
        const float xn1x = (kx1 - c1.cx) * c1.invfx, xn1y = (ky1 - c1.cy) * c1.invfy;
        const float xn2x = (kx2 - c2.cx) * c2.invfx, xn2y = (ky2 - c2.cy) * c2.invfy;
        float r1[3], r2[3];
#pragma unroll
        for (int i = 0; i < 3; i++) {
            r1[i] = (float)ddot3(c1.Rcw[i], c1.Rcw[3 + i], c1.Rcw[6 + i], xn1x, xn1y, 1.0f);      // Rwc = Rcw.t()
            r2[i] = (float)ddot3(c2.Rcw[i], c2.Rcw[3 + i], c2.Rcw[6 + i], xn2x, xn2y, 1.0f);
        }
        const float cosR = (float)(ddot3(r1[0], r1[1], r1[2], r2[0], r2[1], r2[2]) /
                                   (sqrt(ddot3(r1[0], r1[1], r1[2], r1[0], r1[1], r1[2])) * sqrt(ddot3(r2[0], r2[1], r2[2], r2[0], r2[1], r2[2]))));
        float cps = cosR + 1;
        float cps1 = cps, cps2 = cps;
        if (st1) cps1 = (float)cos(2.0 * atan2((double)(c1.mb / 2), (double)K1.depth[idx1]));
        else if (st2) cps2 = (float)cos(2.0 * atan2((double)(c2.mb / 2), (double)K2.depth[idx2]));      // (`else if`: with stereo on both sides only keyframe 1's is computed, :317)
        cps = cps2 < cps1 ? cps2 : cps1;      // std::min(cps1, cps2)
        int accept, v = -1;
        float X[3] = {0.f, 0.f, 0.f};
        if (cosR < cps && cosR > 0 && (st1 || st2 || (double)cosR < kLowParallaxCos)) {
            // :325-341 linear triangulation
            accept = EAO_TRI_TRIANGULATED;
            float Am[4][4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const float a2 = k < 3 ? c1.Rcw[6 + k] : c1.tcw[2], a0 = k < 3 ? c1.Rcw[k] : c1.tcw[0], a1 = k < 3 ? c1.Rcw[3 + k] : c1.tcw[1];
                const float b2 = k < 3 ? c2.Rcw[6 + k] : c2.tcw[2], b0 = k < 3 ? c2.Rcw[k] : c2.tcw[0], b1 = k < 3 ? c2.Rcw[3 + k] : c2.tcw[1];
                Am[0][k] = xn1x * a2 - a0;
                Am[1][k] = xn1y * a2 - a1;
                Am[2][k] = xn2x * b2 - b0;
                Am[3][k] = xn2y * b2 - b1;
            }
            double S[4][4], ev[4];
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int k = i; k < 4; k++) {
                    double s = (double)Am[0][i] * (double)Am[0][k];
                    s += (double)Am[1][i] * (double)Am[1][k];
                    s += (double)Am[2][i] * (double)Am[2][k];
                    s += (double)Am[3][i] * (double)Am[3][k];
                    S[i][k] = s; S[k][i] = s;
                }
            smallest_eigenvector(S, ev);
            const float vf0 = (float)ev[0], vf1 = (float)ev[1], vf2 = (float)ev[2], vf3 = (float)ev[3];
            if (vf3 == 0) v = EAO_TRI_W_ZERO;
            else {
                const double iw = 1. / (double)vf3;
                X[0] = (float)((double)vf0 * iw); X[1] = (float)((double)vf1 * iw); X[2] = (float)((double)vf2 * iw);
            }
        } else if (st1 && cps1 < cps2) {
            accept = EAO_TRI_UNPROJECTED_1;
            if (!unproject_stereo(c1, K1.depth[idx1], K1.rawx[idx1], K1.rawy[idx1], X)) v = EAO_TRI_NO_DEPTH;
        } else if (st2 && cps2 < cps1) {
            accept = EAO_TRI_UNPROJECTED_2;
            if (!unproject_stereo(c2, K2.depth[idx2], K2.rawx[idx2], K2.rawy[idx2], X)) v = EAO_TRI_NO_DEPTH;
        } else {
            accept = EAO_TRI_LOW_PARALLAX;
            v = EAO_TRI_LOW_PARALLAX;
        }
        if (v < 0) {
            // :355-435 the gates, in upstream's order
            v = accept;
            const float z1 = (float)(ddot3(c1.Rcw[6], c1.Rcw[7], c1.Rcw[8], X[0], X[1], X[2]) + (double)c1.tcw[2]);
            const float z2 = (float)(ddot3(c2.Rcw[6], c2.Rcw[7], c2.Rcw[8], X[0], X[1], X[2]) + (double)c2.tcw[2]);
            if (z1 <= 0) v = EAO_TRI_BEHIND_1;
            else if (z2 <= 0) v = EAO_TRI_BEHIND_2;
            else {
                const float sig1 = K1.s2[o1], sig2 = K2.s2[o2];
                const float x1 = (float)(ddot3(c1.Rcw[0], c1.Rcw[1], c1.Rcw[2], X[0], X[1], X[2]) + (double)c1.tcw[0]);
                const float y1 = (float)(ddot3(c1.Rcw[3], c1.Rcw[4], c1.Rcw[5], X[0], X[1], X[2]) + (double)c1.tcw[1]);
                const float invz1 = (float)(1.0 / (double)z1);
                const float u1 = c1.fx * x1 * invz1 + c1.cx, v1 = c1.fy * y1 * invz1 + c1.cy;
                const float eX1 = u1 - kx1, eY1 = v1 - ky1;
                bool out1;
                if (!st1) out1 = (double)(eX1 * eX1 + eY1 * eY1) > kChi2Mono * (double)sig1;
                else {
                    const float u1r = u1 - c1.mbf * invz1;
                    const float eR1 = u1r - ur1;
                    out1 = (double)(eX1 * eX1 + eY1 * eY1 + eR1 * eR1) > kChi2Stereo * (double)sig1;
                }
                const float x2 = (float)(ddot3(c2.Rcw[0], c2.Rcw[1], c2.Rcw[2], X[0], X[1], X[2]) + (double)c2.tcw[0]);
                const float y2 = (float)(ddot3(c2.Rcw[3], c2.Rcw[4], c2.Rcw[5], X[0], X[1], X[2]) + (double)c2.tcw[1]);
                const float invz2 = (float)(1.0 / (double)z2);
                const float u2 = c2.fx * x2 * invz2 + c2.cx, v2 = c2.fy * y2 * invz2 + c2.cy;
                const float eX2 = u2 - kx2, eY2 = v2 - ky2;
                bool out2;
                if (!st2) out2 = (double)(eX2 * eX2 + eY2 * eY2) > kChi2Mono * (double)sig2;
                else {
                    const float u2r = u2 - c1.mbf * invz2;      // mpCurrentKeyFrame->mbf, as upstream writes it (:410)
                    const float eR2 = u2r - ur2;
                    out2 = (double)(eX2 * eX2 + eY2 * eY2 + eR2 * eR2) > kChi2Stereo * (double)sig2;
                }
                if (out1) v = EAO_TRI_REPROJ_1;
                else if (out2) v = EAO_TRI_REPROJ_2;
                else {
                    const float a0 = X[0] - c1.Ow[0], a1 = X[1] - c1.Ow[1], a2 = X[2] - c1.Ow[2];
                    const float b0 = X[0] - c2.Ow[0], b1 = X[1] - c2.Ow[1], b2 = X[2] - c2.Ow[2];
                    const float dist1 = (float)sqrt(ddot3(a0, a1, a2, a0, a1, a2)), dist2 = (float)sqrt(ddot3(b0, b1, b2, b0, b1, b2));
                    if (dist1 == 0 || dist2 == 0) v = EAO_TRI_ZERO_DIST;
                    else {
                        const float ratioDist = dist2 / dist1;
                        const float ratioOctave = K1.sf[o1] / K2.sf[o2];
                        if (ratioDist * A.ratioFactor < ratioOctave || ratioDist > ratioOctave * A.ratioFactor) v = EAO_TRI_SCALE;
                    }
                }
            }
        }
        verdict[idx1] = v;
        x3d[3 * (size_t)idx1] = X[0]; x3d[3 * (size_t)idx1 + 1] = X[1]; x3d[3 * (size_t)idx1 + 2] = X[2];
    }
}

using PinBuf = eao::PinBuf<hipHostMallocDefault>;   // staging of the asynchronous copies
struct Ctx : eao::ThreadStream {   // per host thread, grow-only
    PinBuf in, out;
    eao::DevBuf<unsigned char> din, dout;
};
thread_local Ctx g_tctx;
using eao::align256;

// nullptr: the view serves; else what is wrong with it
const char* view_problem(const eao_frame_view* V, const float* depth) {
    if (!V) return "no view";
    if (V->n < 0) return "negative keypoint count";
    if (V->n > 0 && !(V->kp_x && V->kp_y && V->kp_octave && V->u_right && depth)) return "kp_x, kp_y, kp_octave, u_right and the depth are read";
    if (!(V->scale_factors && V->level_sigma2 && V->nlevels > 0 && V->nlevels <= 64)) return "scale_factors and level_sigma2 of 1..64 levels are read";
    for (int i = 0; i < V->n; i++)
        if (V->kp_octave[i] < 0 || V->kp_octave[i] >= V->nlevels) return "a keypoint's octave lies outside the levels";
    return nullptr;
}

}  // namespace

namespace eao {
namespace tri {

void launch(hipStream_t s, const Side& K1, const eao_tri_camera& cam1, float ratioFactor, int nProb, const Prob* P, int* verdict, float* x3d) {
    if (nProb <= 0 || K1.n <= 0) return;
    TriArgs A;
    A.K1 = K1; A.cam1 = cam1; A.ratioFactor = ratioFactor; A.verdict = verdict; A.x3d = x3d;
    for (int q = 0; q < kMaxProb; q++) A.P[q] = P[q < nProb ? q : 0];
    hipLaunchKernelGGL(k_triangulate, dim3(eao::cdiv(K1.n, 4 * kSeg), nProb), dim3(256), 0, s, A);
}

}  // namespace tri
}  // namespace eao

extern "C" {

eao_status eao_triangulate_matches_batch(const eao_frame_view* K1, const eao_tri_camera* cam1, const float* depth1, const float* raw_x1, const float* raw_y1,
                                         int32_t n_nb, const eao_frame_view* const* K2s, const eao_tri_camera* cams2, const float* const* depth2s,
                                         const float* const* raw_x2s, const float* const* raw_y2s, const int32_t* match12, float ratio_factor,
                                         int32_t* verdict, float* x3d) {
    EAO_REQUIRE(K1 && cam1 && n_nb >= 0, "bad argument");
    if (n_nb == 0) return EAO_OK;
    EAO_REQUIRE(K2s && cams2 && depth2s && match12 && verdict && x3d, "null argument");
    const char* why = view_problem(K1, depth1);
    EAO_REQUIRE(!why, "keyframe 1: %s", why);
    const int n1 = K1->n;
    for (int k = 0; k < n_nb; k++) {
        why = view_problem(K2s[k], depth2s[k]);
        EAO_REQUIRE(!why, "neighbour %d: %s", k, why);
        const int32_t* row = match12 + (size_t)k * n1;
        for (int i = 0; i < n1; i++) EAO_REQUIRE(row[i] >= -1 && row[i] < K2s[k]->n, "neighbour %d: match12[%d] = %d is no keypoint of its %d", k, i, row[i], K2s[k]->n);
    }
    if (n1 == 0) return EAO_OK;
    Ctx& c = g_tctx;
    eao_status st = c.ready(eao::StreamClass::Background);      // LocalMapping waits for this call, Tracking does not
    if (st) return st;
    // one staging block: per keyframe [kx | ky | ur | depth | rawx | rawy | oct | sf | s2], then the table
    struct Off { size_t kx, ky, ur, dp, rx, ry, oc, sf, s2; };
    size_t off = 0;
    auto lay = [&](const eao_frame_view* V) {
        Off o;
        const size_t n = (size_t)std::max(V->n, 1), nl = (size_t)V->nlevels;
        o.kx = off; off = align256(off + 4 * n); o.ky = off; off = align256(off + 4 * n); o.ur = off; off = align256(off + 4 * n); o.dp = off; off = align256(off + 4 * n);
        o.rx = off; off = align256(off + 4 * n); o.ry = off; off = align256(off + 4 * n); o.oc = off; off = align256(off + 4 * n);
        o.sf = off; off = align256(off + 4 * nl); o.s2 = off; off = align256(off + 4 * nl);
        return o;
    };
    std::vector<Off> offs(n_nb + 1);
    offs[0] = lay(K1);
    for (int k = 0; k < n_nb; k++) offs[k + 1] = lay(K2s[k]);
    const size_t cells = (size_t)n_nb * n1, oTab = off, inBytes = align256(oTab + 4 * cells);
    const size_t oX = align256(4 * cells), outBytes = oX + 12 * cells;
    if ((st = c.in.reserve(inBytes)) || (st = c.out.reserve(outBytes)) || (st = c.din.reserve(inBytes)) || (st = c.dout.reserve(outBytes))) return st;
    auto fill = [&](const Off& o, const eao_frame_view* V, const float* depth, const float* rx, const float* ry) {
        const size_t b = 4 * (size_t)V->n, bl = 4 * (size_t)V->nlevels;
        unsigned char* h = c.in.p;
        if (b) {
            std::memcpy(h + o.kx, V->kp_x, b); std::memcpy(h + o.ky, V->kp_y, b); std::memcpy(h + o.ur, V->u_right, b); std::memcpy(h + o.dp, depth, b);
            std::memcpy(h + o.rx, rx ? rx : V->kp_x, b); std::memcpy(h + o.ry, ry ? ry : V->kp_y, b); std::memcpy(h + o.oc, V->kp_octave, b);
        }
        std::memcpy(h + o.sf, V->scale_factors, bl); std::memcpy(h + o.s2, V->level_sigma2, bl);
    };
    auto side = [&](const Off& o, const eao_frame_view* V) {
        const unsigned char* d = c.din.p;
        eao::tri::Side S;
        S.n = V->n; S.nlevels = V->nlevels;
        S.kx = (const float*)(d + o.kx); S.ky = (const float*)(d + o.ky); S.ur = (const float*)(d + o.ur); S.depth = (const float*)(d + o.dp);
        S.rawx = (const float*)(d + o.rx); S.rawy = (const float*)(d + o.ry); S.oct = (const int*)(d + o.oc); S.sf = (const float*)(d + o.sf); S.s2 = (const float*)(d + o.s2);
        return S;
    };
    fill(offs[0], K1, depth1, raw_x1, raw_y1);
    for (int k = 0; k < n_nb; k++) fill(offs[k + 1], K2s[k], depth2s[k], raw_x2s ? raw_x2s[k] : nullptr, raw_y2s ? raw_y2s[k] : nullptr);
    std::memcpy(c.in.p + oTab, match12, 4 * cells);
    eao::Drain drain(c.stream);
    EAO_HIP(hipMemcpyAsync(c.din.p, c.in.p, inBytes, hipMemcpyHostToDevice, c.stream));
    const eao::tri::Side S1 = side(offs[0], K1);
    for (int p0 = 0; p0 < n_nb; p0 += eao::tri::kMaxProb) {
        const int np = std::min(eao::tri::kMaxProb, n_nb - p0);
        eao::tri::Prob P[eao::tri::kMaxProb];
        for (int q = 0; q < np; q++) {
            P[q].K2 = side(offs[p0 + q + 1], K2s[p0 + q]);
            P[q].cam2 = cams2[p0 + q];
            P[q].match = (const int*)(c.din.p + oTab) + (size_t)(p0 + q) * n1;
        }
        eao::tri::launch(c.stream, S1, *cam1, ratio_factor, np, P, (int*)c.dout.p + (size_t)p0 * n1, (float*)(c.dout.p + oX) + (size_t)p0 * n1 * 3);
    }
    EAO_HIP(hipGetLastError());
    EAO_HIP(hipMemcpyAsync(c.out.p, c.dout.p, outBytes, hipMemcpyDeviceToHost, c.stream));
    EAO_HIP(drain.wait(eao::Drain::Block));
    std::memcpy(verdict, c.out.p, 4 * cells);
    std::memcpy(x3d, c.out.p + oX, 12 * cells);
    return EAO_OK;
}

}  // extern "C"
