// initializer_internal.h -- the device records of csrc/initializer.hip (one eao_initializer_initialize call)
#pragma once
#include "common.h"

namespace eao {
namespace init {

constexpr int kMaxMotions = 8;      // ReconstructH's eight solutions; ReconstructF uses the first four

struct Motion {      // one (R, t) of ReconstructF / ReconstructH and what CheckRT made of it
    float R[9], t[3];
    int n_good;
    float cosine;      // vCosParallax[min(50, nGood - 1)] after the sort; 1 when nGood == 0 (parallax = 0)
};

struct Out {
    int returned, branch, no_model, degenerate;
    int best_h, best_f, n_good, motion;
    int n_motions, n_inliers, pad0, pad1;
    float SH, SF, RH, cosine;
    float H21[9], F21[9], R21[9], t21[3];
    Motion mot[kMaxMotions];
};

struct Rec {
    int N, n1, iterations, inspect, min_triangulated;
    float T1[9], T2inv[9], T2t[9];
    float fx, fy, cx, cy;
    float sigma, th2;
    float cos_gt, cos_ge;            // parallax(c) > / >= minParallax  <=>  c <= cos_gt / cos_ge (made on the host from its own acos; -inf: never)
    const float4* raw;               // N (u1, v1, u2, v2), the undistorted keypoints of each pair
    const float4* nrm;               // N, the same through Normalize
    const int* first;                // N, mvMatches12[i].first
    const int* sets;                 // iterations * 8
    float* hypH21; float* hypH12; float* hypF21;      // iterations * 9 each
    float* score;                    // 2 * iterations: H then F
    unsigned char* hyp_flags;        // 2 * iterations * N, only with inspect
    unsigned char* inlier;           // N: flags of the winner of the branch taken
    unsigned* cos_key;               // kMaxMotions * N
    unsigned char* accepted;         // kMaxMotions * N
    unsigned char* good;             // kMaxMotions * n1
    float* p3d;                      // kMaxMotions * n1 * 3
    Out* out;
    float* out_p3d;                  // n1 * 3
    unsigned char* out_tri;          // n1
};

}  // namespace init
}  // namespace eao
