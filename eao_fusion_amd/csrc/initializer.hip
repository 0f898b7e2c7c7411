// initializer.hip -- Initializer (reference include/Initializer.h, src/Initializer.cc): the homography / fundamental RANSAC and the two-view reconstruction of
// Tracking::MonocularInitialization (src/Tracking.cc:1374-1392).
//
// One call is one Initializer::Initialize after its draws (src/Initializer.cc:99-121).  Upstream spreads FindHomography and FindFundamental over two host threads
// (:104-105); here the whole of it is five kernels on the calling thread's latency-class stream, one upload, one wait, one download:
//   k_init_hypotheses   grid (iterations, 2), one wavefront per model: ComputeH21 (:226-266) / ComputeF21 (:268-303).  A is built in float as written; its null vector
//                       is the eigenvector of the smallest eigenvalue of A^T A (double, S and V in LDS, fixed sweeps -- small_dense.h); then H21i = T2inv Hn T1 and
//                       H12i = H21i.inv() (:160-161), or the rank-2 projection through a 3 x 3 SVD and F21i = T2t Fn T1 (:212).
//   k_init_scores       grid (iterations, 2), one workgroup per model: CheckHomography (:305-388) / CheckFundamental (:390-468) over all N matches, read as 16-byte
//                       rows.  Only the score leaves (flags too when the caller inspects).
//   k_init_select       one workgroup: the first argmax of either model (:165, :216: strict >, from 0), RH and the branch (:112-118), the winner's flags recomputed,
//                       then DecomposeE (:909-929) or Faugeras' eight solutions (:584-686).
//   k_init_check_rt     one workgroup per motion hypothesis: CheckRT (:798-907) with Triangulate (:734-747) per inlier match, the sorted-cosine entry by selection.
//   k_init_finish       the final rule of ReconstructF (:499-569) or ReconstructH (:689-731) and the winner's vP3D / vbTriangulated rows.
//
// Arithmetic: the float expressions op for op (-ffp-contract=off); OpenCV's own arithmetic by the conventions of sim3_solver.hip / triangulate.hip (a small product
// accumulates in double and rounds once; a double scalar times a float matrix multiplies in double and rounds once; cv::norm, Mat::dot and cv::determinant are double;
// Mat::inv of a 3 x 3 is cofactors over a double determinant, zero when singular; a singular vector is a Jacobi eigenvector of A^T A rounded to float, its sign free).
// Deviations from upstream, all three stated in include/eao_fusion.h and DESIGN.md "Initializer":
//   1. a score is the sum of its terms in double, rounded once to float (every term is a float below 8 and a multiple of 2^-23, so that sum is exact and independent of
//      its order); upstream adds them one by one in float,
//   2. when the model of the branch taken has no hypothesis scoring above 0 the call returns false with no_model set; upstream multiplies an empty Mat and throws,
//   3. Normalize (:749-795) runs on the host inside the entry point, op for op and in upstream's summation order.
// Reproduced, not repaired: a singular H21i has the zero inverse, NaN chi-squares and a NaN score that never wins; a NaN chi-square fails `> th`, so it is added and
// leaves the flag set; a zero transfer denominator gives inf, which fails the gate.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "initializer_internal.h"
#include "small_dense.h"

using namespace eao;
using namespace eao::dense;
using eao::init::Motion;
using eao::init::Out;
using eao::init::Rec;
using eao::init::kMaxMotions;

namespace {

// ---- Initializer's literals (tests/golden/initializer_constants.json, read from the reference text by tools/reference_literals.py; held to it by
// tests/test_initializer_reference_cpu.py).  Nothing else in this file spells them.  (1.0 and 50 of :116 / :118 are the adapter's: include/eaofusion/Initializer.h.)
constexpr double kRatioH = 0.40;                // src/Initializer.cc:115  RH>0.40
constexpr float kChi2H = 5.991;                 // :333  const float th = 5.991;   :409  const float thScore = 5.991;
constexpr float kChi2F = 3.841;                 // :408  const float th = 3.841;
constexpr double kCosParallax = 0.99998;        // :857, :863, :892  cosParallax<0.99998
constexpr double kDegenerate = 1.00001;         // :597  d1/d2<1.00001 || d2/d3<1.00001
constexpr double kSimilar = 0.7;                // :507-513  nGood>0.7*maxGood
constexpr double kMinGoodFraction = 0.9;        // :504  0.9*N, :721  bestGood>0.9*N
constexpr double kSecondBest = 0.75;            // :721  secondBestGood<0.75*bestGood
constexpr double kReprojFactor = 4.0;           // :494-497, :703  4.0*mSigma2
constexpr int kParallaxRank = 50;               // :900  min(50,int(vCosParallax.size()-1))
// ----

constexpr int kThreads = 256;

__device__ __forceinline__ float recip(float x) { return (float)(1.0 / (double)x); }      // `1.0/x` assigned to a float

// one match of CheckHomography (:339-384); H: H21i, Hi: H12i
__device__ __forceinline__ bool check_h(const float* H, const float* Hi, const float4 m, float invSigmaSquare, double& score) {
    bool bIn = true;
    const float u1 = m.x, v1 = m.y, u2 = m.z, v2 = m.w;
    const float w2in1inv = recip(Hi[6] * u2 + Hi[7] * v2 + Hi[8]);
    const float u2in1 = (Hi[0] * u2 + Hi[1] * v2 + Hi[2]) * w2in1inv;
    const float v2in1 = (Hi[3] * u2 + Hi[4] * v2 + Hi[5]) * w2in1inv;
    const float squareDist1 = (u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1);
    const float chiSquare1 = squareDist1 * invSigmaSquare;
    if (chiSquare1 > kChi2H) bIn = false;
    else score += (double)(kChi2H - chiSquare1);
    const float w1in2inv = recip(H[6] * u1 + H[7] * v1 + H[8]);
    const float u1in2 = (H[0] * u1 + H[1] * v1 + H[2]) * w1in2inv;
    const float v1in2 = (H[3] * u1 + H[4] * v1 + H[5]) * w1in2inv;
    const float squareDist2 = (u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2);
    const float chiSquare2 = squareDist2 * invSigmaSquare;
    if (chiSquare2 > kChi2H) bIn = false;
    else score += (double)(kChi2H - chiSquare2);
    return bIn;
}

// one match of CheckFundamental (:415-464)
__device__ __forceinline__ bool check_f(const float* F, const float4 m, float invSigmaSquare, double& score) {
    bool bIn = true;
    const float u1 = m.x, v1 = m.y, u2 = m.z, v2 = m.w;
    const float a2 = F[0] * u1 + F[1] * v1 + F[2];
    const float b2 = F[3] * u1 + F[4] * v1 + F[5];
    const float c2 = F[6] * u1 + F[7] * v1 + F[8];
    const float num2 = a2 * u2 + b2 * v2 + c2;
    const float squareDist1 = num2 * num2 / (a2 * a2 + b2 * b2);
    const float chiSquare1 = squareDist1 * invSigmaSquare;
    if (chiSquare1 > kChi2F) bIn = false;
    else score += (double)(kChi2H - chiSquare1);
    const float a1 = F[0] * u2 + F[3] * v2 + F[6];
    const float b1 = F[1] * u2 + F[4] * v2 + F[7];
    const float c1 = F[2] * u2 + F[5] * v2 + F[8];
    const float num1 = a1 * u1 + b1 * v1 + c1;
    const float squareDist2 = num1 * num1 / (a1 * a1 + b1 * b1);
    const float chiSquare2 = squareDist2 * invSigmaSquare;
    if (chiSquare2 > kChi2F) bIn = false;
    else score += (double)(kChi2H - chiSquare2);
    return bIn;
}

__device__ __forceinline__ float inv_sigma_square(float sigma) { return recip(sigma * sigma); }      // :335, :411  1.0/(sigma*sigma)

// sums over a workgroup of kThreads; sh: 4 slots.  Every thread gets the total.
__device__ __forceinline__ double block_sum(double v, double* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return sh[0] + sh[1] + sh[2] + sh[3];
}
__device__ __forceinline__ int block_sum(int v, int* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return sh[0] + sh[1] + sh[2] + sh[3];
}

// ---------------------------------------------------------------------- hypotheses
__global__ __launch_bounds__(64) void k_init_hypotheses(const Rec* __restrict__ Wp) {
    const Rec& P = *Wp;
    __shared__ float sA[16 * 9];
    __shared__ double sS[81], sV[81];
    const int h = blockIdx.x, model = blockIdx.y, lane = threadIdx.x;
    const int rows = model == 0 ? 16 : 8;
    if (lane < rows) {
        const int j = model == 0 ? lane >> 1 : lane;
        int idx = P.sets[8 * h + j];
        idx = idx < 0 ? 0 : (idx >= P.N ? P.N - 1 : idx);      // validated on the host; clamped all the same
        const float4 m = P.nrm[idx];
        const float u1 = m.x, v1 = m.y, u2 = m.z, v2 = m.w;
        float* r = sA + 9 * lane;
        if (model == 1) {                 // :281-289
            r[0] = u2 * u1; r[1] = u2 * v1; r[2] = u2; r[3] = v2 * u1; r[4] = v2 * v1; r[5] = v2; r[6] = u1; r[7] = v1; r[8] = 1;
        } else if ((lane & 1) == 0) {     // :239-247
            r[0] = 0; r[1] = 0; r[2] = 0; r[3] = -u1; r[4] = -v1; r[5] = -1; r[6] = v2 * u1; r[7] = v2 * v1; r[8] = v2;
        } else {                          // :249-257
            r[0] = u1; r[1] = v1; r[2] = 1; r[3] = 0; r[4] = 0; r[5] = 0; r[6] = -u2 * u1; r[7] = -u2 * v1; r[8] = -u2;
        }
    }
    wave_sync();
    float hv[9];
    null_vector9(sA, rows, sS, sV, lane, hv);
    float T[9], M[9];
    if (model == 0) {
        float Hi[9];
        mul3(P.T2inv, hv, T);
        mul3(T, P.T1, M);                 // H21i = T2inv*Hn*T1
        inv3(M, Hi);                      // H12i = H21i.inv()
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < 9; k++) { P.hypH21[9 * h + k] = M[k]; P.hypH12[9 * h + k] = Hi[k]; }
        }
    } else {
        float U[9], w[3], Vt[9], UD[9], Fn[9];
        svd3(hv, U, w, Vt);
        w[2] = 0;                         // :300
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int k = 0; k < 3; k++) UD[3 * i + k] = (float)((double)U[3 * i + k] * (double)w[k]);      // u*diag(w)
        mul3(UD, Vt, Fn);
        mul3(P.T2t, Fn, T);
        mul3(T, P.T1, M);                 // F21i = T2t*Fn*T1
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < 9; k++) P.hypF21[9 * h + k] = M[k];
        }
    }
}

// ---------------------------------------------------------------------- scores
__global__ __launch_bounds__(kThreads) void k_init_scores(const Rec* __restrict__ Wp) {
    const Rec& P = *Wp;
    __shared__ double sh[4];
    const int h = blockIdx.x, model = blockIdx.y, N = P.N;
    const float invS2 = inv_sigma_square(P.sigma);
    unsigned char* flags = P.inspect ? P.hyp_flags + ((size_t)model * P.iterations + h) * N : nullptr;
    double score = 0;
    float A[9], B[9];
    if (model == 0) {
#pragma unroll
        for (int k = 0; k < 9; k++) { A[k] = P.hypH21[9 * h + k]; B[k] = P.hypH12[9 * h + k]; }
        for (int i = threadIdx.x; i < N; i += kThreads) {
            const bool in = check_h(A, B, P.raw[i], invS2, score);
            if (flags) flags[i] = in ? 1 : 0;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 9; k++) A[k] = P.hypF21[9 * h + k];
        for (int i = threadIdx.x; i < N; i += kThreads) {
            const bool in = check_f(A, P.raw[i], invS2, score);
            if (flags) flags[i] = in ? 1 : 0;
        }
    }
    const double total = block_sum(score, sh);
    if (threadIdx.x == 0) P.score[model * P.iterations + h] = (float)total;
}

// ---------------------------------------------------------------------- the motion hypotheses (one lane)
__device__ inline void store_motion(Motion& M, const float* R, const float* t) {
#pragma unroll
    for (int k = 0; k < 9; k++) M.R[k] = R[k];
#pragma unroll
    for (int k = 0; k < 3; k++) M.t[k] = t[k];
    M.n_good = 0;
    M.cosine = 1.f;
}

// ReconstructF's head (:479-487): E21 = K.t()*F21*K, DecomposeE (:909-929); the order of :494-497 is (R1,t1) (R2,t1) (R1,t2) (R2,t2)
__device__ inline void motions_f(const Rec& P, const float* F21, Out& O) {
    const float K[9] = {P.fx, 0, P.cx, 0, P.fy, P.cy, 0, 0, 1};
    float Kt[9], T[9], E[9], U[9], w[3], Vt[9];
    transpose3(K, Kt);
    mul3(Kt, F21, T);
    mul3(T, K, E);
    svd3(E, U, w, Vt);
    float t[3] = {U[2], U[5], U[8]};                                  // u.col(2)
    const double nt = sqrt((double)t[0] * (double)t[0] + (double)t[1] * (double)t[1] + (double)t[2] * (double)t[2]);
    const double it = 1.0 / nt;
#pragma unroll
    for (int k = 0; k < 3; k++) t[k] = (float)((double)t[k] * it);    // t/cv::norm(t)
    const float W[9] = {0, -1, 0, 1, 0, 0, 0, 0, 1};
    float Wt[9], R1[9], R2[9], t2[3];
    transpose3(W, Wt);
    mul3(U, W, T);
    mul3(T, Vt, R1);
    if (det3(R1) < 0) {
#pragma unroll
        for (int k = 0; k < 9; k++) R1[k] = -R1[k];
    }
    mul3(U, Wt, T);
    mul3(T, Vt, R2);
    if (det3(R2) < 0) {
#pragma unroll
        for (int k = 0; k < 9; k++) R2[k] = -R2[k];
    }
#pragma unroll
    for (int k = 0; k < 3; k++) t2[k] = -t[k];
    store_motion(O.mot[0], R1, t);
    store_motion(O.mot[1], R2, t);
    store_motion(O.mot[2], R1, t2);
    store_motion(O.mot[3], R2, t2);
    O.n_motions = 4;
}

// ReconstructH's head (:584-686).  false: the d1/d2, d2/d3 return of :597
__device__ inline bool motions_h(const Rec& P, const float* H21, Out& O) {
    const float K[9] = {P.fx, 0, P.cx, 0, P.fy, P.cy, 0, 0, 1};
    float invK[9], T[9], A[9], U[9], w[3], Vt[9];
    inv3(K, invK);
    mul3(invK, H21, T);
    mul3(T, K, A);
    svd3(A, U, w, Vt);
    const float s = (float)(det3(U) * det3(Vt));
    const float d1 = w[0], d2 = w[1], d3 = w[2];
    if ((double)(d1 / d2) < kDegenerate || (double)(d2 / d3) < kDegenerate) return false;
    const float aux1 = sqrtf((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3));
    const float aux3 = sqrtf((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3));
    const float x1[4] = {aux1, aux1, -aux1, -aux1};
    const float x3[4] = {aux3, -aux3, aux3, -aux3};
    const float aux_stheta = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2);
    const float ctheta = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2);
    const float stheta[4] = {aux_stheta, -aux_stheta, -aux_stheta, aux_stheta};
    const float aux_sphi = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2);
    const float cphi = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2);
    const float sphi[4] = {aux_sphi, -aux_sphi, -aux_sphi, aux_sphi};
#pragma unroll
    for (int half = 0; half < 2; half++)
#pragma unroll
        for (int i = 0; i < 4; i++) {
            float Rp[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
            float tp[3];
            float scale;
            if (half == 0) {      // case d' = d2 (:619-648)
                Rp[0] = ctheta; Rp[2] = -stheta[i]; Rp[6] = stheta[i]; Rp[8] = ctheta;
                tp[0] = x1[i]; tp[1] = 0; tp[2] = -x3[i];
                scale = d1 - d3;
            } else {              // case d' = -d2 (:656-686)
                Rp[0] = cphi; Rp[2] = sphi[i]; Rp[4] = -1; Rp[6] = sphi[i]; Rp[8] = -cphi;
                tp[0] = x1[i]; tp[1] = 0; tp[2] = x3[i];
                scale = d1 + d3;
            }
            float URp[9], R[9], t[3];
#pragma unroll
            for (int r = 0; r < 3; r++)
#pragma unroll
                for (int c = 0; c < 3; c++)      // s*U*Rp: the scalar folds into the product
                    URp[3 * r + c] = (float)((double)s * ((double)U[3 * r] * (double)Rp[c] + (double)U[3 * r + 1] * (double)Rp[3 + c] + (double)U[3 * r + 2] * (double)Rp[6 + c]));
            mul3(URp, Vt, R);
#pragma unroll
            for (int k = 0; k < 3; k++) tp[k] = (float)((double)tp[k] * (double)scale);      // tp*=d1-d3
#pragma unroll
            for (int r = 0; r < 3; r++) t[r] = gemm3(U[3 * r], U[3 * r + 1], U[3 * r + 2], tp[0], tp[1], tp[2]);
            const double it = 1.0 / sqrt((double)t[0] * (double)t[0] + (double)t[1] * (double)t[1] + (double)t[2] * (double)t[2]);
#pragma unroll
            for (int k = 0; k < 3; k++) t[k] = (float)((double)t[k] * it);                  // t/cv::norm(t)
            store_motion(O.mot[4 * half + i], R, t);
        }
    O.n_motions = 8;
    return true;
}

// ---------------------------------------------------------------------- selection
__global__ __launch_bounds__(kThreads) void k_init_select(const Rec* __restrict__ Wp) {
    const Rec& P = *Wp;
    Out& O = *P.out;
    __shared__ float sBest[2][kThreads];
    __shared__ int sIdx[2][kThreads];
    __shared__ int sInfo[2];
    __shared__ int sCnt[4];
    const int tid = threadIdx.x, it = P.iterations;
#pragma unroll
    for (int model = 0; model < 2; model++) {
        float best = 0.f;
        int idx = -1;
        for (int h = tid; h < it; h += kThreads) {
            const float s = P.score[model * it + h];
            if (s > best) { best = s; idx = h; }      // currentScore>score: a NaN never wins, the first of equal scores stays
        }
        sBest[model][tid] = best;
        sIdx[model][tid] = idx;
    }
    __syncthreads();
    if (tid == 0) {
        float S[2];
        int I[2];
        for (int model = 0; model < 2; model++) {
            float best = 0.f;
            int idx = -1;
            for (int t = 0; t < kThreads; t++) {
                const float s = sBest[model][t];
                const int i = sIdx[model][t];
                if (i >= 0 && (s > best || (s == best && idx >= 0 && i < idx))) { best = s; idx = i; }
            }
            S[model] = best;
            I[model] = idx;
        }
        const float RH = S[0] / (S[0] + S[1]);
        const int branch = ((double)RH > kRatioH) ? EAO_INIT_BRANCH_H : EAO_INIT_BRANCH_F;
        const int win = branch == EAO_INIT_BRANCH_H ? I[0] : I[1];
        O.returned = 0; O.branch = branch; O.no_model = win < 0 ? 1 : 0; O.degenerate = 0;
        O.best_h = I[0]; O.best_f = I[1]; O.n_good = 0; O.motion = -1;
        O.n_motions = 0; O.n_inliers = 0; O.pad0 = 0; O.pad1 = 0;
        O.SH = S[0]; O.SF = S[1]; O.RH = RH; O.cosine = 1.f;
        for (int k = 0; k < 9; k++) {
            O.H21[k] = I[0] >= 0 ? P.hypH21[9 * I[0] + k] : 0.f;
            O.F21[k] = I[1] >= 0 ? P.hypF21[9 * I[1] + k] : 0.f;
            O.R21[k] = 0.f;
        }
        for (int k = 0; k < 3; k++) O.t21[k] = 0.f;
        sInfo[0] = branch;
        sInfo[1] = win;
    }
    __syncthreads();
    const int branch = sInfo[0], win = sInfo[1];
    if (win < 0) return;
    // the winner's flags again (nothing of the other 2 * iterations - 1 rows was kept)
    const float invS2 = inv_sigma_square(P.sigma);
    float A[9], B[9];
    int cnt = 0;
    double unused = 0;
    if (branch == EAO_INIT_BRANCH_H) {
#pragma unroll
        for (int k = 0; k < 9; k++) { A[k] = P.hypH21[9 * win + k]; B[k] = P.hypH12[9 * win + k]; }
        for (int i = tid; i < P.N; i += kThreads) {
            const bool in = check_h(A, B, P.raw[i], invS2, unused);
            P.inlier[i] = in ? 1 : 0;
            cnt += in ? 1 : 0;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 9; k++) A[k] = P.hypF21[9 * win + k];
        for (int i = tid; i < P.N; i += kThreads) {
            const bool in = check_f(A, P.raw[i], invS2, unused);
            P.inlier[i] = in ? 1 : 0;
            cnt += in ? 1 : 0;
        }
    }
    const int n_inl = block_sum(cnt, sCnt);
    if (tid == 0) {
        O.n_inliers = n_inl;
        if (branch == EAO_INIT_BRANCH_H) {
            if (!motions_h(P, A, O)) O.degenerate = 1;
        } else {
            motions_f(P, A, O);
        }
    }
}

// ---------------------------------------------------------------------- CheckRT
__global__ __launch_bounds__(kThreads) void k_init_check_rt(const Rec* __restrict__ Wp) {
    const Rec& P = *Wp;
    Out& O = *P.out;
    const int mi = blockIdx.x, tid = threadIdx.x, N = P.N, n1 = P.n1;
    if (mi >= O.n_motions) return;      // (uniform over the workgroup) the branch not taken, the :597 return, no model
    __shared__ int hist[256];
    __shared__ int slot[2];
    __shared__ int sCnt[4];
    float R[9], t[3];
#pragma unroll
    for (int k = 0; k < 9; k++) R[k] = O.mot[mi].R[k];
#pragma unroll
    for (int k = 0; k < 3; k++) t[k] = O.mot[mi].t[k];
    unsigned char* good = P.good + (size_t)mi * n1;
    float* p3d = P.p3d + (size_t)mi * n1 * 3;
    unsigned char* accepted = P.accepted + (size_t)mi * N;
    unsigned* cos_key = P.cos_key + (size_t)mi * N;
    for (int i = tid; i < n1; i += kThreads) { good[i] = 0; p3d[3 * i] = 0.f; p3d[3 * i + 1] = 0.f; p3d[3 * i + 2] = 0.f; }      // :808-809
    __syncthreads();
    const float fx = P.fx, fy = P.fy, cx = P.cx, cy = P.cy;
    // P1 = K[I|0] (:815-816), P2 = K*[R|t] (:821-824), O2 = -R.t()*t (:826)
    const float P1[3][4] = {{fx, 0, cx, 0}, {0, fy, cy, 0}, {0, 0, 1, 0}};
    const float K[3][3] = {{fx, 0, cx}, {0, fy, cy}, {0, 0, 1}};
    float P2[3][4], O2[3];
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) P2[r][c] = gemm3(K[r][0], K[r][1], K[r][2], R[c], R[3 + c], R[6 + c]);
        P2[r][3] = gemm3(K[r][0], K[r][1], K[r][2], t[0], t[1], t[2]);
    }
#pragma unroll
    for (int i = 0; i < 3; i++) O2[i] = -gemm3(R[i], R[3 + i], R[6 + i], t[0], t[1], t[2]);
    int nGood = 0;
    for (int i = tid; i < N; i += kThreads) {
        unsigned char acc = 0;
        unsigned key = 0;
        if (P.inlier[i]) {
            const float4 m = P.raw[i];
            int f = P.first[i];
            f = f < 0 ? 0 : (f >= n1 ? n1 - 1 : f);      // validated on the host; clamped all the same
            // Triangulate (:734-747)
            float Am[4][4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                Am[0][k] = m.x * P1[2][k] - P1[0][k];
                Am[1][k] = m.y * P1[2][k] - P1[1][k];
                Am[2][k] = m.z * P2[2][k] - P2[0][k];
                Am[3][k] = m.w * P2[2][k] - P2[1][k];
            }
            double S[4][4], ev[4];
#pragma unroll
            for (int a = 0; a < 4; a++)
#pragma unroll
                for (int k = a; k < 4; k++) {
                    double s = (double)Am[0][a] * (double)Am[0][k];
                    s += (double)Am[1][a] * (double)Am[1][k];
                    s += (double)Am[2][a] * (double)Am[2][k];
                    s += (double)Am[3][a] * (double)Am[3][k];
                    S[a][k] = s; S[k][a] = s;
                }
            smallest_eigenvector(S, ev);
            const double iw = 1. / (double)(float)ev[3];
            const float X[3] = {(float)((double)(float)ev[0] * iw), (float)((double)(float)ev[1] * iw), (float)((double)(float)ev[2] * iw)};
            if (isfinite(X[0]) && isfinite(X[1]) && isfinite(X[2])) {      // (:841-845: vbGood[first] = false is what it already holds)
                // :848-854
                const float dist1 = (float)sqrt((double)X[0] * (double)X[0] + (double)X[1] * (double)X[1] + (double)X[2] * (double)X[2]);
                const float n2[3] = {X[0] - O2[0], X[1] - O2[1], X[2] - O2[2]};
                const float dist2 = (float)sqrt((double)n2[0] * (double)n2[0] + (double)n2[1] * (double)n2[1] + (double)n2[2] * (double)n2[2]);
                const double dot = (double)X[0] * (double)n2[0] + (double)X[1] * (double)n2[1] + (double)X[2] * (double)n2[2];
                const float cosParallax = (float)(dot / (double)(dist1 * dist2));
                const bool par = (double)cosParallax < kCosParallax;
                bool ok = !(X[2] <= 0 && par);                                  // :857
                float C2[3];
#pragma unroll
                for (int r = 0; r < 3; r++) C2[r] = gemm3(R[3 * r], R[3 * r + 1], R[3 * r + 2], X[0], X[1], X[2]) + t[r];      // R*p3dC1+t
                ok = ok && !(C2[2] <= 0 && par);                                // :863
                const float invZ1 = recip(X[2]);
                const float im1x = fx * X[0] * invZ1 + cx, im1y = fy * X[1] * invZ1 + cy;
                const float squareError1 = (im1x - m.x) * (im1x - m.x) + (im1y - m.y) * (im1y - m.y);
                ok = ok && !(squareError1 > P.th2);                             // :874
                const float invZ2 = recip(C2[2]);
                const float im2x = fx * C2[0] * invZ2 + cx, im2y = fy * C2[1] * invZ2 + cy;
                const float squareError2 = (im2x - m.z) * (im2x - m.z) + (im2y - m.w) * (im2y - m.w);
                ok = ok && !(squareError2 > P.th2);                             // :885
                if (ok) {
                    acc = 1;
                    key = ordered_key(cosParallax);
                    p3d[3 * f] = X[0]; p3d[3 * f + 1] = X[1]; p3d[3 * f + 2] = X[2];
                    nGood++;
                    if (par) good[f] = 1;
                }
            }
        }
        accepted[i] = acc;
        cos_key[i] = key;
    }
    nGood = block_sum(nGood, sCnt);      // (its barriers also order the rows above before the selection reads them)
    float cosine = 1.f;                  // nGood == 0: parallax = 0 (:904)
    if (nGood > 0) {
        const int rank = kParallaxRank < nGood - 1 ? kParallaxRank : nGood - 1;
        cosine = key_value(kth_smallest(cos_key, accepted, N, rank, hist, slot));
    }
    if (tid == 0) { O.mot[mi].n_good = nGood; O.mot[mi].cosine = cosine; }
}

// ---------------------------------------------------------------------- the final rule
__global__ __launch_bounds__(kThreads) void k_init_finish(const Rec* __restrict__ Wp) {
    const Rec& P = *Wp;
    Out& O = *P.out;
    __shared__ int sRet[2];
    const int tid = threadIdx.x, n1 = P.n1;
    if (tid == 0) {
        int best = -1, ret = 0;
        const int N = O.n_inliers;
        if (O.n_motions == 4) {            // ReconstructF :499-569
            int maxGood = 0;
            for (int i = 0; i < 4; i++) maxGood = O.mot[i].n_good > maxGood ? O.mot[i].n_good : maxGood;
            const int frac = (int)(kMinGoodFraction * N);
            const int nMinGood = frac > P.min_triangulated ? frac : P.min_triangulated;
            int nsimilar = 0;
            for (int i = 0; i < 4; i++)
                if ((double)O.mot[i].n_good > kSimilar * maxGood) nsimilar++;
            for (int i = 3; i >= 0; i--)
                if (O.mot[i].n_good == maxGood) best = i;      // the if / else-if chain of :523-567 takes the first
            if (!(maxGood < nMinGood || nsimilar > 1)) {
                const float c = O.mot[best].cosine;
                ret = (c >= -1.f && c <= P.cos_gt) ? 1 : 0;    // parallax>minParallax
            }
        } else if (O.n_motions == 8) {     // ReconstructH :689-731
            int bestGood = 0, secondBestGood = 0;
            for (int i = 0; i < 8; i++) {
                const int g = O.mot[i].n_good;
                if (g > bestGood) { secondBestGood = bestGood; bestGood = g; best = i; }
                else if (g > secondBestGood) secondBestGood = g;
            }
            if (best >= 0) {
                const float c = O.mot[best].cosine;
                const bool par = c >= -1.f && c <= P.cos_ge;   // bestParallax>=minParallax
                ret = ((double)secondBestGood < kSecondBest * bestGood && par && bestGood > P.min_triangulated && (double)bestGood > kMinGoodFraction * N) ? 1 : 0;
            }
        }
        O.motion = best;
        O.returned = ret;
        if (best >= 0) { O.n_good = O.mot[best].n_good; O.cosine = O.mot[best].cosine; }
        if (ret) {
            for (int k = 0; k < 9; k++) O.R21[k] = O.mot[best].R[k];
            for (int k = 0; k < 3; k++) O.t21[k] = O.mot[best].t[k];
        }
        sRet[0] = ret;
        sRet[1] = best;
    }
    __syncthreads();
    const int ret = sRet[0], best = sRet[1];
    const unsigned char* good = P.good + (size_t)(best < 0 ? 0 : best) * n1;
    const float* p3d = P.p3d + (size_t)(best < 0 ? 0 : best) * n1 * 3;
    for (int i = tid; i < n1; i += kThreads) P.out_tri[i] = ret ? good[i] : 0;
    for (int i = tid; i < 3 * n1; i += kThreads) P.out_p3d[i] = ret ? p3d[i] : 0.f;
}

// ---------------------------------------------------------------------- host side
constexpr int kKernels = 5;
struct InitCtx : ThreadStream {
    DevBuf<unsigned char> dev;
    std::vector<unsigned char> host;
    KernelClock<kKernels> clock;      // EAO_INIT_EVENTS=1 (tools/bench_initializer.py)
};
thread_local InitCtx g_init;

// Initializer::Normalize (:749-795) over ALL keypoints of a frame, op for op; T row-major
void normalize(const float* xy, int n, std::vector<float>& out, float T[9]) {
    float meanX = 0, meanY = 0;
    for (int i = 0; i < n; i++) { meanX += xy[2 * i]; meanY += xy[2 * i + 1]; }
    meanX = meanX / n;
    meanY = meanY / n;
    float meanDevX = 0, meanDevY = 0;
    out.resize((size_t)2 * n);
    for (int i = 0; i < n; i++) {
        out[2 * i] = xy[2 * i] - meanX;
        out[2 * i + 1] = xy[2 * i + 1] - meanY;
        meanDevX += std::fabs(out[2 * i]);
        meanDevY += std::fabs(out[2 * i + 1]);
    }
    meanDevX = meanDevX / n;
    meanDevY = meanDevY / n;
    const float sX = (float)(1.0 / (double)meanDevX);
    const float sY = (float)(1.0 / (double)meanDevY);
    for (int i = 0; i < n; i++) { out[2 * i] = out[2 * i] * sX; out[2 * i + 1] = out[2 * i + 1] * sY; }
    for (int k = 0; k < 9; k++) T[k] = (k == 0 || k == 4 || k == 8) ? 1.f : 0.f;
    T[0] = sX; T[4] = sY; T[2] = -meanX * sX; T[5] = -meanY * sY;
}

// parallax = acos(cos)*180/CV_PI (:901), the arc cosine in double
float parallax_of(float c) { return (float)(std::acos((double)c) * 180 / 3.1415926535897932384626433832795); }

// The largest float c in [-1, 1] for which pred(parallax_of(c)) holds; pred holds on an interval that starts at -1 (the parallax falls as c grows).  -inf when it
// holds nowhere.  The kernels compare cosines against it, so the library has one arc cosine: the host's.
template <class Pred> float cosine_bound(Pred pred) {
    auto key = [](float f) { uint32_t u; std::memcpy(&u, &f, 4); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); };
    auto val = [](uint32_t k) { const uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k; float f; std::memcpy(&f, &u, 4); return f; };
    if (!pred(parallax_of(-1.f))) return -INFINITY;
    if (pred(parallax_of(1.f))) return 1.f;
    uint32_t lo = key(-1.f), hi = key(1.f);
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (pred(parallax_of(val(mid)))) lo = mid; else hi = mid;
    }
    return val(lo);
}

eao_status check_problem(const eao_initializer_problem* p, const int32_t* sets, int iterations, const eao_initializer_result* r) {
    EAO_REQUIRE(p && r, "null argument");
    EAO_REQUIRE(p->n_matches >= 8, "bad problem: %d matches, ComputeH21 / ComputeF21 draw eight", p->n_matches);
    EAO_REQUIRE(p->n1 >= 1 && p->n2 >= 1 && p->keys1_xy && p->keys2_xy && p->matches12, "bad problem: keypoints or matches missing");
    EAO_REQUIRE(iterations >= 1 && iterations <= 65535 && sets, "bad call: %d iterations (1 .. 65535)", iterations);
    EAO_REQUIRE(r->p3d && r->triangulated, "bad call: result->p3d and result->triangulated are written");
    EAO_REQUIRE(std::isfinite(p->fx) && std::isfinite(p->fy) && std::isfinite(p->cx) && std::isfinite(p->cy), "bad problem: non-finite intrinsic");
    EAO_REQUIRE(std::isfinite(p->sigma) && p->sigma > 0 && std::isfinite(p->min_parallax) && p->min_triangulated >= 0, "bad problem: sigma, min_parallax or min_triangulated");
    for (size_t i = 0; i < (size_t)2 * p->n1; i++) EAO_REQUIRE(std::isfinite(p->keys1_xy[i]), "bad problem: keypoint %zu of frame 1 is not finite", i / 2);
    for (size_t i = 0; i < (size_t)2 * p->n2; i++) EAO_REQUIRE(std::isfinite(p->keys2_xy[i]), "bad problem: keypoint %zu of frame 2 is not finite", i / 2);
    int prev = -1;
    for (int i = 0; i < p->n_matches; i++) {
        const int a = p->matches12[2 * i], b = p->matches12[2 * i + 1];
        EAO_REQUIRE(a >= 0 && a < p->n1 && b >= 0 && b < p->n2, "bad problem: match %d = (%d, %d) of %d x %d keypoints", i, a, b, p->n1, p->n2);
        EAO_REQUIRE(a > prev, "bad problem: match %d: `first` does not ascend (%d after %d)", i, a, prev);
        prev = a;
    }
    for (size_t k = 0; k < (size_t)iterations * 8; k++)
        EAO_REQUIRE(sets[k] >= 0 && sets[k] < p->n_matches, "bad call: set index %d at %zu, %d matches", sets[k], k, p->n_matches);
    return EAO_OK;
}

}  // namespace

extern "C" {

eao_status eao_initializer_initialize(const eao_initializer_problem* problem, const int32_t* sets, int32_t iterations, eao_initializer_result* result) {
    eao_status st = check_problem(problem, sets, iterations, result);
    if (st) return st;
    const eao_initializer_problem& p = *problem;
    eao_initializer_result& r = *result;
    InitCtx& ctx = g_init;
    if ((st = ctx.ready(StreamClass::Latency))) return st;      // Tracking waits for the call
    const size_t N = (size_t)p.n_matches, n1 = (size_t)p.n1, it = (size_t)iterations;
    const bool inspect = r.hyp_H21 || r.hyp_H12 || r.hyp_F21 || r.hyp_SH || r.hyp_SF || r.hyp_inlier_H || r.hyp_inlier_F || r.inlier || r.mot_R || r.mot_t ||
                         r.mot_n_good || r.mot_cos || r.mot_good || r.mot_p3d;
    const bool flags = r.hyp_inlier_H || r.hyp_inlier_F;
    // layout: [Rec | raw | nrm | first | sets] up | [Out | out_p3d | out_tri] down | [hyp matrices | scores | inlier | good | p3d | flags] down with inspect | scratch
    size_t off = align256(sizeof(Rec));
    const size_t oRaw = off; off = align256(off + 16 * N);
    const size_t oNrm = off; off = align256(off + 16 * N);
    const size_t oFirst = off; off = align256(off + 4 * N);
    const size_t oSets = off; off = align256(off + 32 * it);
    const size_t inEnd = off, oOut = off;
    off = align256(off + sizeof(Out));
    const size_t oP3d = off; off = align256(off + 12 * n1);
    const size_t oTri = off; off = align256(off + n1);
    const size_t outEnd = off, oH21 = off;
    off = align256(off + 36 * it);
    const size_t oH12 = off; off = align256(off + 36 * it);
    const size_t oF21 = off; off = align256(off + 36 * it);
    const size_t oScore = off; off = align256(off + 8 * it);
    const size_t oInl = off; off = align256(off + N);
    const size_t oGood = off; off = align256(off + kMaxMotions * n1);
    const size_t oMP3d = off; off = align256(off + kMaxMotions * 12 * n1);
    const size_t oFlags = off; off = align256(off + (flags ? 2 * it * N : 0));
    const size_t inspEnd = off, oKey = off;
    off = align256(off + kMaxMotions * 4 * N);
    const size_t oAcc = off; off = align256(off + kMaxMotions * N);
    const size_t total = off;
    if ((st = ctx.dev.reserve(total))) return st;
    if (ctx.host.size() < total) ctx.host.resize(total);
    unsigned char* h = ctx.host.data();
    unsigned char* d = ctx.dev.p;
    // host prologue: Normalize of both frames (:132-133 and again :183-184, the same values), the pairs raw and normalised
    std::vector<float> vPn1, vPn2;
    float T1[9], T2[9];
    normalize(p.keys1_xy, p.n1, vPn1, T1);
    normalize(p.keys2_xy, p.n2, vPn2, T2);
    Rec& W = *(Rec*)h;
    std::memset(&W, 0, sizeof(W));
    W.N = p.n_matches; W.n1 = p.n1; W.iterations = iterations; W.inspect = flags ? 1 : 0; W.min_triangulated = p.min_triangulated;
    std::memcpy(W.T1, T1, sizeof(T1));
    inv3(T2, W.T2inv);           // :134
    transpose3(T2, W.T2t);       // :185
    W.fx = p.fx; W.fy = p.fy; W.cx = p.cx; W.cy = p.cy;
    W.sigma = p.sigma;
    const float sigma2 = p.sigma * p.sigma;      // mSigma2 (:40)
    W.th2 = (float)(kReprojFactor * (double)sigma2);
    const float minParallax = p.min_parallax;
    W.cos_gt = cosine_bound([minParallax](float par) { return par > minParallax; });
    W.cos_ge = cosine_bound([minParallax](float par) { return par >= minParallax; });
    float* raw = (float*)(h + oRaw);
    float* nrm = (float*)(h + oNrm);
    int* first = (int*)(h + oFirst);
    for (size_t i = 0; i < N; i++) {
        const int a = p.matches12[2 * i], b = p.matches12[2 * i + 1];
        raw[4 * i] = p.keys1_xy[2 * a]; raw[4 * i + 1] = p.keys1_xy[2 * a + 1]; raw[4 * i + 2] = p.keys2_xy[2 * b]; raw[4 * i + 3] = p.keys2_xy[2 * b + 1];
        nrm[4 * i] = vPn1[2 * a]; nrm[4 * i + 1] = vPn1[2 * a + 1]; nrm[4 * i + 2] = vPn2[2 * b]; nrm[4 * i + 3] = vPn2[2 * b + 1];
        first[i] = a;
    }
    std::memcpy(h + oSets, sets, 32 * it);
    W.raw = (const float4*)(d + oRaw); W.nrm = (const float4*)(d + oNrm); W.first = (const int*)(d + oFirst); W.sets = (const int*)(d + oSets);
    W.hypH21 = (float*)(d + oH21); W.hypH12 = (float*)(d + oH12); W.hypF21 = (float*)(d + oF21); W.score = (float*)(d + oScore);
    W.hyp_flags = d + oFlags; W.inlier = d + oInl; W.cos_key = (unsigned*)(d + oKey); W.accepted = d + oAcc; W.good = d + oGood; W.p3d = (float*)(d + oMP3d);
    W.out = (Out*)(d + oOut); W.out_p3d = (float*)(d + oP3d); W.out_tri = d + oTri;
    const Rec* dW = (const Rec*)d;
    static const bool envEvents = getenv("EAO_INIT_EVENTS") && atoi(getenv("EAO_INIT_EVENTS"));
    if (envEvents != ctx.clock.armed()) ctx.clock.arm(envEvents);
    Drain drain(ctx.stream);
    EAO_HIP(hipMemcpyAsync(d, h, inEnd, hipMemcpyHostToDevice, ctx.stream));
    ctx.clock.mark(0, ctx.stream);
    hipLaunchKernelGGL(k_init_hypotheses, dim3(iterations, 2), dim3(64), 0, ctx.stream, dW);
    ctx.clock.mark(1, ctx.stream);
    hipLaunchKernelGGL(k_init_scores, dim3(iterations, 2), dim3(kThreads), 0, ctx.stream, dW);
    ctx.clock.mark(2, ctx.stream);
    hipLaunchKernelGGL(k_init_select, dim3(1), dim3(kThreads), 0, ctx.stream, dW);
    ctx.clock.mark(3, ctx.stream);
    hipLaunchKernelGGL(k_init_check_rt, dim3(kMaxMotions), dim3(kThreads), 0, ctx.stream, dW);
    ctx.clock.mark(4, ctx.stream);
    hipLaunchKernelGGL(k_init_finish, dim3(1), dim3(kThreads), 0, ctx.stream, dW);
    ctx.clock.mark(5, ctx.stream);
    EAO_HIP(hipGetLastError());
    EAO_HIP(hipMemcpyAsync(h + oOut, d + oOut, (inspect ? inspEnd : outEnd) - oOut, hipMemcpyDeviceToHost, ctx.stream));
    EAO_HIP(drain.wait(Drain::Latency));
    ctx.clock.collect();
    const Out& O = *(const Out*)(h + oOut);
    r.returned = O.returned; r.branch = O.branch; r.no_model = O.no_model; r.degenerate = O.degenerate;
    r.SH = O.SH; r.SF = O.SF; r.RH = O.RH;
    r.best_h = O.best_h; r.best_f = O.best_f;
    std::memcpy(r.H21, O.H21, 36); std::memcpy(r.F21, O.F21, 36); std::memcpy(r.R21, O.R21, 36); std::memcpy(r.t21, O.t21, 12);
    r.cos_parallax = O.cosine;
    r.parallax = parallax_of(O.cosine);
    r.n_good = O.n_good; r.motion = O.motion; r.n_motions = O.n_motions; r.n_inliers = O.n_inliers;
    if (O.returned) {      // (on false upstream leaves vP3D and vbTriangulated as they were)
        std::memcpy(r.p3d, h + oP3d, 12 * n1);
        std::memcpy(r.triangulated, h + oTri, n1);
    }
    if (r.hyp_H21) std::memcpy(r.hyp_H21, h + oH21, 36 * it);
    if (r.hyp_H12) std::memcpy(r.hyp_H12, h + oH12, 36 * it);
    if (r.hyp_F21) std::memcpy(r.hyp_F21, h + oF21, 36 * it);
    if (r.hyp_SH) std::memcpy(r.hyp_SH, h + oScore, 4 * it);
    if (r.hyp_SF) std::memcpy(r.hyp_SF, h + oScore + 4 * it, 4 * it);
    if (r.hyp_inlier_H) std::memcpy(r.hyp_inlier_H, h + oFlags, it * N);
    if (r.hyp_inlier_F) std::memcpy(r.hyp_inlier_F, h + oFlags + it * N, it * N);
    if (r.inlier) { if (O.no_model) std::memset(r.inlier, 0, N); else std::memcpy(r.inlier, h + oInl, N); }
    for (int m = 0; m < kMaxMotions; m++) {
        const bool live = m < O.n_motions;
        if (r.mot_R) { if (live) std::memcpy(r.mot_R + 9 * m, O.mot[m].R, 36); else std::memset(r.mot_R + 9 * m, 0, 36); }
        if (r.mot_t) { if (live) std::memcpy(r.mot_t + 3 * m, O.mot[m].t, 12); else std::memset(r.mot_t + 3 * m, 0, 12); }
        if (r.mot_n_good) r.mot_n_good[m] = live ? O.mot[m].n_good : 0;
        if (r.mot_cos) r.mot_cos[m] = live ? O.mot[m].cosine : 0.f;
        if (r.mot_good) { if (live) std::memcpy(r.mot_good + m * n1, h + oGood + m * n1, n1); else std::memset(r.mot_good + m * n1, 0, n1); }
        if (r.mot_p3d) { if (live) std::memcpy(r.mot_p3d + 3 * m * n1, h + oMP3d + 12 * m * n1, 12 * n1); else std::memset(r.mot_p3d + 3 * m * n1, 0, 12 * n1); }
    }
    return EAO_OK;
}

eao_status eao_initializer_last_kernel_ms(float* kernel_ms) {
    EAO_REQUIRE(kernel_ms, "null argument");
    return g_init.clock.read(kernel_ms, "no measurement on this thread: EAO_INIT_EVENTS=1 and a call of eao_initializer_initialize come first");
}

}  // extern "C"
