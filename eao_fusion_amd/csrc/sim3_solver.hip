// sim3_solver.hip -- Sim3Solver (reference src/Sim3Solver.cc, include/Sim3Solver.h): the Horn RANSAC of LoopClosing::ComputeSim3
// (src/LoopClosing.cc:286-311), the step between SearchByBoW and SearchBySim3 / OptimizeSim3 (sim3.hip).
//
// One call is one Sim3Solver::iterate.  The hypotheses of the call are independent of each other, so they are evaluated together -- one
// wavefront per hypothesis: every lane computes ComputeSim3 (:226-337) from the three sampled point pairs (uniform work on about 40 floats;
// redundant work beats a broadcast and a barrier), then the lanes stride over the correspondences for CheckInliers (:340-364), count with
// __ballot / __popcll and keep the flags as a bit mask.  A second kernel, one workgroup per problem, replays the sequential part of the loop
// (:183-206) over the counts: pure integer logic, so that only the result and the new state come back.  The host uploads once, launches the
// two kernels on one stream and reads back once.
//
// Arithmetic as upstream writes it: float where it holds CV_32F, double where it holds double.  OpenCV's own arithmetic is not part of the
// reference tree; the choices made for it (DESIGN.md "Sim3Solver", tests/sim3_solver_reference.py):
//  - a small matrix product (Pr2 * Pr1.t(), R * Pr2, R * X + t, ...) accumulates each element in double, k = 0, 1, 2 in order, and rounds once to
//    float; an added or subtracted vector is then added in float (the rule of sim3.hip's camera_point),
//  - a double scalar applied to a float matrix (C / 3, 2 * ang / norm, ms12i * R, 1.0 / ms12i * R.t(), ms12i * (R * O2)) multiplies in double and
//    rounds once; a chain of scalars folds into one double first,
//  - cv::reduce, Mat::dot and cv::norm accumulate in double, in storage order,
//  - N11 .. N44 are float expressions evaluated left to right (at<float> operands), then held in double and stored back as float: exact,
//  - cv::eigen on the symmetric 4 x 4: a cyclic Jacobi solve in double (10 sweeps, fixed), the column of the largest eigenvalue rounded to float;
//    its sign is free (q and -q give the same rotation through atan2(|v|, w) and v / |v|),
//  - cv::Rodrigues in double as OpenCV writes it (theta, c, s, c1 = 1 - c, R = c I + c1 r r^T + s [r]x), rounded once to float.
// Reproduced, not repaired: a zero imaginary part gives 0 / 0 and a NaN T12; Project does not check depth; a NaN error fails both
// comparisons, so that correspondence is an outlier.  The gates are size_t upstream: (float)(size_t)(9.210 * sigma2), made on the host.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <vector>

#include "common.h"

using namespace eao;

namespace {

constexpr int kWave = 64;

struct HypOut {
    float T12[16], T21[16], R[9], t[3], s;
    int inliers;
};

struct SolverOut {
    eao_sim3_solver_state state;
    int returned, n_inliers, no_more, pad;
    float T12[16];
};

// one problem on the device (all arrays device pointers)
struct SolverRec {
    int n, fix_scale, n_eval, min_inliers, max_its, words;      // words: 64-bit mask words per hypothesis
    float fx1, fy1, cx1, cy1, fx2, fy2, cx2, cy2;
    const float* X1c;        // n*3 mvX3Dc1
    const float* X2c;        // n*3 mvX3Dc2
    const float* im1;        // n*2 mvP1im1
    const float* im2;        // n*2 mvP2im2
    const float* max1;       // n   mvnMaxError1 as the comparison reads it
    const float* max2;       // n
    const int* triples;      // n_eval*3
    HypOut* hyp;             // n_eval
    unsigned long long* masks;   // n_eval*words
    SolverOut* out;
    unsigned char* inlier;   // n
    eao_sim3_solver_state state;
};

// ---------------------------------------------------------------------- the arithmetic rules (one place each)
__host__ __device__ inline float dot3(float a0, float a1, float a2, float b0, float b1, float b2) {   // one element of a small gemm
    return (float)((double)a0 * (double)b0 + (double)a1 * (double)b1 + (double)a2 * (double)b2);
}
__host__ __device__ inline float scaled(double s, float v) { return (float)(s * (double)v); }           // double scalar * float matrix element

// Rcw * X + tcw of a row-major 3 x 4 (stride 4) float transform
__host__ __device__ inline void transform_point(const float* T, const float* X, float out[3]) {
    for (int i = 0; i < 3; i++) out[i] = dot3(T[4 * i], T[4 * i + 1], T[4 * i + 2], X[0], X[1], X[2]) + T[4 * i + 3];
}
// FromCameraToImage / Project's tail (:397-401)
__host__ __device__ inline void to_image(const float P[3], float fx, float fy, float cx, float cy, float uv[2]) {
    const float invz = 1 / P[2];
    const float x = P[0] * invz, y = P[1] * invz;
    uv[0] = fx * x + cx;
    uv[1] = fy * y + cy;
}

// cv::eigen's part: eigenvector of the largest eigenvalue of the symmetric 4 x 4 (float entries) by cyclic Jacobi in double.  A fixed number of
// sweeps: no data-dependent loop, so NaN input ends like any other.  An exactly zero off-diagonal entry is skipped (nothing to annihilate).
__device__ inline void top_eigenvector(const float Nf[4][4], float q[4]) {
    double A[4][4], V[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) { A[i][j] = Nf[i][j]; V[i][j] = (i == j) ? 1.0 : 0.0; }
#pragma unroll 1
    for (int sweep = 0; sweep < 10; sweep++) {
#pragma unroll
        for (int p = 0; p < 3; p++)
#pragma unroll
            for (int r = p + 1; r < 4; r++) {
                const double apq = A[p][r];
                if (apq != 0) {
                    const double theta = (A[r][r] - A[p][p]) / (2 * apq);
                    const double t = (theta < 0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1));
                    const double c = 1 / sqrt(t * t + 1), s = t * c;
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const double akp = A[k][p], akq = A[k][r];
                        A[k][p] = c * akp - s * akq;
                        A[k][r] = s * akp + c * akq;
                    }
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const double apk = A[p][k], aqk = A[r][k];
                        A[p][k] = c * apk - s * aqk;
                        A[r][k] = s * apk + c * aqk;
                    }
                    A[p][r] = 0; A[r][p] = 0;
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const double vkp = V[k][p], vkq = V[k][r];
                        V[k][p] = c * vkp - s * vkq;
                        V[k][r] = s * vkp + c * vkq;
                    }
                }
            }
    }
    double best = A[0][0];
    double v[4] = {V[0][0], V[1][0], V[2][0], V[3][0]};
#pragma unroll
    for (int k = 1; k < 4; k++)
        if (A[k][k] > best) {
            best = A[k][k];
#pragma unroll
            for (int i = 0; i < 4; i++) v[i] = V[i][k];
        }
#pragma unroll
    for (int i = 0; i < 4; i++) q[i] = (float)v[i];
}

// Sim3Solver::ComputeSim3 (:226-337).  P1 / P2: [row][point], the 3 x 3 of :154-155.
__device__ inline void compute_sim3(const float P1[3][3], const float P2[3][3], bool fix_scale, HypOut& o) {
    // Step 1: centroids and relative coordinates (ComputeCentroid :215-224)
    float Pr1[3][3], Pr2[3][3], O1[3], O2[3];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const float s1 = (float)((double)P1[r][0] + (double)P1[r][1] + (double)P1[r][2]);
        const float s2 = (float)((double)P2[r][0] + (double)P2[r][1] + (double)P2[r][2]);
        O1[r] = scaled(1.0 / 3, s1);
        O2[r] = scaled(1.0 / 3, s2);
#pragma unroll
        for (int i = 0; i < 3; i++) { Pr1[r][i] = P1[r][i] - O1[r]; Pr2[r][i] = P2[r][i] - O2[r]; }
    }
    // Step 2: M = Pr2 * Pr1.t()
    float M[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) M[i][j] = dot3(Pr2[i][0], Pr2[i][1], Pr2[i][2], Pr1[j][0], Pr1[j][1], Pr1[j][2]);
    // Step 3: N (:251-265)
    const float N11 = M[0][0] + M[1][1] + M[2][2];
    const float N12 = M[1][2] - M[2][1];
    const float N13 = M[2][0] - M[0][2];
    const float N14 = M[0][1] - M[1][0];
    const float N22 = M[0][0] - M[1][1] - M[2][2];
    const float N23 = M[0][1] + M[1][0];
    const float N24 = M[2][0] + M[0][2];
    const float N33 = -M[0][0] + M[1][1] - M[2][2];
    const float N34 = M[1][2] + M[2][1];
    const float N44 = -M[0][0] - M[1][1] + M[2][2];
    const float N[4][4] = {{N11, N12, N13, N14}, {N12, N22, N23, N24}, {N13, N23, N33, N34}, {N14, N24, N34, N44}};
    // Step 4: eigenvector of the highest eigenvalue, angle-axis, Rodrigues (:270-284)
    float q[4];
    top_eigenvector(N, q);
    const double nrm = sqrt((double)q[1] * (double)q[1] + (double)q[2] * (double)q[2] + (double)q[3] * (double)q[3]);
    const double ang = atan2(nrm, (double)q[0]);
    const double k = (2 * ang) / nrm;
    const float rv[3] = {scaled(k, q[1]), scaled(k, q[2]), scaled(k, q[3])};
    float R[3][3];
    {
        const double rx0 = rv[0], ry0 = rv[1], rz0 = rv[2];
        const double theta = sqrt(rx0 * rx0 + ry0 * ry0 + rz0 * rz0);
        if (theta < DBL_EPSILON) {
#pragma unroll
            for (int i = 0; i < 3; i++)
#pragma unroll
                for (int j = 0; j < 3; j++) R[i][j] = (i == j) ? 1.f : 0.f;
        } else {
            const double c = cos(theta), s = sin(theta), c1 = 1. - c, it = 1. / theta;
            const double r[3] = {rx0 * it, ry0 * it, rz0 * it};
            const double skew[3][3] = {{0, -r[2], r[1]}, {r[2], 0, -r[0]}, {-r[1], r[0], 0}};
#pragma unroll
            for (int i = 0; i < 3; i++)
#pragma unroll
                for (int j = 0; j < 3; j++) R[i][j] = (float)(c * ((i == j) ? 1.0 : 0.0) + c1 * (r[i] * r[j]) + s * skew[i][j]);
        }
    }
    // Step 5: P3 = R * Pr2; Step 6: scale (:288-311)
    float ms = 1.0f;
    if (!fix_scale) {
        double nom = 0, den = 0;
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const float p3 = dot3(R[i][0], R[i][1], R[i][2], Pr2[0][j], Pr2[1][j], Pr2[2][j]);
                nom += (double)Pr1[i][j] * (double)p3;
                den += (double)(p3 * p3);
            }
        ms = (float)(nom / den);
    }
    // Step 7: t = O1 - ms * R * O2; Step 8: T12 = [ms R | t], T21 = [1 / ms R^T | -(1 / ms R^T) t]
    const double msd = ms, inv = 1.0 / (double)ms;
    float t[3], sR[3][3], sRi[3][3], ti[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const double acc = (double)R[i][0] * (double)O2[0] + (double)R[i][1] * (double)O2[1] + (double)R[i][2] * (double)O2[2];
        t[i] = O1[i] - (float)(msd * acc);
#pragma unroll
        for (int j = 0; j < 3; j++) { sR[i][j] = scaled(msd, R[i][j]); sRi[i][j] = scaled(inv, R[j][i]); }
    }
#pragma unroll
    for (int i = 0; i < 3; i++) ti[i] = -dot3(sRi[i][0], sRi[i][1], sRi[i][2], t[0], t[1], t[2]);
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) { o.T12[4 * i + j] = sR[i][j]; o.T21[4 * i + j] = sRi[i][j]; o.R[3 * i + j] = R[i][j]; }
        o.T12[4 * i + 3] = t[i];
        o.T21[4 * i + 3] = ti[i];
        o.t[i] = t[i];
        o.T12[12 + i] = 0; o.T21[12 + i] = 0;
    }
    o.T12[15] = 1; o.T21[15] = 1;
    o.s = ms;
}

// ---------------------------------------------------------------------- kernels
// grid (hypothesis, problem), one wave64 each
__global__ __launch_bounds__(kWave) void k_sim3_solver_hypotheses(const SolverRec* __restrict__ W) {
    const SolverRec& P = W[blockIdx.y];
    const int h = blockIdx.x, lane = threadIdx.x;
    if (h >= P.n_eval) return;                 // (uniform over the wave)
    const int n = P.n;
    float P1[3][3], P2[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        int idx = P.triples[3 * h + i];
        idx = idx < 0 ? 0 : (idx >= n ? n - 1 : idx);     // validated on the host; clamped all the same, n_eval > 0 implies n > 0
#pragma unroll
        for (int r = 0; r < 3; r++) { P1[r][i] = P.X1c[3 * idx + r]; P2[r][i] = P.X2c[3 * idx + r]; }
    }
    HypOut o;
    compute_sim3(P1, P2, P.fix_scale != 0, o);
    // CheckInliers (:340-364)
    int count = 0;
    unsigned long long* mask = P.masks + (size_t)h * P.words;
    for (int base = 0; base < n; base += kWave) {
        const int i = base + lane;
        bool in = false;
        if (i < n) {
            const float X1[3] = {P.X1c[3 * i], P.X1c[3 * i + 1], P.X1c[3 * i + 2]};
            const float X2[3] = {P.X2c[3 * i], P.X2c[3 * i + 1], P.X2c[3 * i + 2]};
            float p[3], uv[2];
            transform_point(o.T12, X2, p);                       // vP2im1
            to_image(p, P.fx1, P.fy1, P.cx1, P.cy1, uv);
            const float d10 = P.im1[2 * i] - uv[0], d11 = P.im1[2 * i + 1] - uv[1];
            transform_point(o.T21, X1, p);                       // vP1im2
            to_image(p, P.fx2, P.fy2, P.cx2, P.cy2, uv);
            const float d20 = uv[0] - P.im2[2 * i], d21 = uv[1] - P.im2[2 * i + 1];
            const float err1 = (float)((double)d10 * (double)d10 + (double)d11 * (double)d11);
            const float err2 = (float)((double)d20 * (double)d20 + (double)d21 * (double)d21);
            in = err1 < P.max1[i] && err2 < P.max2[i];
        }
        const unsigned long long m = __ballot(in);
        if (lane == 0) mask[base / kWave] = m;
        count += __popcll(m);
    }
    if (lane == 0) {
        o.inliers = count;
        P.hyp[h] = o;
    }
}

// one workgroup per problem: the sequential part of iterate (:158-206) over the counts, the new state, the winner's flags
__global__ __launch_bounds__(kWave) void k_sim3_solver_scan(const SolverRec* __restrict__ W) {
    const SolverRec& P = W[blockIdx.x];
    __shared__ int sh_returned;
    if (threadIdx.x == 0) {
        SolverOut r;
        r.state = P.state;
        r.returned = -1; r.n_inliers = 0; r.no_more = 0; r.pad = 0;
        for (int k = 0; k < 16; k++) r.T12[k] = 0;
        if (P.n < P.min_inliers) {
            r.no_more = 1;
        } else {
            int best = -1;
            for (int k = 0; k < P.n_eval; k++) {
                r.state.iterations++;
                const int c = P.hyp[k].inliers;
                if (c >= r.state.best_inliers) {
                    r.state.best_inliers = c;
                    best = k;
                    if (c > P.min_inliers) { r.returned = k; break; }
                }
            }
            if (best >= 0) {
                const HypOut& b = P.hyp[best];
                for (int k = 0; k < 16; k++) r.state.best_T12[k] = b.T12[k];
                for (int k = 0; k < 9; k++) r.state.best_R[k] = b.R[k];
                for (int k = 0; k < 3; k++) r.state.best_t[k] = b.t[k];
                r.state.best_s = b.s;
            }
            if (r.returned >= 0) {
                r.n_inliers = r.state.best_inliers;
                for (int k = 0; k < 16; k++) r.T12[k] = r.state.best_T12[k];
            } else if (r.state.iterations >= P.max_its) {
                r.no_more = 1;
            }
        }
        *P.out = r;
        sh_returned = r.returned;
    }
    __syncthreads();
    const int ret = sh_returned;
    if (ret < 0) return;
    const unsigned long long* mask = P.masks + (size_t)ret * P.words;
    for (int i = threadIdx.x; i < P.n; i += kWave) P.inlier[i] = (unsigned char)((mask[i >> 6] >> (i & 63)) & 1ull);
}

// ---------------------------------------------------------------------- host side
struct SolverCtx : ThreadStream {
    DevBuf<unsigned char> dev;
    std::vector<unsigned char> host;
};
thread_local SolverCtx g_solver;

struct Call {
    const eao_sim3_solver_problem* p;
    int min_inliers, max_its;
    eao_sim3_solver_state* state;
    const int32_t* triples;
    int n_hyp;
    eao_sim3_solver_result* r;
    int n_eval;
    size_t offIn, offHyp, offMask, offInl;
};

eao_status check_call(Call& c) {
    EAO_REQUIRE(c.p && c.state && c.r, "null argument");
    const eao_sim3_solver_problem& p = *c.p;
    EAO_REQUIRE(p.n >= 0, "bad problem: n = %d", p.n);
    EAO_REQUIRE(c.n_hyp >= 0 && c.max_its >= 0 && c.min_inliers >= 0, "bad call: n_hyp %d, max_its %d, min_inliers %d", c.n_hyp, c.max_its, c.min_inliers);
    EAO_REQUIRE(p.n == 0 || (p.T1w && p.T2w && p.Xw1 && p.Xw2 && p.sigma2_1 && p.sigma2_2), "bad problem: missing arrays");
    EAO_REQUIRE(c.state->iterations >= 0, "bad state: iterations = %d", c.state->iterations);
    for (int i = 0; i < p.n; i++)
        EAO_REQUIRE(p.sigma2_1[i] >= 0 && p.sigma2_1[i] <= 1e12f && p.sigma2_2[i] >= 0 && p.sigma2_2[i] <= 1e12f, "bad problem: sigma2 of correspondence %d", i);
    c.n_eval = 0;
    if (p.n < c.min_inliers) return EAO_OK;      // iterate returns before it draws (:146-150): the triples are not read
    const int left = c.max_its - c.state->iterations;
    c.n_eval = std::max(0, std::min(c.n_hyp, left));
    EAO_REQUIRE(c.n_hyp == 0 || c.triples, "bad call: triples missing");
    EAO_REQUIRE(c.n_eval == 0 || p.n > 0, "bad call: hypotheses over no correspondence");
    EAO_REQUIRE(c.n_eval == 0 || c.r->inlier, "bad call: result->inlier missing");
    for (size_t k = 0; k < (size_t)c.n_hyp * 3; k++)
        EAO_REQUIRE(c.triples[k] >= 0 && c.triples[k] < p.n, "bad call: triple index %d at %zu, n = %d", c.triples[k], k, p.n);
    return EAO_OK;
}

eao_status run_solver(std::vector<Call>& calls) {
    const int nb = (int)calls.size();
    for (Call& c : calls) {
        eao_status st = check_call(c);
        if (st) return st;
    }
    SolverCtx& ctx = g_solver;
    eao_status st = ctx.ready(StreamClass::Latency);     // LoopClosing's thread waits for the call, as for eao_optimize_sim3
    if (st) return st;
    // layout: [records][per problem: 12 n floats, 3 n_eval ints] | [outputs][per problem: inlier n] | [per problem: HypOut n_eval, masks]
    size_t off = align256(sizeof(SolverRec) * nb);
    int maxEval = 0;
    bool inspect = false;
    for (Call& c : calls) {
        c.offIn = off;
        off = align256(off + (size_t)c.p->n * 12 * sizeof(float) + (size_t)c.n_eval * 3 * sizeof(int));
        maxEval = std::max(maxEval, c.n_eval);
        inspect = inspect || c.r->hyp_inliers || c.r->hyp_T12 || c.r->hyp_T21 || c.r->hyp_inlier;
    }
    const size_t inEnd = off, offOut = off;
    off = align256(off + sizeof(SolverOut) * nb);
    for (Call& c : calls) { c.offInl = off; off += (size_t)c.p->n; }
    const size_t outEnd = off;
    off = align256(off);
    const size_t hypBegin = off;
    for (Call& c : calls) {
        const size_t words = ((size_t)c.p->n + 63) / 64;
        c.offHyp = off;
        off = align256(off + sizeof(HypOut) * c.n_eval);
        c.offMask = off;
        off = align256(off + sizeof(unsigned long long) * words * c.n_eval);
    }
    const size_t total = std::max<size_t>(off, 256);
    if ((st = ctx.dev.reserve(total))) return st;
    if (ctx.host.size() < total) ctx.host.resize(total);
    unsigned char* h = ctx.host.data();
    unsigned char* d = ctx.dev.p;
    SolverRec* recs = (SolverRec*)h;
    for (int b = 0; b < nb; b++) {
        const Call& c = calls[b];
        const eao_sim3_solver_problem& p = *c.p;
        const size_t n = (size_t)p.n;
        float* X1 = (float*)(h + c.offIn);
        float* X2 = X1 + 3 * n;
        float* im1 = X2 + 3 * n;
        float* im2 = im1 + 2 * n;
        float* max1 = im2 + 2 * n;
        float* max2 = max1 + n;
        int* tri = (int*)(max2 + n);
        for (size_t i = 0; i < n; i++) {
            transform_point(p.T1w, p.Xw1 + 3 * i, X1 + 3 * i);                     // :95
            transform_point(p.T2w, p.Xw2 + 3 * i, X2 + 3 * i);                     // :98
            to_image(X1 + 3 * i, p.fx1, p.fy1, p.cx1, p.cy1, im1 + 2 * i);         // :108
            to_image(X2 + 3 * i, p.fx2, p.fy2, p.cx2, p.cy2, im2 + 2 * i);         // :109
            max1[i] = (float)(size_t)(9.210 * p.sigma2_1[i]);                      // :87, read back as float in err1 < mvnMaxError1[i]
            max2[i] = (float)(size_t)(9.210 * p.sigma2_2[i]);
        }
        if (c.n_eval) std::memcpy(tri, c.triples, (size_t)c.n_eval * 3 * sizeof(int));
        SolverRec& R = recs[b];
        std::memset(&R, 0, sizeof(R));
        R.n = p.n; R.fix_scale = p.fix_scale ? 1 : 0; R.n_eval = c.n_eval; R.min_inliers = c.min_inliers; R.max_its = c.max_its;
        R.words = (int)((n + 63) / 64);
        R.fx1 = p.fx1; R.fy1 = p.fy1; R.cx1 = p.cx1; R.cy1 = p.cy1;
        R.fx2 = p.fx2; R.fy2 = p.fy2; R.cx2 = p.cx2; R.cy2 = p.cy2;
        R.X1c = (const float*)(d + c.offIn);
        R.X2c = R.X1c + 3 * n;
        R.im1 = R.X2c + 3 * n;
        R.im2 = R.im1 + 2 * n;
        R.max1 = R.im2 + 2 * n;
        R.max2 = R.max1 + n;
        R.triples = (const int*)(R.max2 + n);
        R.hyp = (HypOut*)(d + c.offHyp);
        R.masks = (unsigned long long*)(d + c.offMask);
        R.out = (SolverOut*)(d + offOut) + b;
        R.inlier = d + c.offInl;
        R.state = *c.state;
    }
    Drain drain(ctx.stream);
    EAO_HIP(hipMemcpyAsync(d, h, inEnd, hipMemcpyHostToDevice, ctx.stream));
    if (maxEval > 0) hipLaunchKernelGGL(k_sim3_solver_hypotheses, dim3(maxEval, nb), dim3(kWave), 0, ctx.stream, (const SolverRec*)d);
    EAO_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_sim3_solver_scan, dim3(nb), dim3(kWave), 0, ctx.stream, (const SolverRec*)d);
    EAO_HIP(hipGetLastError());
    EAO_HIP(hipMemcpyAsync(h + offOut, d + offOut, outEnd - offOut, hipMemcpyDeviceToHost, ctx.stream));
    if (inspect && total > hypBegin) EAO_HIP(hipMemcpyAsync(h + hypBegin, d + hypBegin, total - hypBegin, hipMemcpyDeviceToHost, ctx.stream));
    EAO_HIP(drain.wait(Drain::Block));
    const SolverOut* outs = (const SolverOut*)(h + offOut);
    for (int b = 0; b < nb; b++) {
        const Call& c = calls[b];
        const SolverOut& o = outs[b];
        const size_t n = (size_t)c.p->n;
        eao_sim3_solver_result& r = *c.r;
        *c.state = o.state;
        r.returned = o.returned; r.n_inliers = o.n_inliers; r.no_more = o.no_more;
        std::memcpy(r.T12, o.T12, sizeof(r.T12));
        if (o.returned >= 0 && n) std::memcpy(r.inlier, h + c.offInl, n);
        const HypOut* hyp = (const HypOut*)(h + c.offHyp);
        const unsigned long long* masks = (const unsigned long long*)(h + c.offMask);
        const size_t words = (n + 63) / 64;
        for (int k = 0; k < c.n_hyp; k++) {
            const bool ev = k < c.n_eval;
            if (r.hyp_inliers) r.hyp_inliers[k] = ev ? hyp[k].inliers : 0;
            if (r.hyp_T12) { if (ev) std::memcpy(r.hyp_T12 + 16 * (size_t)k, hyp[k].T12, 64); else std::memset(r.hyp_T12 + 16 * (size_t)k, 0, 64); }
            if (r.hyp_T21) { if (ev) std::memcpy(r.hyp_T21 + 16 * (size_t)k, hyp[k].T21, 64); else std::memset(r.hyp_T21 + 16 * (size_t)k, 0, 64); }
            if (r.hyp_inlier)
                for (size_t i = 0; i < n; i++) r.hyp_inlier[(size_t)k * n + i] = ev ? (unsigned char)((masks[(size_t)k * words + (i >> 6)] >> (i & 63)) & 1ull) : 0;
        }
    }
    return EAO_OK;
}

}  // namespace

extern "C" {

eao_status eao_sim3_solver_iterate(const eao_sim3_solver_problem* problem, int32_t min_inliers, int32_t max_its, eao_sim3_solver_state* state,
                                   const int32_t* triples, int32_t n_hyp, eao_sim3_solver_result* result) {
    std::vector<Call> calls(1);
    calls[0] = Call{problem, min_inliers, max_its, state, triples, n_hyp, result, 0, 0, 0, 0, 0};
    return run_solver(calls);
}

eao_status eao_sim3_solver_iterate_batch(int32_t n_problems, const eao_sim3_solver_problem* problems, const int32_t* min_inliers, const int32_t* max_its,
                                         eao_sim3_solver_state* states, const int32_t* const* triples, const int32_t* n_hyp,
                                         eao_sim3_solver_result* results) {
    EAO_REQUIRE(n_problems >= 0 && (n_problems == 0 || (problems && min_inliers && max_its && states && triples && n_hyp && results)), "bad batch");
    if (n_problems == 0) return EAO_OK;
    std::vector<Call> calls(n_problems);
    for (int b = 0; b < n_problems; b++)
        calls[b] = Call{&problems[b], min_inliers[b], max_its[b], &states[b], triples[b], n_hyp[b], &results[b], 0, 0, 0, 0, 0};
    return run_solver(calls);
}

}  // extern "C"
