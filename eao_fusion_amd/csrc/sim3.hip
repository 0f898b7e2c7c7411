// sim3.hip -- Optimizer::OptimizeSim3 (reference src/Optimizer.cc:1437-1632): the Sim3 refinement of LoopClosing::ComputeSim3
// (src/LoopClosing.cc:292-345) between Sim3Solver's RANSAC (sim3_solver.hip) and the nInliers >= 20 decision.
//
// The problem is small and dense like PoseOptimization: ONE free 7-dof vertex (VertexSim3Expmap), fixed camera-frame points,
// two edges per correspondence (EdgeSim3ProjectXYZ: obs1 vs S12 * X2c in camera 1; EdgeInverseSim3ProjectXYZ: obs2 vs S12^-1 * X1c
// in camera 2), Huber with delta = sqrtf(th2), 5 LM iterations, the chi2 > th2 inlier pass, 5 or 10 more, the final pass.  One
// persistent workgroup per problem runs all of it; the host uploads once, launches once and reads back once.
//
// g2o details reproduced (Thirdparty/g2o/g2o):
//  - types/sim3.h:70-141  the exp map (four branches on |sigma| < 1e-5 and theta < 1e-5, written as upstream writes them, including
//    R = I + Omega + Omega^2 in the small-angle branches), Quaterniond(R) (Eigen's trace / largest-diagonal branches), map, inverse,
//    operator*.  Quaternion products are NOT renormalised (g2o::Sim3 never does, unlike SE3Quat).
//  - types_seven_dof_expmap.h:48-170  oplusImpl: S <- Sim3(update) * S, update[6] = 0 under _fix_scale; the edges' analytic Jacobians are
//    commented out upstream, so they are numeric: core/base_binary_edge.hpp:147-196, central differences with delta = 1e-9, columns
//    (e(+delta) - e(-delta)) * (1 / (2 delta)); the point vertices are fixed and get none.  The 14 perturbed estimates Sim3(+-delta e_d) * S
//    (and their inverses, for the inverse edge) are the same for every edge: they are built ONCE per linearisation in LDS -- the same
//    values g2o rebuilds for each edge.  Under _fix_scale the 7th column is exactly zero and H77 = lambda after damping: dx[6] = 0.
//  - core/optimization_algorithm_levenberg.cpp:61-189  lambda0 = tau * max diag at iteration 0 of each optimize(), rho with the +1e-3
//    scale, nu doubling, at most 10 trials, the "3 bad iterations" stop.
//  - solvers/linear_solver_dense.h:104-112  Eigen's LDLT + isPositive: the unpivoted 7 x 7 LDL^T below has the same inertia, hence the
//    same success / failure decision.  On failure upstream applies whatever the solver's x held; here x = 0 (the trial is then rejected,
//    tempChi = DBL_MAX).  With lambda > 0 the damped system is positive definite and this never happens.
//  - the inlier passes read e->chi2() as it stands: the error of the LAST TRIAL evaluated, which may be a rejected one (pop() does not
//    recompute errors).  Each evaluation therefore writes its gate flags per correspondence; the last writer is what the pass reads.
//  - no depth check: project() divides by whatever z is.
#include "sim3_internal.h"

using namespace eao;
using namespace eao::lm;

namespace {

constexpr int kSim3Threads = 256;
constexpr double kSim3Delta = 1e-9;                       // core/base_binary_edge.hpp:147

struct Sim3Out {
    Sim3 S;
    int n_inliers, iters0, iters1, early_exit;
};

// one problem on the device (all arrays device pointers)
struct Sim3Rec {
    int n, fix_scale;
    double th2, delta;          // the gate and the Huber width (g2o squares it itself)
    double fx1, fy1, cx1, cy1, fx2, fy2, cx2, cy2;
    const double* X1c;       // n*3 camera-1 points (vertex id1 of upstream)
    const double* X2c;       // n*3 camera-2 points (id2)
    const double* o1;        // n*2 measurement of e12
    const double* o2;        // n*2 measurement of e21
    const double* i1;        // n   information of e12
    const double* i2;        // n   information of e21
    Sim3 S0;
    unsigned char* removed;  // n: vpMatches1 nulled
    unsigned char* lastbad;  // n: chi2 gate of the last evaluated state
    Sim3Out* out;
};

// obs - cam_map(project(S.map(X)))
__device__ inline void proj_error(const Sim3& S, const double X[3], double ox, double oy, double fx, double fy, double cx, double cy, double e[2]) {
    double p[3];
    quat_rotate(S.r, X, p);
    for (int k = 0; k < 3; k++) p[k] = S.s * p[k] + S.t[k];
    const double u = p[0] / p[2], v = p[1] / p[2];
    e[0] = ox - (u * fx + cx);
    e[1] = oy - (v * fy + cy);
}

// 7 x 7 LDL^T solve of (H + lambda I) x = b (the ldlt6_solve pattern of lm_internal.h): unpivoted, same inertia as Eigen's pivoted
// LDLT.  Hp: H's upper triangle packed row by row.
__device__ inline bool ldlt7_solve(const double* Hp, double lambda, const double* b, double* x) {
    double a[7][7], y[7];
#pragma unroll
    for (int r = 0, k = 0; r < 7; r++)
#pragma unroll
        for (int c = r; c < 7; c++, k++) a[r][c] = Hp[k] + (r == c ? lambda : 0.0);
    bool positive = true;
#pragma unroll
    for (int r = 0; r < 7; r++) {
        const double d = a[r][r];
        if (!(d > 0)) positive = false;
#pragma unroll
        for (int i = r + 1; i < 7; i++) {
            const double l = a[r][i] / d;
#pragma unroll
            for (int c = i; c < 7; c++) a[i][c] = a[i][c] - l * a[r][c];
            a[i][r] = l;
        }
    }
    if (!positive) return false;
#pragma unroll
    for (int i = 0; i < 7; i++) {
        double v = b[i];
#pragma unroll
        for (int k = 0; k < i; k++) v = v - a[i][k] * y[k];
        y[i] = v;
    }
#pragma unroll
    for (int i = 6; i >= 0; i--) {
        double v = y[i] / a[i][i];
#pragma unroll
        for (int k = i + 1; k < 7; k++) v = v - a[k][i] * x[k];
        x[i] = v;
    }
    return true;
}

// ---------------------------------------------------------------------- the kernel
struct Sim3Shared {
    Sim3 pert[14], pertInv[14];      // Sim3(+-delta e_d) * cur and inverses: [2d] = +delta, [2d + 1] = -delta
    Sim3 curS[2];                    // the current estimate and its inverse during a linearisation
    double jac[14 * kSim3Threads];   // each thread's 2 x 7 Jacobian of the edge at hand: entry (row r, column d) at [(2 d + r) * 256 + thread]      // Sim3(+-delta e_d) * cur and inverses: [2d] = +delta, [2d + 1] = -delta
    double red[(kSim3Threads / 64) * 36];
    double sum[36];                  // the linearisation's sums: H upper triangle (28, row by row), b (7), robust chi2
    double chi[1];                   // a trial's robust chi2
};

// Fixed-order sum of NV accumulators over the workgroup: a butterfly of __shfl_xor per wave (lane 0's total is used), then the
// four wave totals in wave order.  out[0 .. NV) is valid in every thread on return, so every thread can run the LM arithmetic itself.
template <int NV>
__device__ inline void wg_sum(double (&v)[NV], double* red /* (kSim3Threads / 64) * NV */, double* out) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < NV; k++) {
        double x = v[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
        if (lane == 0) red[wv * NV + k] = x;
    }
    __syncthreads();
    if (threadIdx.x < NV) {
        double s = 0;
        for (int w = 0; w < kSim3Threads / 64; w++) s += red[w * NV + threadIdx.x];
        out[threadIdx.x] = s;
    }
    __syncthreads();
}

// the two errors of correspondence m at (S, S^-1)
__device__ __forceinline__ void edge_errors(const Sim3Rec& P, int m, const Sim3& S, const Sim3& Si, double e12[2], double e21[2]) {
    const double X1[3] = {P.X1c[3 * m], P.X1c[3 * m + 1], P.X1c[3 * m + 2]};
    const double X2[3] = {P.X2c[3 * m], P.X2c[3 * m + 1], P.X2c[3 * m + 2]};
    proj_error(S, X2, P.o1[2 * m], P.o1[2 * m + 1], P.fx1, P.fy1, P.cx1, P.cy1, e12);
    proj_error(Si, X1, P.o2[2 * m], P.o2[2 * m + 1], P.fx2, P.fy2, P.cx2, P.cy2, e21);
}

__device__ __forceinline__ double chi2_of(const double e[2], double info) { return e[0] * (info * e[0]) + e[1] * (info * e[1]); }

// Evaluates every active edge at (S, S^-1): robust chi2 summed over the workgroup (valid in all threads on return), and the
// inlier gate of this state into lastbad (computeActiveErrors).
__device__ double evaluate(const Sim3Rec& P, Sim3Shared& sh, const Sim3& S, const Sim3& Si) {
    double acc[1] = {0};
    for (int m = threadIdx.x; m < P.n; m += kSim3Threads) {
        if (P.removed[m]) continue;
        double e12[2], e21[2], r0, r1;
        edge_errors(P, m, S, Si, e12, e21);
        const double c12 = chi2_of(e12, P.i1[m]), c21 = chi2_of(e21, P.i2[m]);
        P.lastbad[m] = (c12 > P.th2 || c21 > P.th2) ? 1 : 0;
        huber(c12, P.delta, r0, r1); acc[0] += r0;
        huber(c21, P.delta, r0, r1); acc[0] += r0;
    }
    wg_sum<1>(acc, sh.red, sh.chi);
    return sh.chi[0];
}

// J^T (rho' Omega) J and J^T omega_r of one edge into the 28 + 7 accumulators
__device__ __forceinline__ void accumulate(double (&acc)[36], const double J[2][7], const double e[2], double info, double rho1) {
    const double w = rho1 * info;
    const double or0 = -(info * e[0]) * rho1, or1 = -(info * e[1]) * rho1;
    int k = 0;
#pragma unroll
    for (int a = 0; a < 7; a++)
#pragma unroll
        for (int c = a; c < 7; c++) acc[k++] += J[0][a] * w * J[0][c] + J[1][a] * w * J[1][c];
#pragma unroll
    for (int a = 0; a < 7; a++) acc[28 + a] += J[0][a] * or0 + J[1][a] * or1;
}

__device__ __forceinline__ void load_jacobian(const double* jac, double (&J)[2][7]) {
#pragma unroll
    for (int d = 0; d < 7; d++) { J[0][d] = jac[(2 * d) * kSim3Threads]; J[1][d] = jac[(2 * d + 1) * kSim3Threads]; }
}

// computeActiveErrors + buildSystem over the active edges at sh.curS (numeric linearisation): H's upper triangle, b and the robust chi2
// into sh.sum.  Register budget: the 36 accumulators and one edge's 2 x 7 Jacobian.  The 14 error evaluations of an edge run as a loop
// (not unrolled) whose columns go to this thread's slots of sh.jac: unrolled, the compiler loaded all 28 perturbed estimates at once
// (448 VGPRs) and spilled the loop to scratch.  Out of line, so that the serial LM arithmetic (7 x 7 LDL^T, the exp map) does not share
// its register allocation.
__device__ __attribute__((noinline)) void linearize(const Sim3Rec& P, Sim3Shared& sh) {
    const int t = threadIdx.x;
    double acc[36];
#pragma unroll
    for (int k = 0; k < 36; k++) acc[k] = 0;
    const double scalar = 1.0 / (2 * kSim3Delta);
#pragma unroll 1
    for (int m = t; m < P.n; m += kSim3Threads) {
        if (P.removed[m]) continue;
        const double X1[3] = {P.X1c[3 * m], P.X1c[3 * m + 1], P.X1c[3 * m + 2]};
        const double X2[3] = {P.X2c[3 * m], P.X2c[3 * m + 1], P.X2c[3 * m + 2]};
        const double o1x = P.o1[2 * m], o1y = P.o1[2 * m + 1], o2x = P.o2[2 * m], o2y = P.o2[2 * m + 1];
        const double in1 = P.i1[m], in2 = P.i2[m];
        double e12[2], e21[2], r0, r1;
        proj_error(sh.curS[0], X2, o1x, o1y, P.fx1, P.fy1, P.cx1, P.cy1, e12);
        proj_error(sh.curS[1], X1, o2x, o2y, P.fx2, P.fy2, P.cx2, P.cy2, e21);
        double J[2][7];
        double* jac = sh.jac + t;     // this thread's column of the Jacobian buffer
        // EdgeSim3ProjectXYZ
#pragma unroll 1
        for (int d = 0; d < 7; d++) {
            double ep[2], em[2];
            proj_error(sh.pert[2 * d], X2, o1x, o1y, P.fx1, P.fy1, P.cx1, P.cy1, ep);
            proj_error(sh.pert[2 * d + 1], X2, o1x, o1y, P.fx1, P.fy1, P.cx1, P.cy1, em);
            jac[(2 * d) * kSim3Threads] = scalar * (ep[0] - em[0]);
            jac[(2 * d + 1) * kSim3Threads] = scalar * (ep[1] - em[1]);
        }
        load_jacobian(jac, J);
        const double c12 = chi2_of(e12, in1);
        huber(c12, P.delta, r0, r1);
        acc[35] += r0;
        accumulate(acc, J, e12, in1, r1);
        // EdgeInverseSim3ProjectXYZ
#pragma unroll 1
        for (int d = 0; d < 7; d++) {
            double ep[2], em[2];
            proj_error(sh.pertInv[2 * d], X1, o2x, o2y, P.fx2, P.fy2, P.cx2, P.cy2, ep);
            proj_error(sh.pertInv[2 * d + 1], X1, o2x, o2y, P.fx2, P.fy2, P.cx2, P.cy2, em);
            jac[(2 * d) * kSim3Threads] = scalar * (ep[0] - em[0]);
            jac[(2 * d + 1) * kSim3Threads] = scalar * (ep[1] - em[1]);
        }
        load_jacobian(jac, J);
        const double c21 = chi2_of(e21, in2);
        huber(c21, P.delta, r0, r1);
        acc[35] += r0;
        accumulate(acc, J, e21, in2, r1);
    }
    wg_sum<36>(acc, sh.red, sh.sum);
}

// SparseOptimizer::optimize(its) over the active edges; returns the iterations done.  The LM state (estimate, lambda, nu, chi2) lives
// in the registers of EVERY thread: all of them read the same workgroup sums and run the same serial arithmetic, so they hold the same
// values and no hand-over through LDS is needed for it.  Only the 14 perturbed estimates (made by threads 0..13) and the sums go through LDS.
__device__ int optimize(const Sim3Rec& P, Sim3Shared& sh, Sim3& cur, int its, int nActive) {
    const int t = threadIdx.x;
    if (nActive == 0) return 0;    // no active vertex: optimize() returns at once
    int done = 0;
    double lambda = 0, ni = refc::LM_NI;
    int nBad = 0;
    for (int it = 0; it < its; it++) {
        // ---- computeActiveErrors + buildSystem (numeric linearisation)
        if (t < 14) {
            double u[7] = {0, 0, 0, 0, 0, 0, 0};
            const int d = t >> 1;
#pragma unroll
            for (int k = 0; k < 7; k++) if (k == d) u[k] = (t & 1) ? -kSim3Delta : kSim3Delta;
            if (P.fix_scale) u[6] = 0;
            const Sim3 Sp = sim3_mul(sim3_exp(u), cur);
            sh.pert[t] = Sp;
            sh.pertInv[t] = sim3_inverse(Sp);
        } else if (t == 14) {
            sh.curS[0] = cur;
        } else if (t == 15) {
            sh.curS[1] = sim3_inverse(cur);
        }
        __syncthreads();
        linearize(P, sh);
        cur = sh.curS[0];     // the same value every thread holds: reloaded, so that it is not live in registers across the loop above
        // H and b stay in LDS (sh.sum) for the whole iteration: every thread reads them from there
        const double* Hp = sh.sum;            // packed upper triangle, row by row
        const double* bv = sh.sum + 28;
        double currentChi = sh.sum[35];
        const double iniChi = currentChi;
        if (it == 0) {   // computeLambdaInit, _ni = 2, _nBad = 0
            double maxDiag = 0;
            for (int a = 0, k = 0; a < 7; k += 7 - a, a++) maxDiag = fmax(fabs(Hp[k]), maxDiag);
            lambda = refc::LM_TAU * maxDiag;
            ni = refc::LM_NI;
            nBad = 0;
        }
        // ---- the trials
        int qmax = 0;
        double rho = 0;
        for (;;) {
            double x[7];
            const bool ok = ldlt7_solve(Hp, lambda, bv, x);
            if (!ok) for (int a = 0; a < 7; a++) x[a] = 0;
            if (P.fix_scale) x[6] = 0;     // oplusImpl zeroes the solver's own x[6]
            const Sim3 trial = sim3_mul(sim3_exp(x), cur);
            double tempChi = evaluate(P, sh, trial, sim3_inverse(trial));
            if (!ok) tempChi = DBL_MAX;
            rho = currentChi - tempChi;
            double scale = 0;
            for (int a = 0; a < 7; a++) scale += x[a] * (lambda * x[a] + bv[a]);
            scale += 1e-3;
            rho /= scale;
            if (rho > 0 && isfinite(tempChi)) {
                double alpha = 1. - pow((2 * rho - 1), 3);
                alpha = fmin(alpha, 2. / 3.);
                const double scaleFactor = fmax(1. / 3., alpha);
                lambda *= scaleFactor;
                ni = refc::LM_NI;
                currentChi = tempChi;
                cur = trial;
            } else {
                lambda *= ni;
                ni *= 2;
            }
            qmax++;
            if (!(rho < 0 && qmax < refc::LM_MAX_TRIALS)) break;
        }
        done++;
        if (qmax == refc::LM_MAX_TRIALS || rho == 0) break;
        if ((iniChi - currentChi) * 1e3 < iniChi) nBad++;
        else nBad = 0;
        if (nBad >= 3) break;
    }
    return done;
}

// inlier pass over the active edges with the stale gate flags: marks the failures removed, returns {bad, good} summed
__device__ void inlier_pass(const Sim3Rec& P, Sim3Shared& sh, double& nBadOut, double& nGoodOut) {
    double acc[2] = {0, 0};
    for (int m = threadIdx.x; m < P.n; m += kSim3Threads) {
        if (P.removed[m]) continue;
        if (P.lastbad[m]) { P.removed[m] = 1; acc[0] += 1; }     // (each correspondence is visited by one thread only)
        else acc[1] += 1;
    }
    wg_sum<2>(acc, sh.red, sh.sum);
    nBadOut = sh.sum[0]; nGoodOut = sh.sum[1];
}

__global__ __launch_bounds__(kSim3Threads) void k_optimize_sim3(const Sim3Rec* __restrict__ W) {
    __shared__ Sim3Shared sh;
    const Sim3Rec& P = W[blockIdx.x];
    for (int m = threadIdx.x; m < P.n; m += kSim3Threads) { P.removed[m] = 0; P.lastbad[m] = 0; }
    Sim3 cur = P.S0;
    __syncthreads();
    const int it0 = optimize(P, sh, cur, 5, P.n);     // optimizer.optimize(5)
    double nBad, nGood;
    inlier_pass(P, sh, nBad, nGood);
    const int nCorr = P.n, bad = (int)nBad;
    if (nCorr - bad < 10) {                      // return 0: g2oS12 is not written back
        if (threadIdx.x == 0) { P.out->S = P.S0; P.out->n_inliers = 0; P.out->iters0 = it0; P.out->iters1 = 0; P.out->early_exit = 1; }
        return;
    }
    const int it1 = optimize(P, sh, cur, bad > 0 ? 10 : 5, nCorr - bad);
    inlier_pass(P, sh, nBad, nGood);
    if (threadIdx.x == 0) { P.out->S = cur; P.out->n_inliers = (int)nGood; P.out->iters0 = it0; P.out->iters1 = it1; P.out->early_exit = 0; }
}

// ---------------------------------------------------------------------- host side
struct Sim3Ctx : ThreadStream {
    DevBuf<unsigned char> dev;
    std::vector<unsigned char> host;
    float lastMs = 0;
};
thread_local Sim3Ctx g_sim3;

// R * X accumulated in double, rounded once to float; + t in float (cv::Mat float gemm then add); then promoted
void camera_point(const float* T, const float* X, double out[3]) {
    for (int i = 0; i < 3; i++) {
        const double acc = (double)T[4 * i] * X[0] + (double)T[4 * i + 1] * X[1] + (double)T[4 * i + 2] * X[2];
        const float v = (float)acc + T[4 * i + 3];
        out[i] = v;
    }
}

eao_status check_problem(const eao_sim3_problem* p, const eao_sim3_result* r) {
    EAO_REQUIRE(p && r, "null argument");
    EAO_REQUIRE(p->n >= 0, "bad problem: n = %d", p->n);
    EAO_REQUIRE(p->n == 0 || (p->T1w && p->T2w && p->Xw1 && p->Xw2 && p->obs1 && p->obs2 && p->inv_sigma2_1 && p->inv_sigma2_2 && r->removed),
                "bad problem: missing arrays");
    EAO_REQUIRE(p->s > 0 && std::isfinite(p->s), "bad problem: scale %g", p->s);
    return EAO_OK;
}

eao_status run_sim3(const eao_sim3_problem* ps, int nb, eao_sim3_result* rs) {
    for (int b = 0; b < nb; b++) {
        eao_status st = check_problem(&ps[b], &rs[b]);
        if (st) return st;
    }
    Sim3Ctx& c = g_sim3;
    eao_status st = c.ready(StreamClass::Latency);
    if (!st) st = c.timing();
    if (st) return st;
    // layout: [records][per problem: 12 n doubles] | [outputs][per problem: removed n] | [per problem: lastbad n]
    size_t off = align256(sizeof(Sim3Rec) * nb);
    std::vector<size_t> offD(nb), offR(nb), offL(nb);
    for (int b = 0; b < nb; b++) { offD[b] = off; off = align256(off + (size_t)ps[b].n * 12 * sizeof(double)); }
    const size_t inEnd = off;
    const size_t offOut = off;
    off = align256(off + sizeof(Sim3Out) * nb);
    for (int b = 0; b < nb; b++) { offR[b] = off; off += (size_t)ps[b].n; }
    const size_t outEnd = off;
    off = align256(off);
    for (int b = 0; b < nb; b++) { offL[b] = off; off += (size_t)ps[b].n; }
    const size_t total = std::max<size_t>(off, 256);
    if ((st = c.dev.reserve(total))) return st;
    if (c.host.size() < total) c.host.resize(total);
    unsigned char* h = c.host.data();
    unsigned char* d = c.dev.p;
    Sim3Rec* recs = (Sim3Rec*)h;
    for (int b = 0; b < nb; b++) {
        const eao_sim3_problem& p = ps[b];
        const int n = p.n;
        double* X1 = (double*)(h + offD[b]);
        double* X2 = X1 + 3 * (size_t)n;
        double* o1 = X2 + 3 * (size_t)n;
        double* o2 = o1 + 2 * (size_t)n;
        double* i1 = o2 + 2 * (size_t)n;
        double* i2 = i1 + n;
        for (int i = 0; i < n; i++) {
            camera_point(p.T1w, p.Xw1 + 3 * i, X1 + 3 * i);
            camera_point(p.T2w, p.Xw2 + 3 * i, X2 + 3 * i);
            o1[2 * i] = p.obs1[2 * i]; o1[2 * i + 1] = p.obs1[2 * i + 1];
            o2[2 * i] = p.obs2[2 * i]; o2[2 * i + 1] = p.obs2[2 * i + 1];
            i1[i] = p.inv_sigma2_1[i]; i2[i] = p.inv_sigma2_2[i];
        }
        Sim3Rec& R = recs[b];
        R.n = n; R.fix_scale = p.fix_scale ? 1 : 0;
        R.th2 = p.th2;
        const float deltaHuber = std::sqrt(p.th2);      // const float deltaHuber = sqrt(th2); RobustKernelHuber::setDelta(double)
        R.delta = deltaHuber;
        R.fx1 = p.fx1; R.fy1 = p.fy1; R.cx1 = p.cx1; R.cy1 = p.cy1;
        R.fx2 = p.fx2; R.fy2 = p.fy2; R.cx2 = p.cx2; R.cy2 = p.cy2;
        const size_t dd = offD[b];
        R.X1c = (const double*)(d + dd);
        R.X2c = R.X1c + 3 * (size_t)n;
        R.o1 = R.X2c + 3 * (size_t)n;
        R.o2 = R.o1 + 2 * (size_t)n;
        R.i1 = R.o2 + 2 * (size_t)n;
        R.i2 = R.i1 + n;
        R.S0.r.x = p.q[0]; R.S0.r.y = p.q[1]; R.S0.r.z = p.q[2]; R.S0.r.w = p.q[3];
        for (int k = 0; k < 3; k++) R.S0.t[k] = p.t[k];
        R.S0.s = p.s;
        R.removed = d + offR[b];
        R.lastbad = d + offL[b];
        R.out = (Sim3Out*)(d + offOut) + b;
    }
    Drain drain(c.stream);
    EAO_HIP(hipMemcpyAsync(d, h, inEnd, hipMemcpyHostToDevice, c.stream));
    EAO_HIP(hipEventRecord(c.ev0, c.stream));
    if (nb > 0) hipLaunchKernelGGL(k_optimize_sim3, dim3(nb), dim3(kSim3Threads), 0, c.stream, (const Sim3Rec*)d);
    EAO_HIP(hipGetLastError());
    EAO_HIP(hipEventRecord(c.ev1, c.stream));
    EAO_HIP(hipMemcpyAsync(h + offOut, d + offOut, outEnd - offOut, hipMemcpyDeviceToHost, c.stream));
    EAO_HIP(drain.wait(Drain::Block));
    EAO_HIP(hipEventElapsedTime(&c.lastMs, c.ev0, c.ev1));
    g_trace.clear();
    g_trace.deviceMs = c.lastMs;
    const Sim3Out* outs = (const Sim3Out*)(h + offOut);
    for (int b = 0; b < nb; b++) {
        const Sim3Out& o = outs[b];
        eao_sim3_result& r = rs[b];
        r.q[0] = o.S.r.x; r.q[1] = o.S.r.y; r.q[2] = o.S.r.z; r.q[3] = o.S.r.w;
        for (int k = 0; k < 3; k++) r.t[k] = o.S.t[k];
        r.s = o.S.s;
        if (ps[b].n) std::memcpy(r.removed, h + offR[b], ps[b].n);
        r.n_inliers = o.n_inliers;
        r.lm_iterations[0] = o.iters0; r.lm_iterations[1] = o.iters1;
        r.early_exit = o.early_exit;
        g_trace.linearizations += o.iters0 + o.iters1;
    }
    return EAO_OK;
}

}  // namespace

extern "C" {

eao_status eao_optimize_sim3(const eao_sim3_problem* p, eao_sim3_result* r) {
    EAO_REQUIRE(p && r, "null argument");
    return run_sim3(p, 1, r);
}

eao_status eao_optimize_sim3_batch(const eao_sim3_problem* problems, int32_t n, eao_sim3_result* results) {
    EAO_REQUIRE(n >= 0 && (n == 0 || (problems && results)), "bad batch");
    if (n == 0) return EAO_OK;
    return run_sim3(problems, n, results);
}

}  // extern "C"
