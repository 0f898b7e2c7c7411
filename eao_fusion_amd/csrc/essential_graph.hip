// essential_graph.hip -- Optimizer::OptimizeEssentialGraph (reference src/Optimizer.cc:1141-1435): the Sim3 pose graph LoopClosing::CorrectLoop
// (src/LoopClosing.cc:584) runs between OptimizeSim3 and the global bundle adjustment.
//
// One free 7-dof vertex (VertexSim3Expmap) per keyframe with an edge, the loop keyframe fixed; binary EdgeSim3 edges, information = identity, no robust
// kernel; optimize(20) of Levenberg-Marquardt with lambda0 = 1e-16.  No vertex is marginalised: the whole system is Hpp, 7 x 7 blocks on the pattern of the edges.
//
// g2o details reproduced (Thirdparty/g2o/g2o):
//  - types/sim3.h:148-230  Sim3::log: sigma = log(s), R = toRotationMatrix() (not renormalised), d = (trace - 1) / 2, four branches on |sigma| < 1e-5 and
//    d > 1 - 1e-5, acos(d), upsilon = W.lu().solve(t) -- a 3 x 3 partial-pivot LU -- with the coefficients A, B, C written as upstream writes them.
//  - types_seven_dof_expmap.h:114-122  EdgeSim3::computeError = (C * v0 * v1^-1).log(); :48-72 oplusImpl: S <- Sim3(update) * S, update[6] = 0 under
//    _fix_scale (in the solver's own x, which computeScale reads afterwards).
//  - core/base_binary_edge.hpp:147-196  no analytic Jacobian: central differences with delta = 1e-9 on every free vertex; under _fix_scale the 7th column is
//    exactly zero, so every scale row of H is 0 + lambda and its right-hand side 0.
//  - core/optimization_algorithm_levenberg.cpp:61-189  setUserLambdaInit(1e-16): lambda0 = 1e-16; rho with the +1e-3 scale, nu doubling, at most 10 trials per
//    iteration; a failed solve rejects the trial (tempChi = DBL_MAX); optimize(20) stops on qmax == 10, rho == 0 or three iterations below 0.1 % gain.
//  - solvers/linear_solver_eigen.h:95-125  SimplicialLDLT fails on an exactly zero pivot only: so does the factor chain here (a pivot of 1e-16 is legitimate).
//
// Kernels (one stream, nothing waits for the host inside a batch of trials):
//   k_eg_measure     the edges' measurements S_ji, once
//   k_eg_linearize   per iteration: (edge, evaluation) over lanes -- the base error and +-delta on the 7 components of either vertex, 29 evaluations of two products,
//                    an inverse and a log each; Ji, Jj (7 x 7) and e per edge
//   k_eg_assemble    per iteration: one wavefront per block of H (diagonal blocks and the pairs with an edge), a gather over a host-built CSR in edge order; b with
//                    the diagonal blocks.  No floating-point atomics anywhere: the same call returns the same bytes.
//   k_eg_begin       per iteration: chi2 in a fixed order, lambda0 on the first
//   k_eg_scatter     per trial: H + lambda I, the right-hand side row and the identity padding into the 64 x 64 tiles of the map-scale factor chain
//   (gba.hip)        k_bal_diag / k_bal_step / k_bal_linv / k_bal_backsolve on a plan built with block width 7 (gba_build_plan)
//   k_eg_apply       per trial: exp(dx) * S into the other state buffer
//   k_eg_errors      per trial: the edges' chi2 at the trial state
//   k_eg_decide      per trial: the sums in a fixed order, accept / reject / stop; the trace and the verdict land in pinned host memory
//   k_eg_finish      Tiw and the map points
// Every kernel behind the first returns at once when the halt flag is set, k_eg_linearize / k_eg_assemble / k_eg_begin also when the last trial did not end an
// iteration; the host enqueues kEgSlots trials at a time and looks at the pinned verdict between the batches.
#include "sim3_internal.h"

using namespace eao;
using namespace eao::lm;

namespace {

constexpr double kEgDelta = 1e-9;                 // core/base_binary_edge.hpp:147
constexpr double kEgLambdaInit = 1e-16;           // src/Optimizer.cc:1154
constexpr int kEgMaxIterations = 20;              // src/Optimizer.cc:1348
constexpr int kEgSlots = 6;                       // trials enqueued between two looks at the verdict
constexpr int kEgEvals = 29;

struct EgState { double lambda, ni, currentChi, iniChi, rho; int iters, qmax, nBad, needLin; };
struct EgStatus {            // pinned host memory, written by k_eg_begin / k_eg_decide
    int done, iters, pad0, pad1;
    double chi0;
    int trials[kEgMaxIterations];
    double lambda[kEgMaxIterations], chi2[kEgMaxIterations];
};

struct EgDev {               // what the kernels take by value; every pointer a device address (status: pinned)
    int n, nf, m, fixScale, nBlocks, nPts, N;
    const int* ei; const int* ej; const int* kind; const unsigned char* hasNc;
    const Sim3* Sin; const Sim3* Snc;
    Sim3* S[2];
    Sim3* C;
    const int* blk;          // n: free block of a vertex, -1 for the fixed one and those without an edge
    const int* freeV;        // nf: vertex of a block
    const int* rowOf;        // nf: first row of a block in the elimination order
    const int* rowCam;       // N: natural index of a row's unknown, -1 for padding
    double* e; double* Ji; double* Jj; double* echi;
    const int* blkStart;     // nBlocks + 1: the blocks of H -- nf diagonal ones, then the pairs -- and the edges that add to each, in edge order
    const int* blkItem;      // edge << 1 | role.  diagonal: role 0 = the block's vertex is vertex 0 of the edge; pair: role 0 = the block's row vertex is vertex 0
    const int2* blkRC;       // nBlocks: (row block, column block), the row block further down in the elimination order
    double* Hblk; double* bvec;
    const BADev* W;          // the record the factor chain reads (big*, xp, ctl)
    int* ctl; EgState* st; EgStatus* status;
    const float* Xw; const int* ref;
    double* outS; float* outT; float* outX;
};

// ---------------------------------------------------------------------- Sim3::log (types/sim3.h:148-230)
__device__ inline void lu3_solve(double A[9], const double b[3], double x[3]) {      // Eigen's PartialPivLU of a 3 x 3: the column's largest |entry|, the first on a tie
    double y[3] = {b[0], b[1], b[2]};
#pragma unroll
    for (int k = 0; k < 2; k++) {
        int p = k;
        double best = fabs(A[k * 3 + k]);
#pragma unroll
        for (int i = k + 1; i < 3; i++) if (fabs(A[i * 3 + k]) > best) { best = fabs(A[i * 3 + k]); p = i; }
#pragma unroll
        for (int i = k + 1; i < 3; i++)
            if (p == i) {
#pragma unroll
                for (int c = 0; c < 3; c++) { const double tmp = A[k * 3 + c]; A[k * 3 + c] = A[i * 3 + c]; A[i * 3 + c] = tmp; }
                const double tmp = y[k]; y[k] = y[i]; y[i] = tmp;
            }
#pragma unroll
        for (int i = k + 1; i < 3; i++) {
            const double l = A[i * 3 + k] / A[k * 3 + k];
#pragma unroll
            for (int c = k + 1; c < 3; c++) A[i * 3 + c] = A[i * 3 + c] - l * A[k * 3 + c];
            y[i] = y[i] - l * y[k];
        }
    }
    x[2] = y[2] / A[8];
    x[1] = (y[1] - A[5] * x[2]) / A[4];
    x[0] = (y[0] - A[1] * x[1] - A[2] * x[2]) / A[0];
}

__device__ inline void sim3_log(const Sim3& S, double res[7]) {
    const double s = S.s;
    const double sigma = log(s);
    double R[9];
    quat_to_matrix(S.r, R);
    const double d = 0.5 * (R[0] + R[4] + R[8] - 1);
    const double dR[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};
    double omega[3], A, B, C;
    if (fabs(sigma) < kSim3Eps) {
        C = 1;
        if (d > 1 - kSim3Eps) {
            for (int i = 0; i < 3; i++) omega[i] = 0.5 * dR[i];
            A = 1. / 2.; B = 1. / 6.;
        } else {
            const double theta = acos(d), theta2 = theta * theta;
            const double f = theta / (2 * sqrt(1 - d * d));
            for (int i = 0; i < 3; i++) omega[i] = f * dR[i];
            A = (1 - cos(theta)) / theta2;
            B = (theta - sin(theta)) / (theta2 * theta);
        }
    } else {
        C = (s - 1) / sigma;
        if (d > 1 - kSim3Eps) {
            const double sigma2 = sigma * sigma;
            for (int i = 0; i < 3; i++) omega[i] = 0.5 * dR[i];
            A = ((sigma - 1) * s + 1) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma);
        } else {
            const double theta = acos(d);
            const double f = theta / (2 * sqrt(1 - d * d));
            for (int i = 0; i < 3; i++) omega[i] = f * dR[i];
            const double theta2 = theta * theta;
            const double a = s * sin(theta), b = s * cos(theta), c = theta2 + sigma * sigma;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / theta2;
        }
    }
    const double Om[9] = {0, -omega[2], omega[1], omega[2], 0, -omega[0], -omega[1], omega[0], 0};
    double W[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            const double om2 = Om[i * 3] * Om[j] + Om[i * 3 + 1] * Om[3 + j] + Om[i * 3 + 2] * Om[6 + j];
            W[i * 3 + j] = A * Om[i * 3 + j] + B * om2 + (i == j ? C : 0.0);
        }
    double ups[3];
    lu3_solve(W, S.t, ups);
    for (int i = 0; i < 3; i++) { res[i] = omega[i]; res[i + 3] = ups[i]; }
    res[6] = sigma;
}

// EdgeSim3::computeError: (C * v0 * v1^-1).log()
__device__ __forceinline__ void edge_error(const Sim3& C, const Sim3& Si, const Sim3& Sj, double err[7]) {
    sim3_log(sim3_mul(sim3_mul(C, Si), sim3_inverse(Sj)), err);
}

__device__ __forceinline__ double dot7(const double e[7]) {
    double c = 0;
#pragma unroll
    for (int k = 0; k < 7; k++) c += e[k] * e[k];
    return c;
}

// sum of v[0 .. cnt) by the 256 threads of a workgroup in a fixed order: a strided sum per thread, then a tree through LDS; valid in every thread
__device__ inline double wg_sum_fixed(const double* v, int cnt, double* lds /* 256 */) {
    double acc = 0;
    for (int i = threadIdx.x; i < cnt; i += 256) acc += v[i];
    __syncthreads();
    lds[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) lds[threadIdx.x] += lds[threadIdx.x + s];
        __syncthreads();
    }
    return lds[0];
}

// ---------------------------------------------------------------------- kernels
__global__ __launch_bounds__(256) void k_eg_measure(EgDev D) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= D.m) return;
    const int i = D.ei[k], j = D.ej[k];
    const bool normal = D.kind[k] == 1;
    const Sim3 Siw = normal && D.hasNc[i] ? D.Snc[i] : D.Sin[i];
    const Sim3 Sjw = normal && D.hasNc[j] ? D.Snc[j] : D.Sin[j];
    D.C[k] = sim3_mul(Sjw, sim3_inverse(Siw));
}

// 8 edges per workgroup, 32 lanes each: lane 0 the base error, 1..14 vertex 0 at +-delta e_d, 15..28 vertex 1
__global__ __launch_bounds__(256) void k_eg_linearize(EgDev D) {
    __shared__ Sim3 pert[14];
    __shared__ double ev[8][kEgEvals][7];
    if (D.ctl[kCtlHalt] || !D.st->needLin) return;
    const int t = threadIdx.x, p = t & 31, slot = t >> 5, k = blockIdx.x * 8 + slot;
    if (t < 14) {      // Sim3(+-delta e_d): [2d] = +delta, [2d + 1] = -delta, the 7th entry zeroed under _fix_scale
        double u[7] = {0, 0, 0, 0, 0, 0, 0};
        const int d = t >> 1;
#pragma unroll
        for (int q = 0; q < 7; q++) if (q == d) u[q] = (t & 1) ? -kEgDelta : kEgDelta;
        if (D.fixScale) u[6] = 0;
        pert[t] = sim3_exp(u);
    }
    __syncthreads();
    const Sim3* S = D.S[D.ctl[kCtlCur]];
    if (k < D.m && p < kEgEvals) {
        const int i = D.ei[k], j = D.ej[k];
        double err[7] = {0, 0, 0, 0, 0, 0, 0};
        const int v = p == 0 ? -1 : (p - 1) / 14;            // the perturbed vertex
        const bool isFree = v < 0 || D.blk[v == 0 ? i : j] >= 0;      // (a fixed vertex's Jacobian is not formed)
        if (isFree) {
            Sim3 Si = S[i], Sj = S[j];
            if (v == 0) Si = sim3_mul(pert[p - 1], Si);
            if (v == 1) Sj = sim3_mul(pert[p - 15], Sj);
            edge_error(D.C[k], Si, Sj, err);
        }
#pragma unroll
        for (int q = 0; q < 7; q++) ev[slot][p][q] = err[q];
        if (p == 0) {
#pragma unroll
            for (int q = 0; q < 7; q++) D.e[(size_t)k * 7 + q] = err[q];
            D.echi[k] = dot7(err);
        }
    }
    __syncthreads();
    if (k < D.m) {
        const double scalar = 1.0 / (2 * kEgDelta);
        for (int idx = p; idx < 98; idx += 32) {
            const int v = idx / 49, r = (idx % 49) / 7, d = idx % 7;
            const double Jrd = scalar * (ev[slot][1 + v * 14 + 2 * d][r] - ev[slot][2 + v * 14 + 2 * d][r]);
            (v ? D.Jj : D.Ji)[(size_t)k * 49 + r * 7 + d] = Jrd;
        }
    }
}

// one wavefront per block of H: lanes 0..48 its entries, 49..55 the block row of b (diagonal blocks)
__global__ __launch_bounds__(64) void k_eg_assemble(EgDev D) {
    if (D.ctl[kCtlHalt] || !D.st->needLin) return;
    const int blkI = blockIdx.x, t = threadIdx.x;
    const bool diag = blkI < D.nf;
    const int beg = D.blkStart[blkI], end = D.blkStart[blkI + 1];
    if (t < 49) {
        const int r = t / 7, c = t % 7;
        double acc = 0;
        for (int it = beg; it < end; it++) {
            const int item = D.blkItem[it], k = item >> 1, role = item & 1;
            const double* Jr = (role ? D.Jj : D.Ji) + (size_t)k * 49;                        // the row vertex's Jacobian
            const double* Jc = diag ? Jr : (role ? D.Ji : D.Jj) + (size_t)k * 49;            // the column vertex's
#pragma unroll
            for (int q = 0; q < 7; q++) acc += Jr[q * 7 + r] * Jc[q * 7 + c];
        }
        D.Hblk[(size_t)blkI * 49 + t] = acc;
    } else if (diag && t < 56) {
        const int r = t - 49;
        double acc = 0;
        for (int it = beg; it < end; it++) {
            const int item = D.blkItem[it], k = item >> 1, role = item & 1;
            const double* J = (role ? D.Jj : D.Ji) + (size_t)k * 49;
            const double* e = D.e + (size_t)k * 7;
#pragma unroll
            for (int q = 0; q < 7; q++) acc -= J[q * 7 + r] * e[q];
        }
        D.bvec[(size_t)blkI * 7 + r] = acc;
    }
}

__global__ __launch_bounds__(256) void k_eg_begin(EgDev D) {
    __shared__ double lds[256];
    if (D.ctl[kCtlHalt] || !D.st->needLin) return;
    const double chi = wg_sum_fixed(D.echi, D.m, lds);
    if (threadIdx.x == 0) {
        EgState& st = *D.st;
        st.currentChi = chi; st.iniChi = chi;
        if (st.iters == 0) { st.lambda = kEgLambdaInit; st.ni = 2; st.nBad = 0; D.status->chi0 = chi; }
        st.qmax = 0; st.rho = 0;
        st.needLin = 0;
    }
}

// H + lambda I, b and the padding into the (zeroed) working tiles, lower triangle
__global__ __launch_bounds__(64) void k_eg_scatter(EgDev D) {
    if (D.ctl[kCtlHalt]) return;
    const BADev& P = *D.W;
    const int blkI = blockIdx.x, t = threadIdx.x, N = D.N;
    if (blkI == 0) {
        if (t == 0) *P.bigFail = 0;
        for (int r = t; r < N; r += 64) if (D.rowCam[r] < 0) *big_elem(P, P.big, r, r) = 1.0;
    }
    const int2 rc = D.blkRC[blkI];
    const int R1 = D.rowOf[rc.x], R2 = D.rowOf[rc.y];
    if (t < 49) {
        const int r = t / 7, c = t % 7;
        const double h = D.Hblk[(size_t)blkI * 49 + t];
        if (blkI >= D.nf) *big_elem(P, P.big, R1 + r, R2 + c) = h;
        else if (c <= r) *big_elem(P, P.big, R1 + r, R1 + c) = h + (r == c ? D.st->lambda : 0.0);
    } else if (blkI < D.nf && t < 56) {
        const int r = t - 49;
        *big_elem(P, P.big, N, R1 + r) = D.bvec[(size_t)blkI * 7 + r];
    }
}

__global__ __launch_bounds__(256) void k_eg_apply(EgDev D) {
    if (D.ctl[kCtlHalt]) return;
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= D.nf) return;
    const int cur = D.ctl[kCtlCur], v = D.freeV[b];
    double* xp = D.W->xp;
    if (D.fixScale) xp[(size_t)b * 7 + 6] = 0;      // oplusImpl zeroes the solver's own x[6]
    double u[7];
#pragma unroll
    for (int q = 0; q < 7; q++) u[q] = xp[(size_t)b * 7 + q];
    D.S[cur ^ 1][v] = sim3_mul(sim3_exp(u), D.S[cur][v]);
}

__global__ __launch_bounds__(256) void k_eg_errors(EgDev D) {
    if (D.ctl[kCtlHalt]) return;
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= D.m) return;
    const Sim3* S = D.S[D.ctl[kCtlCur] ^ 1];
    double err[7];
    edge_error(D.C[k], S[D.ei[k]], S[D.ej[k]], err);
    D.echi[k] = dot7(err);
}

__global__ __launch_bounds__(256) void k_eg_decide(EgDev D) {
    __shared__ double lds[256];
    if (D.ctl[kCtlHalt]) return;
    EgState& st = *D.st;
    const double lambda = st.lambda;
    double tempChi = wg_sum_fixed(D.echi, D.m, lds);
    // computeScale: sum of x (lambda x + b), the terms in natural order through the same fixed-order sum (the products land in Hblk's first entries' place: a scratch)
    double acc = 0;
    const double* xp = D.W->xp;
    for (int i = threadIdx.x; i < D.nf * 7; i += 256) acc += xp[i] * (lambda * xp[i] + D.bvec[i]);
    __syncthreads();
    lds[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) lds[threadIdx.x] += lds[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    double scale = lds[0];
    if (*D.W->bigFail) tempChi = DBL_MAX;      // a failed solve rejects the trial
    double rho = st.currentChi - tempChi;
    scale += 1e-3;
    rho /= scale;
    if (rho > 0 && isfinite(tempChi)) {
        double alpha = 1. - pow((2 * rho - 1), 3);
        alpha = fmin(alpha, 2. / 3.);
        st.lambda = lambda * fmax(1. / 3., alpha);
        st.ni = 2;
        st.currentChi = tempChi;
        D.ctl[kCtlCur] ^= 1;
    } else {
        st.lambda = lambda * st.ni;
        st.ni *= 2;
    }
    st.rho = rho;
    st.qmax++;
    if (rho < 0 && st.qmax < refc::LM_MAX_TRIALS) return;      // another trial of this iteration
    EgStatus& out = *D.status;
    out.trials[st.iters] = st.qmax; out.lambda[st.iters] = st.lambda; out.chi2[st.iters] = st.currentChi;
    st.iters++;
    bool stop = st.qmax == refc::LM_MAX_TRIALS || rho == 0;
    if (!stop) {
        if ((st.iniChi - st.currentChi) * 1e3 < st.iniChi) st.nBad++;
        else st.nBad = 0;
        stop = st.nBad >= 3;
    }
    if (st.iters >= kEgMaxIterations) stop = true;
    if (stop) {
        D.ctl[kCtlHalt] = 1;
        out.iters = st.iters;
        __threadfence_system();
        out.done = 1;
    } else {
        st.needLin = 1;
    }
}

// the vertices as they stand, Tiw = [R | t / s], the map points through the inverse of their reference keyframe's optimised Sim3
__global__ __launch_bounds__(256) void k_eg_finish(EgDev D) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    const Sim3* S = D.S[D.ctl[kCtlCur]];
    if (g < D.n) {
        const Sim3 s = D.blk[g] >= 0 ? S[g] : D.Sin[g];
        double* o = D.outS + (size_t)g * 8;
        o[0] = s.r.x; o[1] = s.r.y; o[2] = s.r.z; o[3] = s.r.w; o[4] = s.t[0]; o[5] = s.t[1]; o[6] = s.t[2]; o[7] = s.s;
        double R[9];
        quat_to_matrix(s.r, R);
        const double is = 1. / s.s;
        float* T = D.outT + (size_t)g * 16;
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) T[i * 4 + j] = (float)R[i * 3 + j];
            T[i * 4 + 3] = (float)(s.t[i] * is);
        }
        T[12] = T[13] = T[14] = 0.f; T[15] = 1.f;
    }
    const int pI = g - D.n;
    if (pI >= 0 && pI < D.nPts) {
        const int r = D.ref[pI];
        const float* X = D.Xw + (size_t)pI * 3;
        float* o = D.outX + (size_t)pI * 3;
        if (r < 0) { o[0] = X[0]; o[1] = X[1]; o[2] = X[2]; return; }
        const Sim3 Srw = D.Sin[r];
        const Sim3 Swr = sim3_inverse(D.blk[r] >= 0 ? S[r] : D.Sin[r]);
        const double x[3] = {X[0], X[1], X[2]};
        double a[3], b[3], c[3], d[3];
        quat_rotate(Srw.r, x, a);
        for (int q = 0; q < 3; q++) b[q] = Srw.s * a[q] + Srw.t[q];
        quat_rotate(Swr.r, b, c);
        for (int q = 0; q < 3; q++) d[q] = Swr.s * c[q] + Swr.t[q];
        o[0] = (float)d[0]; o[1] = (float)d[1]; o[2] = (float)d[2];
    }
}

// ---------------------------------------------------------------------- host side
struct EgCtx : ThreadStream {      // per host thread, grow-only; the stream class of the map bundle adjustment (LoopClosing's thread)
    EgStatus* status = nullptr;      // pinned + mapped
    DevBuf<unsigned char> dev;
    std::vector<unsigned char> host;
    GbaPlan plan;
    ~EgCtx() { if (status) (void)hipHostFree(status); }
};
thread_local EgCtx g_eg;

bool finite_rows(const double* a, size_t cnt) {
    for (size_t i = 0; i < cnt; i++) if (!std::isfinite(a[i])) return false;
    return true;
}

eao_status eg_check(const eao_essential_graph_problem* p, const eao_essential_graph_result* r) {
    EAO_REQUIRE(p && r, "null argument");
    EAO_REQUIRE(p->n >= 1 && p->n_edges >= 0 && p->n_points >= 0, "bad problem: n = %d, n_edges = %d, n_points = %d", p->n, p->n_edges, p->n_points);
    EAO_REQUIRE(p->Scw && p->has_nc && p->Snc && r->Scw && r->Tiw, "bad problem: missing keyframe arrays");
    EAO_REQUIRE(p->n_edges == 0 || p->edges, "bad problem: missing edges");
    EAO_REQUIRE(p->n_points == 0 || (p->Xw && p->ref && r->Xw_corrected), "bad problem: missing point arrays");
    EAO_REQUIRE(p->fixed >= 0 && p->fixed < p->n, "bad problem: fixed = %d is not a keyframe index (n = %d)", p->fixed, p->n);
    EAO_REQUIRE(finite_rows(p->Scw, (size_t)p->n * 8), "bad problem: non-finite Scw");
    for (int i = 0; i < p->n; i++) {
        EAO_REQUIRE(p->Scw[(size_t)i * 8 + 7] > 0, "bad problem: keyframe %d has scale %g", i, p->Scw[(size_t)i * 8 + 7]);
        if (p->has_nc[i]) EAO_REQUIRE(finite_rows(p->Snc + (size_t)i * 8, 8) && p->Snc[(size_t)i * 8 + 7] > 0, "bad problem: non-finite Snc of keyframe %d", i);
    }
    for (int k = 0; k < p->n_edges; k++) {
        const int i = p->edges[3 * k], j = p->edges[3 * k + 1], kind = p->edges[3 * k + 2];
        EAO_REQUIRE(i >= 0 && i < p->n && j >= 0 && j < p->n, "bad problem: edge %d links (%d, %d), n = %d", k, i, j, p->n);
        EAO_REQUIRE(i != j, "bad problem: edge %d links keyframe %d to itself", k, i);
        EAO_REQUIRE(kind == 0 || kind == 1, "bad problem: edge %d has kind %d", k, kind);
    }
    for (int k = 0; k < p->n_points; k++) {
        EAO_REQUIRE(std::isfinite(p->Xw[3 * (size_t)k]) && std::isfinite(p->Xw[3 * (size_t)k + 1]) && std::isfinite(p->Xw[3 * (size_t)k + 2]), "bad problem: non-finite map point %d", k);
        EAO_REQUIRE(p->ref[k] >= -1 && p->ref[k] < p->n, "bad problem: map point %d references keyframe %d, n = %d", k, p->ref[k], p->n);
    }
    return EAO_OK;
}

inline void row_to_sim3(const double* a, Sim3& S) {
    S.r.x = a[0]; S.r.y = a[1]; S.r.z = a[2]; S.r.w = a[3];
    S.t[0] = a[4]; S.t[1] = a[5]; S.t[2] = a[6]; S.s = a[7];
}

// The structure of a checked problem: the active free vertices (ascending), the blocks of H with the edges that add to each, and the elimination plan.
struct EgStructure {
    int nf = 0, nActive = 0, nPairs = 0, nBlocks = 0;
    std::vector<int> blk, freeV;                  // vertex -> free block or -1; block -> vertex
    std::vector<int> blkStart, blkItem;
    std::vector<int2> blkRC;
};

// pl: the plan of the pattern (built when the context's does not fit it).  The pattern handed to gba_build_plan holds every vertex's own pair (v, v) besides the
// pairs with an edge: a 7-row block can straddle a 64-row tile boundary, and only a listed pair makes the tiles of a block live -- the tile below the diagonal
// that such a vertex's own block reaches into is otherwise live only if an edge or the fill-in happens to reach it.
eao_status eg_structure(const eao_essential_graph_problem* p, EgStructure& g, GbaPlan& pl) {
    const int n = p->n, m = p->n_edges;
    g.blk.assign((size_t)n, -1);
    {
        std::vector<unsigned char> act((size_t)n, 0);
        for (int k = 0; k < m; k++) { act[p->edges[3 * k]] = 1; act[p->edges[3 * k + 1]] = 1; }
        for (int v = 0; v < n; v++) {
            g.nActive += act[v];
            if (act[v] && v != p->fixed) { g.blk[v] = (int)g.freeV.size(); g.freeV.push_back(v); }
        }
    }
    const int nf = g.nf = (int)g.freeV.size();
    EAO_REQUIRE(nf <= kBigMaxFree, "at most %d free keyframes with an edge in this build (got %d)", kBigMaxFree, nf);
    std::vector<int> prA, prB;                             // unique pairs a < b of free blocks with an edge
    std::vector<std::pair<long long, int>> pairItems;      // (pair key, edge): sorted by key, edge order inside a key
    for (int k = 0; k < m; k++) {
        const int a = g.blk[p->edges[3 * k]], b = g.blk[p->edges[3 * k + 1]];
        if (a < 0 || b < 0) continue;
        pairItems.push_back({(long long)std::min(a, b) * nf + std::max(a, b), k});
    }
    std::stable_sort(pairItems.begin(), pairItems.end(), [](const std::pair<long long, int>& x, const std::pair<long long, int>& y) { return x.first < y.first; });
    for (size_t q = 0; q < pairItems.size(); q++)
        if (q == 0 || pairItems[q].first != pairItems[q - 1].first) { prA.push_back((int)(pairItems[q].first / nf)); prB.push_back((int)(pairItems[q].first % nf)); }
    if (nf > 0) {
        std::vector<int> patA(prA), patB(prB);
        for (int v = 0; v < nf; v++) { patA.push_back(v); patB.push_back(v); }
        const uint64_t key = gba_pattern_hash(nf, patA, patB) ^ 0x7777000000000000ull;
        if (!pl.valid || pl.key != key || pl.nFa != nf) { gba_build_plan(nf, patA, patB, 0, pl, 7); pl.key = key; pl.valid = true; }
    }
    g.nPairs = (int)prA.size(); g.nBlocks = nf + g.nPairs;
    g.blkStart.assign((size_t)g.nBlocks + 1, 0);
    g.blkRC.resize((size_t)std::max(g.nBlocks, 1));
    std::vector<std::vector<int>> diagItems((size_t)nf);
    for (int k = 0; k < m; k++) {
        const int a = g.blk[p->edges[3 * k]], b = g.blk[p->edges[3 * k + 1]];
        if (a >= 0) diagItems[a].push_back(k << 1);
        if (b >= 0) diagItems[b].push_back(k << 1 | 1);
    }
    for (int v = 0; v < nf; v++) {
        g.blkRC[v] = make_int2(v, v);
        g.blkItem.insert(g.blkItem.end(), diagItems[v].begin(), diagItems[v].end());
        g.blkStart[v + 1] = (int)g.blkItem.size();
    }
    int q = 0;
    for (int pi = 0; pi < g.nPairs; pi++) {
        const int a = prA[pi], b = prB[pi];
        const int row = pl.rowOf[a] > pl.rowOf[b] ? a : b, col = row == a ? b : a;
        g.blkRC[nf + pi] = make_int2(row, col);
        for (; q < (int)pairItems.size() && pairItems[q].first == (long long)a * nf + b; q++) {
            const int k = pairItems[q].second;
            g.blkItem.push_back(k << 1 | (g.blk[p->edges[3 * k]] == row ? 0 : 1));
        }
        g.blkStart[nf + pi + 1] = (int)g.blkItem.size();
    }
    return EAO_OK;
}

// The call's arena: [uploaded part][scratch, zeroed per call][results].  lay() places every slice behind `base`; it runs once on a null base for the sizes.
struct EgLayout {
    EgDev D{};
    BADev* W = nullptr;
    int* tileMap = nullptr; int4* work = nullptr; int4* sb = nullptr; int* diagList = nullptr;      // the plan's tables
    double *xp = nullptr, *big = nullptr, *bigL = nullptr, *bigDiag = nullptr, *bigLinv = nullptr;  // the factor chain's pools
    int* bigFail = nullptr;
    size_t upEnd = 0, scratchEnd = 0, outOff = 0, outEnd = 0;
    void lay(unsigned char* base, int n, int m, int nPts, const EgStructure& g, const GbaPlan* pl) {
        Arena a{base, 0};
        const int nf = g.nf, N = pl ? pl->N : 0, m1 = std::max(m, 1), p1 = std::max(nPts, 1), f1 = std::max(nf, 1), b1 = std::max(g.nBlocks, 1);
        W = a.take<BADev>(1);
        D.st = a.take<EgState>(1);
        D.ctl = a.take<int>(8);
        D.ei = a.take<int>(m1); D.ej = a.take<int>(m1); D.kind = a.take<int>(m1);
        D.hasNc = a.take<unsigned char>(n);
        D.Sin = a.take<Sim3>(n); D.Snc = a.take<Sim3>(n);
        D.S[0] = a.take<Sim3>(n); D.S[1] = a.take<Sim3>(n);
        D.blk = a.take<int>(n); D.freeV = a.take<int>(f1); D.rowOf = a.take<int>(f1); D.rowCam = a.take<int>(std::max(N, 1));
        D.blkStart = a.take<int>(g.nBlocks + 1); D.blkItem = a.take<int>(std::max<size_t>(g.blkItem.size(), 1)); D.blkRC = a.take<int2>(b1);
        D.Xw = a.take<float>((size_t)p1 * 3); D.ref = a.take<int>(p1);
        tileMap = a.take<int>(pl ? pl->tileMap.size() : 1);
        work = a.take<int4>(pl ? std::max<size_t>(pl->work.size(), 1) : 1);
        sb = a.take<int4>(pl ? std::max<size_t>(pl->sb.size(), 1) : 1);
        diagList = a.take<int>(pl ? std::max<size_t>(pl->diagList.size(), 1) : 1);
        upEnd = align256(a.off);
        D.C = a.take<Sim3>(m1);
        D.e = a.take<double>((size_t)m1 * 7); D.Ji = a.take<double>((size_t)m1 * 49); D.Jj = a.take<double>((size_t)m1 * 49); D.echi = a.take<double>(m1);
        D.Hblk = a.take<double>((size_t)b1 * 49); D.bvec = a.take<double>((size_t)f1 * 7);
        xp = a.take<double>((size_t)f1 * 7);
        const size_t tiles = pl ? (size_t)pl->bigTiles : 0;
        big = a.take<double>(std::max<size_t>(tiles << 12, 8));
        bigL = a.take<double>(std::max<size_t>(tiles << 12, 8));
        bigDiag = a.take<double>(std::max<size_t>((size_t)N * kBigNB, 8));
        bigLinv = a.take<double>(std::max<size_t>((size_t)N * kBigNB, 8));
        bigFail = a.take<int>(4);
        scratchEnd = align256(a.off);
        D.outS = a.take<double>((size_t)n * 8);
        outOff = (size_t)((unsigned char*)D.outS - base);
        D.outT = a.take<float>((size_t)n * 16); D.outX = a.take<float>((size_t)p1 * 3);
        outEnd = a.off;
    }
};

eao_status run_essential_graph(const eao_essential_graph_problem* p, eao_essential_graph_result* r) {
    eao_status st = eg_check(p, r);
    if (st) return st;
    const int n = p->n, m = p->n_edges, nPts = p->n_points;
    EgCtx& c = g_eg;
    EgStructure g;
    GbaPlan& pl = c.plan;
    if ((st = eg_structure(p, g, pl))) return st;      // (the capacity error included: before the device is touched and before anything is written)
    const int nf = g.nf, nBlocks = g.nBlocks;
    if ((st = c.ready(StreamClass::Bulk)) || (st = c.timing())) return st;
    if (!c.status) EAO_HIP(hipHostMalloc((void**)&c.status, sizeof(EgStatus), hipHostMallocMapped));
    if ((st = gba_attributes())) return st;
    const bool solve = nf > 0 && m > 0;
    const int N = solve ? pl.N : 0;
    EgLayout L;
    L.lay(nullptr, n, m, nPts, g, solve ? &pl : nullptr);      // sizes only
    const size_t total = L.outEnd + 256;
    if ((st = c.dev.reserve(total))) return st;
    if (c.host.size() < total) c.host.resize(total);
    unsigned char* h = c.host.data();
    unsigned char* d = c.dev.p;
    L.lay(d, n, m, nPts, g, solve ? &pl : nullptr);
    EgDev& D = L.D;
    const size_t upEnd = L.upEnd, outOff = L.outOff;
    auto hostp = [&](const void* devp) { return h + ((const unsigned char*)devp - d); };
    D.n = n; D.nf = nf; D.m = m; D.fixScale = p->fix_scale ? 1 : 0; D.nBlocks = nBlocks; D.nPts = nPts; D.N = N;
    D.W = L.W; D.status = c.status;
    std::memset(h, 0, upEnd);
    {
        int* ei = (int*)hostp(D.ei); int* ej = (int*)hostp(D.ej); int* kind = (int*)hostp(D.kind);
        for (int k = 0; k < m; k++) { ei[k] = p->edges[3 * k]; ej[k] = p->edges[3 * k + 1]; kind[k] = p->edges[3 * k + 2]; }
        unsigned char* has = hostp(D.hasNc);
        Sim3* Sin = (Sim3*)hostp(D.Sin); Sim3* Snc = (Sim3*)hostp(D.Snc); Sim3* S0 = (Sim3*)hostp(D.S[0]); Sim3* S1 = (Sim3*)hostp(D.S[1]);
        for (int v = 0; v < n; v++) {
            has[v] = p->has_nc[v] ? 1 : 0;
            row_to_sim3(p->Scw + (size_t)v * 8, Sin[v]);
            if (has[v]) row_to_sim3(p->Snc + (size_t)v * 8, Snc[v]); else Snc[v] = Sin[v];
            S0[v] = Sin[v]; S1[v] = Sin[v];
        }
        std::memcpy(hostp(D.blk), g.blk.data(), (size_t)n * 4);
        if (nf) std::memcpy(hostp(D.freeV), g.freeV.data(), (size_t)nf * 4);
        std::memcpy(hostp(D.blkStart), g.blkStart.data(), g.blkStart.size() * 4);
        if (!g.blkItem.empty()) std::memcpy(hostp(D.blkItem), g.blkItem.data(), g.blkItem.size() * 4);
        if (nBlocks) std::memcpy(hostp(D.blkRC), g.blkRC.data(), (size_t)nBlocks * sizeof(int2));
        if (nPts) { std::memcpy(hostp(D.Xw), p->Xw, (size_t)nPts * 12); std::memcpy(hostp(D.ref), p->ref, (size_t)nPts * 4); }
        ((EgState*)hostp(D.st))->needLin = 1;
        // the record of the factor chain: only what k_bal_diag / k_bal_step / k_bal_linv / k_bal_backsolve read
        BADev& W = *(BADev*)hostp(L.W);
        W.ctl = D.ctl; W.xp = L.xp;
        W.big = L.big; W.bigL = L.bigL; W.bigDiag = L.bigDiag; W.bigLinv = L.bigLinv; W.bigFail = L.bigFail;
        W.bigTile = L.tileMap; W.bigWork = L.work; W.bigSB = L.sb; W.bigDiagList = L.diagList; W.bigRowCam = D.rowCam; W.bigRow = D.rowOf;
        if (solve) {
            W.bigT = pl.T; W.bigTiles = pl.bigTiles; W.bigDense = pl.bigTiles == pl.T * (pl.T + 1) / 2 ? 1 : 0; W.bigN = pl.N;
            std::memcpy(hostp(D.rowOf), pl.rowOf.data(), (size_t)nf * 4);
            std::memcpy(hostp(D.rowCam), pl.rowCam.data(), (size_t)N * 4);
            std::memcpy(hostp(L.tileMap), pl.tileMap.data(), pl.tileMap.size() * 4);
            if (!pl.work.empty()) std::memcpy(hostp(L.work), pl.work.data(), pl.work.size() * sizeof(int4));
            if (!pl.sb.empty()) std::memcpy(hostp(L.sb), pl.sb.data(), pl.sb.size() * sizeof(int4));
            if (!pl.diagList.empty()) std::memcpy(hostp(L.diagList), pl.diagList.data(), pl.diagList.size() * 4);
        }
    }
    std::memset(c.status, 0, sizeof(EgStatus));
    hipStream_t s = c.stream;
    Drain drain(s);
    EAO_HIP(hipMemcpyAsync(d, h, upEnd, hipMemcpyHostToDevice, s));
    EAO_HIP(hipMemsetAsync(d + upEnd, 0, L.scratchEnd - upEnd, s));
    EAO_HIP(hipEventRecord(c.ev0, s));
    if (solve) {
        hipLaunchKernelGGL(k_eg_measure, dim3(cdiv(m, 256)), dim3(256), 0, s, D);
        BigStepArgs A{L.big, L.bigL, L.bigDiag, L.bigFail, L.work, D.ctl, nullptr, N, 0, {}};
        const size_t bigBytes = ((size_t)pl.bigTiles << 12) * sizeof(double);
        // worst case 20 iterations of 10 trials; the verdict is read between batches of kEgSlots trials, never per trial
        for (int slot = 0; slot < kEgMaxIterations * refc::LM_MAX_TRIALS && !c.status->done; ) {
            for (int q = 0; q < kEgSlots; q++, slot++) {
                hipLaunchKernelGGL(k_eg_linearize, dim3(cdiv(m, 8)), dim3(256), 0, s, D);
                hipLaunchKernelGGL(k_eg_assemble, dim3(nBlocks), dim3(64), 0, s, D);
                hipLaunchKernelGGL(k_eg_begin, dim3(1), dim3(256), 0, s, D);
                EAO_HIP(hipMemsetAsync(L.big, 0, bigBytes, s));
                hipLaunchKernelGGL(k_eg_scatter, dim3(nBlocks), dim3(64), 0, s, D);
                gba_enqueue_factor_solve(L.W, 0, pl, A, s);
                hipLaunchKernelGGL(k_eg_apply, dim3(cdiv(nf, 256)), dim3(256), 0, s, D);
                hipLaunchKernelGGL(k_eg_errors, dim3(cdiv(m, 256)), dim3(256), 0, s, D);
                hipLaunchKernelGGL(k_eg_decide, dim3(1), dim3(256), 0, s, D);
            }
            EAO_HIP(hipGetLastError());
            EAO_HIP(drain.wait_more(Drain::Block));
        }
        EAO_REQUIRE(c.status->done, "internal: the LM loop did not reach a verdict");
    }
    hipLaunchKernelGGL(k_eg_finish, dim3(cdiv(n + nPts, 256)), dim3(256), 0, s, D);
    EAO_HIP(hipGetLastError());
    EAO_HIP(hipEventRecord(c.ev1, s));
    EAO_HIP(hipMemcpyAsync(h + outOff, d + outOff, L.outEnd - outOff, hipMemcpyDeviceToHost, s));
    EAO_HIP(drain.wait(Drain::Block));
    float ms = 0;
    EAO_HIP(hipEventElapsedTime(&ms, c.ev0, c.ev1));
    g_trace.clear();
    g_trace.deviceMs = ms;
    std::memcpy(r->Scw, hostp(D.outS), (size_t)n * 8 * sizeof(double));
    std::memcpy(r->Tiw, hostp(D.outT), (size_t)n * 16 * sizeof(float));
    if (nPts) std::memcpy(r->Xw_corrected, hostp(D.outX), (size_t)nPts * 3 * sizeof(float));
    const EgStatus& out = *c.status;
    r->n_active = g.nActive;
    r->lm_iterations = solve ? out.iters : 0;
    r->chi2_initial = solve ? out.chi0 : 0.0;
    for (int k = 0; k < kEgMaxIterations; k++) {
        const bool on = solve && k < out.iters;
        r->trials[k] = on ? out.trials[k] : 0; r->lambda[k] = on ? out.lambda[k] : 0.0; r->chi2[k] = on ? out.chi2[k] : 0.0;
        if (on) { g_trace.lambda.push_back(out.lambda[k]); g_trace.chi2.push_back(out.chi2[k]); g_trace.trials.push_back(out.trials[k]); }
    }
    g_trace.linearizations = r->lm_iterations;
    return EAO_OK;
}

}  // namespace

extern "C" {

eao_status eao_optimize_essential_graph(const eao_essential_graph_problem* p, eao_essential_graph_result* r) {
    return run_essential_graph(p, r);
}

eao_status eao_essential_graph_plan(const eao_essential_graph_problem* p, eao_gba_plan_info* info, int32_t* row_of, int32_t* tile_map, int32_t cap_tile_map) {
    EAO_REQUIRE(p && info, "null argument");
    eao_essential_graph_result none = eao_essential_graph_result();
    double dS = 0; float dT = 0;
    none.Scw = &dS; none.Tiw = &dT; none.Xw_corrected = &dT;      // (eg_check only asks that the result's arrays are there)
    eao_status st = eg_check(p, &none);
    if (st) return st;
    EgStructure g;
    GbaPlan pl;
    if ((st = eg_structure(p, g, pl))) return st;
    EAO_REQUIRE(g.nf > 0, "no free keyframe with an edge: nothing is solved");
    *info = eao_gba_plan_info{pl.nFa, pl.N, pl.T, pl.nbk, pl.bigTiles, pl.P, pl.nSep, pl.sepStart, pl.rcm, pl.bandwidth, pl.chainNatural, pl.chainEstimate,
                              (int32_t)pl.launches.size(), (int32_t)(pl.work.size() / 2), (int32_t)pl.diagList.size(), (int32_t)pl.sb.size(), (int32_t)pl.sbLaunches.size()};
    if (row_of) for (int v = 0; v < p->n; v++) row_of[v] = g.blk[v] >= 0 ? pl.rowOf[g.blk[v]] : -1;
    if (tile_map && cap_tile_map >= (int)pl.tileMap.size()) std::memcpy(tile_map, pl.tileMap.data(), pl.tileMap.size() * 4);
    return EAO_OK;
}

}  // extern "C"
