// pnp_internal.h -- EPnP as PnPsolver holds it (reference src/PnPsolver.cc:375-950), restated in double, op for op, for ONE wavefront: compute_pose over a list of
// correspondences, and the test of CheckInliers.  pnp_solver.hip's two numeric kernels (the hypotheses, Refine) are this one function over different lists.
//
// Layout: everything the lanes share lives in a Ws (LDS) or in the per-list arrays of a Pts (alphas, pcs, tmp: LDS for a sampled set, device memory for Refine's
// list); no register array is indexed by a run-time value.  A loop over the correspondences or over the entries of a small matrix is dealt to the lanes (PNP_LANES);
// every SUM runs inside one lane, over the correspondences in list order -- upstream's own order, so the bytes depend neither on the launch nor on the wave.  The
// short serial pieces (the 6 x k solves, gauss_newton, qr_solve, the tail of estimate_R_and_t) run on lane 0 (PNP_ONE).  The host pass of the compiler sees the
// same statements with the lanes as loops, which is how the restatement is checked against tests/pnp_solver_reference.py without a device.
//
// OpenCV's parts: cvSVD of the symmetric 3 x 3 and 12 x 12 = dense::jacobi_sym, singular values |lambda| descending, the lower index first
// among equals; cvSVD of ABt = the scheme of dense::svd3 in double; cvInvert / cvSolve(CV_SVD) = pinv(): one-sided Jacobi, a singular value counts when it exceeds
// 2 * DBL_EPSILON * (the sum of all).  Deviations from upstream: the sign of the PCA axes (sign_rows) and gauss_newton's X = 0 start.
#pragma once
#include <cfloat>
#include <cmath>

#include "common.h"
#include "small_dense.h"

namespace eao {
namespace pnp {

// ---- PnPsolver's literals (tests/golden/pnp_solver_constants.json, read from the reference text by tools/reference_literals.py; held to it by
// tests/test_pnp_solver_reference_cpu.py).  Nothing else in this file spells them.
// pnp-constants-begin
constexpr int kGaussNewtonIterations = 5;      // iterations_number
constexpr float kAlphaOne = 1.0f;              // a[0] = 1.0f - a[1] - a[2] - a[3]
constexpr float kLTwo = 2.0f;                  // row[1] = 2.0f * dot(...)
// pnp-constants-end
// ours: fixed sweep counts (quadratic convergence; 12 x 12 is diagonal to double precision after 8 to 10 on the systems of fill_M, the rest is margin)
constexpr int kSweepsPca = 10, kSweepsMtM = 16, kSweepsAbt = 10, kSweepsPinv = 12;
constexpr int kMinSetLo = 4, kMinSetHi = 64;

#if defined(__HIP_DEVICE_COMPILE__)
#define PNP_LANES(e, count) for (int e = lane; e < (count); e += 64)
#define PNP_ONE if (lane == 0)
#define PNP_SYNC() wave_sync()
#else
#define PNP_LANES(e, count) for (int e = 0; e < (count); e++)
#define PNP_ONE
#define PNP_SYNC() ((void)0)
#endif

struct Ws {
    double cws[4][3], ccs[4][3];
    double S3[9], V3[9], dc[3], uct[9], cc[9], cc_inv[9];
    double S[144], V[144], ut[144];
    double l[60], rho[6];
    double betas[4][4], rep[4], Rs[4][9], ts[4][3];
    double lsA[30], lsV[25], lsW2[5], lsP[30], lsX[5];
    double gnA[24], gnB[6], gnX[4], A1[4], A2[4];
    double pc0[3], pw0[3], abt[9], eS[9], eV[9];
    double R[9], t[3];
    int order[12];
    int choice, neg;
};

// one list of correspondences: entry i is correspondence idx[i] of the problem
struct Pts {
    const float* p3d;      // problem: n*3
    const float* p2d;      // problem: n*2
    const int* idx;
    int n;                 // number_of_correspondences
    double fu, fv, uc, vc;
    double* alphas;        // 4 n
    double* pcs;           // 3 n
    double* tmp;           // n
};
__host__ __device__ inline double pw(const Pts& P, int i, int j) { return (double)P.p3d[3 * P.idx[i] + j]; }      // add_correspondence (:363-373): float -> double
__host__ __device__ inline double us(const Pts& P, int i, int j) { return (double)P.p2d[2 * P.idx[i] + j]; }

__host__ __device__ inline double dot3d(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
__host__ __device__ inline double dist2(const double* a, const double* b) {
    return (a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]) + (a[2] - b[2]) * (a[2] - b[2]);
}

// order[i]: the index of the i-th largest |S[j][j]| (the lower index first among equals; a NaN never moves forward)
__host__ __device__ inline void order_desc(const double* S, int n, int* order) {
    for (int i = 0; i < n; i++) order[i] = i;
    for (int i = 1; i < n; i++) {
        const int o = order[i];
        const double v = fabs(S[o * n + o]);
        int j = i;
        while (j > 0 && fabs(S[order[j - 1] * n + order[j - 1]]) < v) { order[j] = order[j - 1]; j--; }
        order[j] = o;
    }
}

// the sign rule of the PCA axes: each row's component of largest magnitude is positive (the lowest index wins a tie)
__host__ __device__ inline void sign_rows(double* uct) {
    for (int i = 0; i < 3; i++) {
        int m = 0;
        for (int j = 1; j < 3; j++)
            if (fabs(uct[3 * i + j]) > fabs(uct[3 * i + m])) m = j;
        if (uct[3 * i + m] < 0.0)
            for (int j = 0; j < 3; j++) uct[3 * i + j] = -uct[3 * i + j];
    }
}

// cvInvert(CV_SVD) / cvSolve(CV_SVD): the pseudo-inverse P (n x m) of the m x n A (row-major; m <= 6, n <= 5; A is overwritten), serial.
__host__ __device__ inline void pinv(Ws& w, int m, int n) {
    double* A = w.lsA;
    double* V = w.lsV;
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) V[n * i + j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < kSweepsPinv; sweep++)
        for (int p = 0; p < n - 1; p++)
            for (int q = p + 1; q < n; q++) {
                double al = 0.0, be = 0.0, ga = 0.0;
                for (int i = 0; i < m; i++) {
                    al += A[n * i + p] * A[n * i + p];
                    be += A[n * i + q] * A[n * i + q];
                    ga += A[n * i + p] * A[n * i + q];
                }
                double c, s;
                dense::jacobi_cs(al, be, ga, c, s);
                for (int i = 0; i < m; i++) { const double a = A[n * i + p], b = A[n * i + q]; A[n * i + p] = c * a - s * b; A[n * i + q] = s * a + c * b; }
                for (int i = 0; i < n; i++) { const double a = V[n * i + p], b = V[n * i + q]; V[n * i + p] = c * a - s * b; V[n * i + q] = s * a + c * b; }
            }
    double sum = 0.0;
    for (int j = 0; j < n; j++) {
        double s2 = 0.0;
        for (int i = 0; i < m; i++) s2 += A[n * i + j] * A[n * i + j];
        w.lsW2[j] = s2;
        sum += sqrt(s2);
    }
    const double thr = 2.0 * DBL_EPSILON * sum;
    for (int r = 0; r < n; r++)
        for (int i = 0; i < m; i++) {
            double acc = 0.0;
            for (int j = 0; j < n; j++)
                if (sqrt(w.lsW2[j]) > thr) acc += V[n * r + j] * A[n * i + j] / w.lsW2[j];
            w.lsP[m * r + i] = acc;
        }
}
// x = pinv(A) b
__host__ __device__ inline void solve_svd(Ws& w, int m, int n, const double* b) {
    pinv(w, m, n);
    for (int r = 0; r < n; r++) {
        double acc = 0.0;
        for (int i = 0; i < m; i++) acc += w.lsP[m * r + i] * b[i];
        w.lsX[r] = acc;
    }
}

// qr_solve (:860-950) on the 6 x 4 gnA, gnB -> gnX, line by line; the `eta == 0` return leaves gnX as it was
__host__ __device__ inline void qr_solve(Ws& w) {
    const int nr = 6, nc = 4;
    double* pA = w.gnA;
    double* A1 = w.A1;
    double* A2 = w.A2;
    int kk = 0;      // ppAkk
    for (int k = 0; k < nc; k++) {
        int ik = kk;      // ppAik
        double eta = fabs(pA[ik]);
        for (int i = k + 1; i < nr; i++) {
            const double elt = fabs(pA[ik]);
            if (eta < elt) eta = elt;
            ik += nc;
        }
        if (eta == 0) {
            A1[k] = A2[k] = 0.0;
            return;
        } else {
            int ik2 = kk;
            double sum = 0.0;
            const double inv_eta = 1. / eta;
            for (int i = k; i < nr; i++) {
                pA[ik2] *= inv_eta;
                sum += pA[ik2] * pA[ik2];
                ik2 += nc;
            }
            double sigma = sqrt(sum);
            if (pA[kk] < 0) sigma = -sigma;
            pA[kk] += sigma;
            A1[k] = sigma * pA[kk];
            A2[k] = -eta * sigma;
            for (int j = k + 1; j < nc; j++) {
                int ij = kk;
                double sum2 = 0;
                for (int i = k; i < nr; i++) {
                    sum2 += pA[ij] * pA[ij + j - k];
                    ij += nc;
                }
                const double tau = sum2 / A1[k];
                ij = kk;
                for (int i = k; i < nr; i++) {
                    pA[ij + j - k] -= tau * pA[ij];
                    ij += nc;
                }
            }
        }
        kk += nc + 1;
    }
    // b <- Qt b
    double* pb = w.gnB;
    int jj = 0;
    for (int j = 0; j < nc; j++) {
        int ij = jj;
        double tau = 0;
        for (int i = j; i < nr; i++) {
            tau += pA[ij] * pb[i];
            ij += nc;
        }
        tau /= A1[j];
        ij = jj;
        for (int i = j; i < nr; i++) {
            pb[i] -= tau * pA[ij];
            ij += nc;
        }
        jj += nc + 1;
    }
    // X = R-1 b
    double* pX = w.gnX;
    pX[nc - 1] = pb[nc - 1] / A2[nc - 1];
    for (int i = nc - 2; i >= 0; i--) {
        int ij = i * nc + (i + 1);
        double sum = 0;
        for (int j = i + 1; j < nc; j++) {
            sum += pA[ij] * pX[j];
            ij++;
        }
        pX[i] = (pb[i] - sum) / A2[i];
    }
}

// gauss_newton (:840-858) with compute_A_and_b_gauss_newton (:812-838)
__host__ __device__ inline void gauss_newton(Ws& w, double* betas) {
    for (int i = 0; i < 4; i++) w.gnX[i] = 0.0;      // (deviation 2: upstream's x is uninitialised)
    for (int k = 0; k < kGaussNewtonIterations; k++) {
        for (int i = 0; i < 6; i++) {
            const double* rowL = w.l + i * 10;
            double* rowA = w.gnA + i * 4;
            rowA[0] = 2 * rowL[0] * betas[0] + rowL[1] * betas[1] + rowL[3] * betas[2] + rowL[6] * betas[3];
            rowA[1] = rowL[1] * betas[0] + 2 * rowL[2] * betas[1] + rowL[4] * betas[2] + rowL[7] * betas[3];
            rowA[2] = rowL[3] * betas[0] + rowL[4] * betas[1] + 2 * rowL[5] * betas[2] + rowL[8] * betas[3];
            rowA[3] = rowL[6] * betas[0] + rowL[7] * betas[1] + rowL[8] * betas[2] + 2 * rowL[9] * betas[3];
            w.gnB[i] = w.rho[i] - (rowL[0] * betas[0] * betas[0] + rowL[1] * betas[0] * betas[1] + rowL[2] * betas[1] * betas[1] + rowL[3] * betas[0] * betas[2] +
                                   rowL[4] * betas[1] * betas[2] + rowL[5] * betas[2] * betas[2] + rowL[6] * betas[0] * betas[3] + rowL[7] * betas[1] * betas[3] +
                                   rowL[8] * betas[2] * betas[3] + rowL[9] * betas[3] * betas[3]);
        }
        qr_solve(w);
        for (int i = 0; i < 4; i++) betas[i] += w.gnX[i];
    }
}

// the columns of L_6x10 a find_betas_approx_* keeps -> lsA (6 x nc), then cvSolve.  nc = 4: columns 0, 1, 3, 6; nc = 3, 5: the first nc
__host__ __device__ inline void solve_columns(Ws& w, int nc) {
    for (int i = 0; i < 6; i++)
        for (int j = 0; j < nc; j++) w.lsA[nc * i + j] = w.l[10 * i + (nc != 4 || j < 2 ? j : (j == 2 ? 3 : 6))];
    solve_svd(w, 6, nc, w.rho);
}
__host__ __device__ inline void find_betas_approx_1(Ws& w, double* betas) {      // :667-694
    solve_columns(w, 4);
    const double* b4 = w.lsX;
    if (b4[0] < 0) {
        betas[0] = sqrt(-b4[0]);
        betas[1] = -b4[1] / betas[0];
        betas[2] = -b4[2] / betas[0];
        betas[3] = -b4[3] / betas[0];
    } else {
        betas[0] = sqrt(b4[0]);
        betas[1] = b4[1] / betas[0];
        betas[2] = b4[2] / betas[0];
        betas[3] = b4[3] / betas[0];
    }
}
__host__ __device__ inline void find_betas_approx_2(Ws& w, double* betas) {      // :699-726
    solve_columns(w, 3);
    const double* b3 = w.lsX;
    if (b3[0] < 0) {
        betas[0] = sqrt(-b3[0]);
        betas[1] = (b3[2] < 0) ? sqrt(-b3[2]) : 0.0;
    } else {
        betas[0] = sqrt(b3[0]);
        betas[1] = (b3[2] > 0) ? sqrt(b3[2]) : 0.0;
    }
    if (b3[1] < 0) betas[0] = -betas[0];
    betas[2] = 0.0;
    betas[3] = 0.0;
}
__host__ __device__ inline void find_betas_approx_3(Ws& w, double* betas) {      // :731-758
    solve_columns(w, 5);
    const double* b5 = w.lsX;
    if (b5[0] < 0) {
        betas[0] = sqrt(-b5[0]);
        betas[1] = (b5[2] < 0) ? sqrt(-b5[2]) : 0.0;
    } else {
        betas[0] = sqrt(b5[0]);
        betas[1] = (b5[2] > 0) ? sqrt(b5[2]) : 0.0;
    }
    if (b5[1] < 0) betas[0] = -betas[0];
    betas[2] = b5[3] / betas[0];
    betas[3] = 0.0;
}

// compute_L_6x10 (:760-800) and compute_rho (:802-810), serial
__host__ __device__ inline void compute_L_and_rho(Ws& w) {
    for (int i = 0; i < 6; i++) {
        // the pair (a, b) of row i: (0,1) (0,2) (0,3) (1,2) (1,3) (2,3)
        const int a = i < 3 ? 0 : (i < 5 ? 1 : 2);
        const int b = i < 3 ? i + 1 : (i < 5 ? i - 1 : 3);
        double dv[4][3];
        for (int k = 0; k < 4; k++) {
            const double* v = w.ut + 12 * (11 - k);
            for (int c = 0; c < 3; c++) dv[k][c] = v[3 * a + c] - v[3 * b + c];
        }
        double* row = w.l + 10 * i;
        row[0] = dot3d(dv[0], dv[0]);
        row[1] = kLTwo * dot3d(dv[0], dv[1]);
        row[2] = dot3d(dv[1], dv[1]);
        row[3] = kLTwo * dot3d(dv[0], dv[2]);
        row[4] = kLTwo * dot3d(dv[1], dv[2]);
        row[5] = dot3d(dv[2], dv[2]);
        row[6] = kLTwo * dot3d(dv[0], dv[3]);
        row[7] = kLTwo * dot3d(dv[1], dv[3]);
        row[8] = kLTwo * dot3d(dv[2], dv[3]);
        row[9] = dot3d(dv[3], dv[3]);
    }
    w.rho[0] = dist2(w.cws[0], w.cws[1]);
    w.rho[1] = dist2(w.cws[0], w.cws[2]);
    w.rho[2] = dist2(w.cws[0], w.cws[3]);
    w.rho[3] = dist2(w.cws[1], w.cws[2]);
    w.rho[4] = dist2(w.cws[1], w.cws[3]);
    w.rho[5] = dist2(w.cws[2], w.cws[3]);
}

// one entry of the two rows fill_M (:436-451) writes for a correspondence: which = 0 is M1, 1 is M2
__host__ __device__ inline double m_entry(const Pts& P, const double* as, double u, double v, int col, int which) {
    const int i = col / 3, c = col - 3 * i;
    if (which == 0) return c == 0 ? as[i] * P.fu : (c == 1 ? 0.0 : as[i] * (P.uc - u));
    return c == 0 ? 0.0 : (c == 1 ? as[i] * P.fv : as[i] * (P.vc - v));
}

// the tail of estimate_R_and_t (:608-626) on lane 0: R = U V^T from the SVD of abt (eigenvectors of abt^T abt in eV, unsorted), the det < 0 flip, t
__host__ __device__ inline void rotation_from_abt(Ws& w, double* R, double* t) {
    int* ord = w.order;      // (LDS: its index is a run-time value)
    order_desc(w.eS, 3, ord);
    const double* A = w.abt;
    double a[3][3];      // a[i] = A v_i
    for (int i = 0; i < 3; i++)
        for (int r = 0; r < 3; r++) a[i][r] = A[3 * r] * w.eV[ord[i]] + A[3 * r + 1] * w.eV[3 + ord[i]] + A[3 * r + 2] * w.eV[6 + ord[i]];
    double u0[3], u1[3], u2[3];
    const double n0 = sqrt(a[0][0] * a[0][0] + a[0][1] * a[0][1] + a[0][2] * a[0][2]);
    const bool z0 = !(n0 > 0.0) && n0 == n0;      // (a NaN norm is not repaired: it divides)
    u0[0] = z0 ? 1.0 : a[0][0] / n0; u0[1] = z0 ? 0.0 : a[0][1] / n0; u0[2] = z0 ? 0.0 : a[0][2] / n0;
    const double pr = u0[0] * a[1][0] + u0[1] * a[1][1] + u0[2] * a[1][2];
    double b0 = a[1][0] - pr * u0[0], b1 = a[1][1] - pr * u0[1], b2 = a[1][2] - pr * u0[2];
    double n1 = sqrt(b0 * b0 + b1 * b1 + b2 * b2);
    if (n1 <= 1e-300) {      // rank <= 1: any unit vector perpendicular to u0
        const double ax = fabs(u0[0]), ay = fabs(u0[1]), az = fabs(u0[2]);
        const bool ex = ax <= ay && ax <= az, ey = !ex && ay <= az;
        const double e0 = ex ? 1.0 : 0.0, e1 = ey ? 1.0 : 0.0, e2 = (!ex && !ey) ? 1.0 : 0.0;
        b0 = u0[1] * e2 - u0[2] * e1; b1 = u0[2] * e0 - u0[0] * e2; b2 = u0[0] * e1 - u0[1] * e0;
        n1 = sqrt(b0 * b0 + b1 * b1 + b2 * b2);
    }
    u1[0] = b0 / n1; u1[1] = b1 / n1; u1[2] = b2 / n1;
    u2[0] = u0[1] * u1[2] - u0[2] * u1[1]; u2[1] = u0[2] * u1[0] - u0[0] * u1[2]; u2[2] = u0[0] * u1[1] - u0[1] * u1[0];
    const double sg = (u2[0] * a[2][0] + u2[1] * a[2][1] + u2[2] * a[2][2]) < 0.0 ? -1.0 : 1.0;
    // abt_u row i = (u0[i], u1[i], sg u2[i]); abt_v row j = (v0[j], v1[j], v2[j]); R[i][j] = dot(abt_u + 3 * i, abt_v + 3 * j)
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            const double ur[3] = {u0[i], u1[i], sg * u2[i]};
            const double vr[3] = {w.eV[3 * j + ord[0]], w.eV[3 * j + ord[1]], w.eV[3 * j + ord[2]]};
            R[3 * i + j] = dot3d(ur, vr);
        }
    const double det = R[0] * R[4] * R[8] + R[1] * R[5] * R[6] + R[2] * R[3] * R[7] - R[2] * R[4] * R[6] - R[1] * R[3] * R[8] - R[0] * R[5] * R[7];
    if (det < 0) {
        R[6] = -R[6];
        R[7] = -R[7];
        R[8] = -R[8];
    }
    t[0] = w.pc0[0] - dot3d(R, w.pw0);
    t[1] = w.pc0[1] - dot3d(R + 3, w.pw0);
    t[2] = w.pc0[2] - dot3d(R + 6, w.pw0);
}

// compute_R_and_t (:651-662) for betas[b]: compute_ccs, compute_pcs, solve_for_sign, estimate_R_and_t, reprojection_error -> Rs[b], ts[b], rep[b]
__host__ __device__ inline void compute_R_and_t(Ws& w, const Pts& P, int b, int lane) {
    const int n = P.n;
    PNP_ONE {      // compute_ccs (:453-464)
        for (int i = 0; i < 4; i++) w.ccs[i][0] = w.ccs[i][1] = w.ccs[i][2] = 0.0f;
        for (int i = 0; i < 4; i++) {
            const double* v = w.ut + 12 * (11 - i);
            for (int j = 0; j < 4; j++)
                for (int k = 0; k < 3; k++) w.ccs[j][k] += w.betas[b][i] * v[3 * j + k];
        }
    }
    PNP_SYNC();
    PNP_LANES(i, n) {      // compute_pcs (:466-475)
        const double* a = P.alphas + 4 * i;
        for (int j = 0; j < 3; j++) P.pcs[3 * i + j] = a[0] * w.ccs[0][j] + a[1] * w.ccs[1][j] + a[2] * w.ccs[2][j] + a[3] * w.ccs[3][j];
    }
    PNP_SYNC();
    PNP_ONE { w.neg = (n > 0 && P.pcs[2] < 0.0) ? 1 : 0; }      // solve_for_sign (:636-649)
    PNP_SYNC();
    if (w.neg) {
        PNP_LANES(i, 3 * n) P.pcs[i] = -P.pcs[i];
        PNP_ONE {
            for (int i = 0; i < 4; i++)
                for (int j = 0; j < 3; j++) w.ccs[i][j] = -w.ccs[i][j];
        }
    }
    PNP_SYNC();
    // estimate_R_and_t (:569-627)
    PNP_LANES(j, 6) {
        double s = 0.0;
        if (j < 3) {
            for (int i = 0; i < n; i++) s += P.pcs[3 * i + j];
            w.pc0[j] = s / n;
        } else {
            for (int i = 0; i < n; i++) s += pw(P, i, j - 3);
            w.pw0[j - 3] = s / n;
        }
    }
    PNP_SYNC();
    PNP_LANES(e, 9) {
        const int j = e / 3, c = e - 3 * j;
        double s = 0.0;
        for (int i = 0; i < n; i++) s += (P.pcs[3 * i + j] - w.pc0[j]) * (pw(P, i, c) - w.pw0[c]);
        w.abt[e] = s;
    }
    PNP_SYNC();
    PNP_LANES(e, 9) {
        const int i = e / 3, j = e - 3 * i;
        w.eS[e] = w.abt[i] * w.abt[j] + w.abt[3 + i] * w.abt[3 + j] + w.abt[6 + i] * w.abt[6 + j];
        w.eV[e] = i == j ? 1.0 : 0.0;
    }
    PNP_SYNC();
    dense::jacobi_sym<3>(w.eS, w.eV, kSweepsAbt, lane);
    PNP_ONE { rotation_from_abt(w, w.Rs[b], w.ts[b]); }
    PNP_SYNC();
    // reprojection_error (:550-567): the terms by the lanes, their sum in list order
    PNP_LANES(i, n) {
        const double* R = w.Rs[b];
        const double* t = w.ts[b];
        const double p[3] = {pw(P, i, 0), pw(P, i, 1), pw(P, i, 2)};
        const double Xc = dot3d(R, p) + t[0];
        const double Yc = dot3d(R + 3, p) + t[1];
        const double inv_Zc = 1.0 / (dot3d(R + 6, p) + t[2]);
        const double ue = P.uc + P.fu * Xc * inv_Zc;
        const double ve = P.vc + P.fv * Yc * inv_Zc;
        const double u = us(P, i, 0), v = us(P, i, 1);
        P.tmp[i] = sqrt((u - ue) * (u - ue) + (v - ve) * (v - ve));
    }
    PNP_SYNC();
    PNP_ONE {
        double sum2 = 0.0;
        for (int i = 0; i < n; i++) sum2 += P.tmp[i];
        w.rep[b] = sum2 / n;
    }
    PNP_SYNC();
}

// compute_pose (:477-525): w.R, w.t, w.rep[1..3], w.choice.  All 64 lanes of the wave call it.
__host__ __device__ inline void compute_pose(Ws& w, const Pts& P, int lane) {
    const int n = P.n;
    // choose_control_points (:375-409)
    PNP_LANES(j, 3) {
        double s = 0;
        for (int i = 0; i < n; i++) s += pw(P, i, j);
        w.cws[0][j] = s / n;
    }
    PNP_SYNC();
    PNP_LANES(e, 9) {      // cvMulTransposed(PW0, PW0tPW0, 1)
        const int a = e / 3, b = e - 3 * a;
        double s = 0.0;
        for (int i = 0; i < n; i++) s += (pw(P, i, a) - w.cws[0][a]) * (pw(P, i, b) - w.cws[0][b]);
        w.S3[e] = s;
        w.V3[e] = a == b ? 1.0 : 0.0;
    }
    PNP_SYNC();
    dense::jacobi_sym<3>(w.S3, w.V3, kSweepsPca, lane);
    PNP_ONE {
        order_desc(w.S3, 3, w.order);
        for (int i = 0; i < 3; i++) {
            w.dc[i] = fabs(w.S3[4 * w.order[i]]);
            for (int j = 0; j < 3; j++) w.uct[3 * i + j] = w.V3[3 * j + w.order[i]];
        }
        sign_rows(w.uct);      // (deviation 1)
        for (int i = 1; i < 4; i++) {
            const double k = sqrt(w.dc[i - 1] / n);
            for (int j = 0; j < 3; j++) w.cws[i][j] = w.cws[0][j] + k * w.uct[3 * (i - 1) + j];
        }
        // compute_barycentric_coordinates (:411-434): cvInvert(CC, CC_inv, CV_SVD)
        for (int i = 0; i < 3; i++)
            for (int j = 1; j < 4; j++) w.lsA[3 * i + j - 1] = w.cws[j][i] - w.cws[0][i];
        pinv(w, 3, 3);
        for (int i = 0; i < 9; i++) w.cc_inv[i] = w.lsP[i];
    }
    PNP_SYNC();
    PNP_LANES(i, n) {
        const double* ci = w.cc_inv;
        double* a = P.alphas + 4 * i;
        const double p[3] = {pw(P, i, 0), pw(P, i, 1), pw(P, i, 2)};
        for (int j = 0; j < 3; j++) a[1 + j] = ci[3 * j] * (p[0] - w.cws[0][0]) + ci[3 * j + 1] * (p[1] - w.cws[0][1]) + ci[3 * j + 2] * (p[2] - w.cws[0][2]);
        a[0] = kAlphaOne - a[1] - a[2] - a[3];
    }
    PNP_SYNC();
    // fill_M (:436-451) and cvMulTransposed(M, MtM, 1): entry (a, b) is the sum over M's rows in their order, inside one lane
    PNP_LANES(e, 144) {
        const int a = e / 12, b = e - 12 * a;
        double s = 0.0;
        for (int i = 0; i < n; i++) {
            const double* as = P.alphas + 4 * i;
            const double u = us(P, i, 0), v = us(P, i, 1);
            s += m_entry(P, as, u, v, a, 0) * m_entry(P, as, u, v, b, 0);
            s += m_entry(P, as, u, v, a, 1) * m_entry(P, as, u, v, b, 1);
        }
        w.S[e] = s;
        w.V[e] = a == b ? 1.0 : 0.0;
    }
    PNP_SYNC();
    dense::jacobi_sym<12>(w.S, w.V, kSweepsMtM, lane);
    PNP_ONE { order_desc(w.S, 12, w.order); }
    PNP_SYNC();
    PNP_LANES(e, 144) {      // CV_SVD_U_T: row i of ut is the i-th singular vector
        const int i = e / 12, k = e - 12 * i;
        w.ut[e] = w.V[12 * k + w.order[i]];
    }
    PNP_SYNC();
    PNP_ONE {
        compute_L_and_rho(w);
        find_betas_approx_1(w, w.betas[1]);
        gauss_newton(w, w.betas[1]);
    }
    PNP_SYNC();
    compute_R_and_t(w, P, 1, lane);
    PNP_ONE {
        find_betas_approx_2(w, w.betas[2]);
        gauss_newton(w, w.betas[2]);
    }
    PNP_SYNC();
    compute_R_and_t(w, P, 2, lane);
    PNP_ONE {
        find_betas_approx_3(w, w.betas[3]);
        gauss_newton(w, w.betas[3]);
    }
    PNP_SYNC();
    compute_R_and_t(w, P, 3, lane);
    PNP_ONE {
        int N = 1;
        if (w.rep[2] < w.rep[1]) N = 2;
        if (w.rep[3] < w.rep[N]) N = 3;
        w.choice = N;
        for (int i = 0; i < 9; i++) w.R[i] = w.Rs[N][i];
        for (int i = 0; i < 3; i++) w.t[i] = w.ts[N][i];
    }
    PNP_SYNC();
}

// the test of CheckInliers (:312-338) for one correspondence, with upstream's widths: Xc, Yc, invZc are double expressions rounded to float, ue / ve double,
// distX / distY / error2 float, the gate a float.  A NaN error2 fails the comparison.
__host__ __device__ inline bool is_inlier(const double* R, const double* t, const float* X, const float* uv, double fu, double fv, double uc, double vc, float max_error) {
    const float Xc = (float)(R[0] * X[0] + R[1] * X[1] + R[2] * X[2] + t[0]);
    const float Yc = (float)(R[3] * X[0] + R[4] * X[1] + R[5] * X[2] + t[1]);
    const float invZc = (float)(1 / (R[6] * X[0] + R[7] * X[1] + R[8] * X[2] + t[2]));
    const double ue = uc + fu * Xc * invZc;
    const double ve = vc + fv * Yc * invZc;
    const float distX = (float)(uv[0] - ue);
    const float distY = (float)(uv[1] - ve);
    const float error2 = distX * distX + distY * distY;
    return error2 < max_error;
}

}  // namespace pnp
}  // namespace eao
