// small_dense.h -- the small dense helpers the geometric solvers share (device code; include from a .hip).
//   smallest_eigenvector   4 x 4 symmetric, per lane in registers (triangulate.hip, initializer.hip: the vt.row(3) of a 4 x 4 cv::SVD)
//   jacobi_sym<N>          symmetric N x N eigenproblem, one wavefront, S and V in LDS (null_vector9; pnp_internal.h: cvSVD of the symmetric 3 x 3 and 12 x 12)
//   null_vector9           right singular vector of the smallest singular value of a k x 9 float system, one wavefront, S and V in LDS
//   svd3                   full 3 x 3 SVD of a float matrix (U, w, Vt as cv::SVD::compute with FULL_UV holds them: CV_32F, w descending)
//   inv3 / mul3 / det3     OpenCV's 3 x 3 float inverse, product and determinant
//   kth_smallest           k-th smallest of a masked float list, one workgroup, radix select over the ordered bit patterns
// Conventions (DESIGN.md "Sim3Solver", section 4e, "Initializer"): a small cv::Mat product accumulates each element in double, k in storage order, and rounds once
// to float; a singular vector is an eigenvector of A^T A formed in double from the float A, by cyclic Jacobi with a FIXED sweep count (no data-dependent loop, so a
// NaN input ends like any other), rounded to float.  No array below is indexed by a runtime value unless it lives in LDS.
#pragma once
#include "common.h"

namespace eao {
namespace dense {

constexpr int kSweeps4 = 8;       // 4 x 4: diagonal to double precision after 5 or 6 (quadratic convergence)
constexpr int kSweeps3 = 8;       // 3 x 3
constexpr int kSweeps9 = 12;      // 9 x 9: 7 or 8 suffice on the systems of ComputeH21 / ComputeF21; the rest is margin at 36 rotations a sweep

// eigenvector of the smallest eigenvalue of the symmetric S = A^T A, by kSweeps4 cyclic Jacobi sweeps; every index below is a compile-time constant after unrolling
__device__ __forceinline__ void smallest_eigenvector(double (&S)[4][4], double (&v)[4]) {
    double V[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) V[i][j] = i == j ? 1.0 : 0.0;
#pragma unroll 1
    for (int sweep = 0; sweep < kSweeps4; sweep++) {
#pragma unroll
        for (int p = 0; p < 3; p++)
#pragma unroll
            for (int q = p + 1; q < 4; q++) {
                const double apq = S[p][q];
                double c = 1.0, s = 0.0;
                if (apq != 0.0) {
                    const double theta = (S[q][q] - S[p][p]) / (2.0 * apq);
                    const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                    c = 1.0 / sqrt(t * t + 1.0);
                    s = t * c;
                }
#pragma unroll
                for (int k = 0; k < 4; k++) { const double a = S[k][p], b = S[k][q]; S[k][p] = c * a - s * b; S[k][q] = s * a + c * b; }
#pragma unroll
                for (int k = 0; k < 4; k++) { const double a = S[p][k], b = S[q][k]; S[p][k] = c * a - s * b; S[q][k] = s * a + c * b; }
#pragma unroll
                for (int k = 0; k < 4; k++) { const double a = V[k][p], b = V[k][q]; V[k][p] = c * a - s * b; V[k][q] = s * a + c * b; }
            }
    }
    double best = S[0][0];
#pragma unroll
    for (int k = 0; k < 4; k++) v[k] = V[k][0];
#pragma unroll
    for (int j = 1; j < 4; j++) {
        const bool less = S[j][j] < best;      // the first of equal eigenvalues
        best = less ? S[j][j] : best;
#pragma unroll
        for (int k = 0; k < 4; k++) v[k] = less ? V[k][j] : v[k];
    }
}

// the Jacobi rotation that annihilates S[p][q] (c = 1, s = 0 when it is exactly zero: nothing to annihilate)
__host__ __device__ __forceinline__ void jacobi_cs(double app, double aqq, double apq, double& c, double& s) {
    c = 1.0; s = 0.0;
    if (apq != 0.0) {
        const double theta = (aqq - app) / (2.0 * apq);
        const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        c = 1.0 / sqrt(t * t + 1.0);
        s = t * c;
    }
}

// One wavefront, N <= 64.  `sweeps` cyclic Jacobi sweeps over the symmetric N x N S (row-major doubles in LDS); V (N x N, the identity on entry) leaves with the
// eigenvectors in its columns, S with the eigenvalues on its diagonal, in no particular order.  Lane k < N owns row / column k of a rotation; the pair (p, q) is
// uniform over the wave, so the runtime indices are LDS addresses, never register indices.  The sweep count is fixed: a NaN ends like any other input.  The host
// pass of the compiler sees the same rotations with the lanes as a loop (a rotation's two phases touch disjoint entries per k), for CPU checks of the callers.
template <int N>
__host__ __device__ inline void jacobi_sym(double* S, double* V, int sweeps, int lane) {
#if defined(__HIP_DEVICE_COMPILE__)
    const bool own = lane < N;
    const int k = own ? lane : 0;
#pragma unroll 1
    for (int sweep = 0; sweep < sweeps; sweep++) {
#pragma unroll 1
        for (int p = 0; p < N - 1; p++)
#pragma unroll 1
            for (int q = p + 1; q < N; q++) {
                double c, s;
                jacobi_cs(S[N * p + p], S[N * q + q], S[N * p + q], c, s);
                wave_sync();
                if (own) { const double a = S[N * k + p], b = S[N * k + q]; S[N * k + p] = c * a - s * b; S[N * k + q] = s * a + c * b; }
                wave_sync();
                if (own) {
                    const double a = S[N * p + k], b = S[N * q + k]; S[N * p + k] = c * a - s * b; S[N * q + k] = s * a + c * b;
                    const double va = V[N * k + p], vb = V[N * k + q]; V[N * k + p] = c * va - s * vb; V[N * k + q] = s * va + c * vb;
                }
                wave_sync();
            }
    }
#else
    (void)lane;
    for (int sweep = 0; sweep < sweeps; sweep++)
        for (int p = 0; p < N - 1; p++)
            for (int q = p + 1; q < N; q++) {
                double c, s;
                jacobi_cs(S[N * p + p], S[N * q + q], S[N * p + q], c, s);
                for (int k = 0; k < N; k++) { const double a = S[N * k + p], b = S[N * k + q]; S[N * k + p] = c * a - s * b; S[N * k + q] = s * a + c * b; }
                for (int k = 0; k < N; k++) {
                    const double a = S[N * p + k], b = S[N * q + k]; S[N * p + k] = c * a - s * b; S[N * q + k] = s * a + c * b;
                    const double va = V[N * k + p], vb = V[N * k + q]; V[N * k + p] = c * va - s * vb; V[N * k + q] = s * va + c * vb;
                }
            }
#endif
}

// One wavefront.  A: rows x 9 floats in LDS (row-major, rows <= 16); S, V: 81 doubles each in LDS (scratch).  Every lane leaves with the same h: the eigenvector of
// the smallest eigenvalue (the first of equal ones) of A^T A, rounded to float -- vt.row(8) of cv::SVDecomp(A, FULL_UV) up to its sign (jacobi_sym<9>).
__device__ __forceinline__ void null_vector9(const float* A, int rows, double* S, double* V, int lane, float (&h)[9]) {
    for (int e = lane; e < 81; e += 64) {
        const int i = e / 9, j = e - 9 * i;
        double s = 0.0;
        for (int r = 0; r < rows; r++) s += (double)A[9 * r + i] * (double)A[9 * r + j];
        S[e] = s;
        V[e] = i == j ? 1.0 : 0.0;
    }
    wave_sync();
    jacobi_sym<9>(S, V, kSweeps9, lane);
    int jmin = 0;
    double best = S[0];
#pragma unroll 1
    for (int j = 1; j < 9; j++) {
        const double d = S[10 * j];
        if (d < best) { best = d; jmin = j; }
    }
#pragma unroll
    for (int i = 0; i < 9; i++) h[i] = (float)V[9 * i + jmin];
}

// one element of a small float gemm
__host__ __device__ inline float gemm3(float a0, float a1, float a2, float b0, float b1, float b2) {
    return (float)((double)a0 * (double)b0 + (double)a1 * (double)b1 + (double)a2 * (double)b2);
}
// C = A * B, row-major 3 x 3 floats (C may not alias)
__host__ __device__ inline void mul3(const float* A, const float* B, float* C) {
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) C[3 * i + j] = gemm3(A[3 * i], A[3 * i + 1], A[3 * i + 2], B[j], B[3 + j], B[6 + j]);
}
__host__ __device__ inline void transpose3(const float* A, float* T) {
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) T[3 * i + j] = A[3 * j + i];
}
// cv::determinant of a 3 x 3 CV_32F: double
__host__ __device__ inline double det3(const float* m) {
    return (double)m[0] * ((double)m[4] * (double)m[8] - (double)m[5] * (double)m[7]) - (double)m[1] * ((double)m[3] * (double)m[8] - (double)m[5] * (double)m[6]) +
           (double)m[2] * ((double)m[3] * (double)m[7] - (double)m[4] * (double)m[6]);
}
// cv::Mat::inv() of a 3 x 3 CV_32F: cofactors over a double determinant, each element rounded once; a zero determinant gives the zero matrix
__host__ __device__ inline void inv3(const float* m, float* o) {
    double d = det3(m);
    if (d != 0.0) {
        d = 1.0 / d;
        o[0] = (float)(((double)m[4] * (double)m[8] - (double)m[5] * (double)m[7]) * d);
        o[1] = (float)(((double)m[2] * (double)m[7] - (double)m[1] * (double)m[8]) * d);
        o[2] = (float)(((double)m[1] * (double)m[5] - (double)m[2] * (double)m[4]) * d);
        o[3] = (float)(((double)m[5] * (double)m[6] - (double)m[3] * (double)m[8]) * d);
        o[4] = (float)(((double)m[0] * (double)m[8] - (double)m[2] * (double)m[6]) * d);
        o[5] = (float)(((double)m[2] * (double)m[3] - (double)m[0] * (double)m[5]) * d);
        o[6] = (float)(((double)m[3] * (double)m[7] - (double)m[4] * (double)m[6]) * d);
        o[7] = (float)(((double)m[1] * (double)m[6] - (double)m[0] * (double)m[7]) * d);
        o[8] = (float)(((double)m[0] * (double)m[4] - (double)m[1] * (double)m[3]) * d);
    } else {
        for (int i = 0; i < 9; i++) o[i] = 0.f;
    }
}

// Full SVD of the row-major 3 x 3 float A: A = U diag(w) Vt, w descending, all three as floats.  V and w from the symmetric eigen problem of A^T A (double); u0 and
// u1 are A v normalised (Gram-Schmidt between them); u2 is u0 x u1, its sign that of A v2 -- so a column that belongs to a vanishing singular value never divides by
// it.  The signs of the pairs (u_i, v_i) are free, as cv::SVD's are.
__device__ __forceinline__ void svd3(const float (&A)[9], float (&U)[9], float (&w)[3], float (&Vt)[9]) {
    double S[3][3], V[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            S[i][j] = (double)A[i] * (double)A[j] + (double)A[3 + i] * (double)A[3 + j] + (double)A[6 + i] * (double)A[6 + j];
            V[i][j] = i == j ? 1.0 : 0.0;
        }
#pragma unroll 1
    for (int sweep = 0; sweep < kSweeps3; sweep++) {
#pragma unroll
        for (int p = 0; p < 2; p++)
#pragma unroll
            for (int q = p + 1; q < 3; q++) {
                double c, s;
                jacobi_cs(S[p][p], S[q][q], S[p][q], c, s);
#pragma unroll
                for (int k = 0; k < 3; k++) { const double a = S[k][p], b = S[k][q]; S[k][p] = c * a - s * b; S[k][q] = s * a + c * b; }
#pragma unroll
                for (int k = 0; k < 3; k++) { const double a = S[p][k], b = S[q][k]; S[p][k] = c * a - s * b; S[q][k] = s * a + c * b; }
#pragma unroll
                for (int k = 0; k < 3; k++) { const double a = V[k][p], b = V[k][q]; V[k][p] = c * a - s * b; V[k][q] = s * a + c * b; }
            }
    }
    double l[3] = {S[0][0], S[1][1], S[2][2]};
    // descending: three compare-exchanges over (eigenvalue, column)
#define EAO_SVD3_CX(a, b)                                                                     \
    {                                                                                         \
        const bool sw = l[a] < l[b];                                                          \
        const double t = l[a]; l[a] = sw ? l[b] : l[a]; l[b] = sw ? t : l[b];                 \
        _Pragma("unroll") for (int k = 0; k < 3; k++) {                                       \
            const double u = V[k][a]; V[k][a] = sw ? V[k][b] : V[k][a]; V[k][b] = sw ? u : V[k][b]; \
        }                                                                                     \
    }
    EAO_SVD3_CX(0, 1) EAO_SVD3_CX(1, 2) EAO_SVD3_CX(0, 1)
#undef EAO_SVD3_CX
    double a[3][3];      // a[i] = A v_i
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int r = 0; r < 3; r++) a[i][r] = (double)A[3 * r] * V[0][i] + (double)A[3 * r + 1] * V[1][i] + (double)A[3 * r + 2] * V[2][i];
    double u0[3], u1[3], u2[3];
    const double n0 = sqrt(a[0][0] * a[0][0] + a[0][1] * a[0][1] + a[0][2] * a[0][2]);
    const bool z0 = !(n0 > 0.0);
    u0[0] = z0 ? 1.0 : a[0][0] / n0; u0[1] = z0 ? 0.0 : a[0][1] / n0; u0[2] = z0 ? 0.0 : a[0][2] / n0;
    const double pr = u0[0] * a[1][0] + u0[1] * a[1][1] + u0[2] * a[1][2];
    double b0 = a[1][0] - pr * u0[0], b1 = a[1][1] - pr * u0[1], b2 = a[1][2] - pr * u0[2];
    double n1 = sqrt(b0 * b0 + b1 * b1 + b2 * b2);
    if (!(n1 > 1e-300)) {      // rank <= 1: any unit vector perpendicular to u0 (its cross product with the axis it is least aligned with)
        const double ax = fabs(u0[0]), ay = fabs(u0[1]), az = fabs(u0[2]);
        const bool ex = ax <= ay && ax <= az, ey = !ex && ay <= az;
        const double e0 = ex ? 1.0 : 0.0, e1 = ey ? 1.0 : 0.0, e2 = (!ex && !ey) ? 1.0 : 0.0;
        b0 = u0[1] * e2 - u0[2] * e1; b1 = u0[2] * e0 - u0[0] * e2; b2 = u0[0] * e1 - u0[1] * e0;
        n1 = sqrt(b0 * b0 + b1 * b1 + b2 * b2);
    }
    u1[0] = b0 / n1; u1[1] = b1 / n1; u1[2] = b2 / n1;
    u2[0] = u0[1] * u1[2] - u0[2] * u1[1]; u2[1] = u0[2] * u1[0] - u0[0] * u1[2]; u2[2] = u0[0] * u1[1] - u0[1] * u1[0];
    const double sg = (u2[0] * a[2][0] + u2[1] * a[2][1] + u2[2] * a[2][2]) < 0.0 ? -1.0 : 1.0;
#pragma unroll
    for (int r = 0; r < 3; r++) {
        U[3 * r] = (float)u0[r]; U[3 * r + 1] = (float)u1[r]; U[3 * r + 2] = (float)(sg * u2[r]);
#pragma unroll
        for (int c = 0; c < 3; c++) Vt[3 * r + c] = (float)V[c][r];
    }
#pragma unroll
    for (int i = 0; i < 3; i++) w[i] = (float)sqrt(l[i] > 0.0 ? l[i] : 0.0);
}

// a float's bit pattern as an unsigned key with the floats' order (-inf < ... < -0 < +0 < ... < +inf < NaN with the sign bit clear)
__device__ __forceinline__ unsigned ordered_key(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_value(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// One workgroup (all of its threads call it).  The k-th smallest (0-based) of key[i], i < n with take[i] != 0, as a key; hist: 256 ints of LDS, slot: 2 ints of LDS.
// Four passes of a radix select, most significant byte first.  Counts are integers, so the atomics leave no run-to-run difference.  0 <= k < number taken.
__device__ __forceinline__ unsigned kth_smallest(const unsigned* key, const unsigned char* take, int n, int k, int* hist, int* slot) {
    unsigned prefix = 0, mask = 0;
#pragma unroll 1
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (int b = threadIdx.x; b < 256; b += blockDim.x) hist[b] = 0;
        __syncthreads();
        for (int i = threadIdx.x; i < n; i += blockDim.x)
            if (take[i] && (key[i] & mask) == prefix) atomicAdd(&hist[(key[i] >> shift) & 255u], 1);
        __syncthreads();
        if (threadIdx.x == 0) {
            int b = 0, left = k;
            while (b < 255 && left >= hist[b]) { left -= hist[b]; b++; }
            slot[0] = b; slot[1] = left;
        }
        __syncthreads();
        prefix |= (unsigned)slot[0] << shift;
        mask |= 255u << shift;
        k = slot[1];
        __syncthreads();
    }
    return prefix;
}

}  // namespace dense
}  // namespace eao
