// sim3_internal.h -- g2o::Sim3 on the device, shared by sim3.hip (Optimizer::OptimizeSim3) and essential_graph.hip (Optimizer::OptimizeEssentialGraph):
// the exp map, the product and the inverse, written op by op as upstream writes them (Thirdparty/g2o/g2o/types/sim3.h:70-141, :233-255).
#pragma once
#include "lm_internal.h"

// As in lm_internal.h: the TYPE lives in eao::lm (one definition for all units); the device helper FUNCTIONS are internal to each unit (anonymous namespace, all
// inline) -- they call lm_internal.h's quaternion helpers, which are internal to each unit themselves, and the library is built without relocatable device code.
namespace eao {
namespace lm {
struct Sim3 { Quat r; double t[3]; double s; };
}  // namespace lm
}  // namespace eao

namespace {

constexpr double kSim3Eps = 0.00001;                      // types/sim3.h:93

// ---------------------------------------------------------------------- Sim3 arithmetic (types/sim3.h), op by op as upstream
// Eigen::Quaternion(const Matrix3d&).  Not lm_internal.h's quat_from_matrix on purpose: that one takes 0.5 * recip(t) (v_rcp_f64 + Newton,
// about one ulp) and picks the largest diagonal with >= (ties to the lower index); this one divides 0.5 / t exactly and picks as Eigen does
// (a strict > moves to the later index), so that every exp() here is the one tests/sim3_reference.py computes, bit for bit.
__device__ inline Quat quat_from_R_eigen(const double m[9]) {
    Quat q;
    double t = m[0] + m[4] + m[8];
    if (t > 0) {
        t = sqrt(t + 1.0);
        q.w = 0.5 * t;
        t = 0.5 / t;
        q.x = (m[7] - m[5]) * t; q.y = (m[2] - m[6]) * t; q.z = (m[3] - m[1]) * t;
        return q;
    }
    int i = 0;
    if (m[4] > m[0]) i = 1;
    if (m[8] > (i == 1 ? m[4] : m[0])) i = 2;
    if (i == 0) {
        t = sqrt(m[0] - m[4] - m[8] + 1.0);
        q.x = 0.5 * t; t = 0.5 / t;
        q.w = (m[7] - m[5]) * t; q.y = (m[3] + m[1]) * t; q.z = (m[6] + m[2]) * t;
    } else if (i == 1) {
        t = sqrt(m[4] - m[8] - m[0] + 1.0);
        q.y = 0.5 * t; t = 0.5 / t;
        q.w = (m[2] - m[6]) * t; q.z = (m[7] + m[5]) * t; q.x = (m[1] + m[3]) * t;
    } else {
        t = sqrt(m[8] - m[0] - m[4] + 1.0);
        q.z = 0.5 * t; t = 0.5 / t;
        q.w = (m[3] - m[1]) * t; q.x = (m[2] + m[6]) * t; q.y = (m[5] + m[7]) * t;
    }
    return q;
}

__device__ inline Sim3 sim3_exp(const double u[7]) {   // Sim3(const Vector7d&)
    const double w0 = u[0], w1 = u[1], w2 = u[2], sigma = u[6];
    const double theta = sqrt(w0 * w0 + w1 * w1 + w2 * w2);
    const double Om[9] = {0, -w2, w1, w2, 0, -w0, -w1, w0, 0};
    double Om2[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) Om2[i * 3 + j] = Om[i * 3] * Om[j] + Om[i * 3 + 1] * Om[3 + j] + Om[i * 3 + 2] * Om[6 + j];
    Sim3 S;
    S.s = exp(sigma);
    double A, B, C, R[9];
    if (fabs(sigma) < kSim3Eps) {
        C = 1;
        if (theta < kSim3Eps) {
            A = 1. / 2.; B = 1. / 6.;
            for (int i = 0; i < 9; i++) R[i] = ((i % 4 == 0) ? 1.0 : 0.0) + Om[i] + Om2[i];
        } else {
            const double st = sin(theta), ct = cos(theta), th2 = theta * theta;
            A = (1 - ct) / th2;
            B = (theta - st) / (th2 * theta);
            const double a = st / theta, b = (1 - ct) / (theta * theta);
            for (int i = 0; i < 9; i++) R[i] = ((i % 4 == 0) ? 1.0 : 0.0) + a * Om[i] + b * Om2[i];
        }
    } else {
        C = (S.s - 1) / sigma;
        if (theta < kSim3Eps) {
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1) * S.s + 1) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1) * S.s) / (sigma2 * sigma);
            for (int i = 0; i < 9; i++) R[i] = ((i % 4 == 0) ? 1.0 : 0.0) + Om[i] + Om2[i];
        } else {
            const double st = sin(theta), ct = cos(theta);
            const double ra = st / theta, rb = (1 - ct) / (theta * theta);
            for (int i = 0; i < 9; i++) R[i] = ((i % 4 == 0) ? 1.0 : 0.0) + ra * Om[i] + rb * Om2[i];
            const double a = S.s * st, b = S.s * ct;
            const double th2 = theta * theta, sigma2 = sigma * sigma;
            const double c = th2 + sigma2;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / c) / th2;
        }
    }
    S.r = quat_from_R_eigen(R);
    double W[9];
    for (int i = 0; i < 9; i++) W[i] = A * Om[i] + B * Om2[i] + ((i % 4 == 0) ? C : 0.0);
    for (int i = 0; i < 3; i++) S.t[i] = W[i * 3] * u[3] + W[i * 3 + 1] * u[4] + W[i * 3 + 2] * u[5];
    return S;
}

__device__ inline Sim3 sim3_mul(const Sim3& a, const Sim3& b) {   // operator*
    Sim3 r;
    r.r = quat_mul(a.r, b.r);
    double rt[3];
    quat_rotate(a.r, b.t, rt);
    for (int i = 0; i < 3; i++) r.t[i] = a.s * rt[i] + a.t[i];
    r.s = a.s * b.s;
    return r;
}

__device__ inline Sim3 sim3_inverse(const Sim3& a) {   // Sim3(r.conjugate(), r.conjugate() * ((-1. / s) * t), 1. / s)
    Sim3 r;
    r.r.x = -a.r.x; r.r.y = -a.r.y; r.r.z = -a.r.z; r.r.w = a.r.w;
    const double c = -1. / a.s;
    const double ct[3] = {c * a.t[0], c * a.t[1], c * a.t[2]};
    quat_rotate(r.r, ct, r.t);
    r.s = 1. / a.s;
    return r;
}

}  // namespace
