// Optimizer::OptimizeEssentialGraph core (see essgraph.hip): the g2o::Sim3
// arithmetic of sim3opt_core.h plus Sim3::log (types/sim3/sim3.h:148-230),
// the vertex construction of Optimizer.cc:1813-1815 and EdgeSim3's error
// (types/sim3/types_seven_dof_expmap.h:106-114), in the operation order of the
// reference's g2o/Eigen expressions.
#pragma once
#include "sim3opt_core.h"

namespace gfess {
namespace {

using gfsim3opt::Sim3;
using gfsim3opt::sim3_exp;
using gfsim3opt::sim3_inverse;
using gfsim3opt::sim3_map;
using gfsim3opt::sim3_mul;

SE3_HD Sim3 sim3_load(const double* p) {
    Sim3 S;
    S.r.x = p[0];
    S.r.y = p[1];
    S.r.z = p[2];
    S.r.w = p[3];
    S.t[0] = p[4];
    S.t[1] = p[5];
    S.t[2] = p[6];
    S.s = p[7];
    return S;
}

SE3_HD void sim3_store(const Sim3& S, double* p) {
    p[0] = S.r.x;
    p[1] = S.r.y;
    p[2] = S.r.z;
    p[3] = S.r.w;
    p[4] = S.t[0];
    p[5] = S.t[1];
    p[6] = S.t[2];
    p[7] = S.s;
}

// g2o::Sim3(Converter::toMatrix3d(Rcw), Converter::toVector3d(tcw), 1.0) of a
// row-major 4x4 float pose (Optimizer.cc:1813-1815, LoopClosing.cc:454-456)
SE3_HD Sim3 sim3_from_pose(const float* T) {
    double R[9];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) R[3 * i + j] = (double)T[4 * i + j];
    Sim3 S;
    S.r = gfse3::from_R(R);
#pragma unroll
    for (int i = 0; i < 3; i++) S.t[i] = (double)T[4 * i + 3];
    S.s = 1.0;
    return S;
}

// conditional exchange as two selects: no run-time index into a local array
SE3_HD void cswap(bool c, double& a, double& b) {
    const double ta = c ? b : a, tb = c ? a : b;
    a = ta;
    b = tb;
}

// x = W.lu().solve(t): Eigen::PartialPivLU of a 3x3 (row exchanges on the
// largest |entry| of the column, first one on ties) carried on the augmented
// system, then the back substitution. W row-major, destroyed.
SE3_HD void lu3_solve(double* W, const double* t, double* x) {
    double b0 = t[0], b1 = t[1], b2 = t[2];
    // column 0
    {
        const double a0 = fabs(W[0]), a1 = fabs(W[3]), a2 = fabs(W[6]);
        const bool p1 = a1 > a0;
        const bool p2 = a2 > (p1 ? a1 : a0);
        const bool s1 = p1 && !p2;
#pragma unroll
        for (int j = 0; j < 3; j++) {
            cswap(s1, W[j], W[3 + j]);
            cswap(p2, W[j], W[6 + j]);
        }
        cswap(s1, b0, b1);
        cswap(p2, b0, b2);
        W[3] /= W[0];
        W[6] /= W[0];
        W[4] -= W[3] * W[1];
        W[5] -= W[3] * W[2];
        W[7] -= W[6] * W[1];
        W[8] -= W[6] * W[2];
        b1 -= W[3] * b0;
        b2 -= W[6] * b0;
    }
    // column 1
    {
        const bool p = fabs(W[7]) > fabs(W[4]);
#pragma unroll
        for (int j = 0; j < 3; j++) cswap(p, W[3 + j], W[6 + j]);
        cswap(p, b1, b2);
        W[7] /= W[4];
        W[8] -= W[7] * W[5];
        b2 -= W[7] * b1;
    }
    b2 /= W[8];
    b1 -= W[5] * b2;
    b1 /= W[4];
    b0 -= W[1] * b1;
    b0 -= W[2] * b2;
    b0 /= W[0];
    x[0] = b0;
    x[1] = b1;
    x[2] = b2;
}

// Sim3::log (sim3.h:148-230), all four eps branches
SE3_HD void sim3_log(const Sim3& S, double* res) {
    const double sigma = log(S.s);
    double R[9];
    gfse3::to_R(S.r, R);
    const double d = 0.5 * (R[0] + R[4] + R[8] - 1);
    const double dR[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};  // deltaR (se3_ops.hpp:40-47)
    const double eps = 0.00001;
    double A, B, C, f;
    const bool smallrot = d > 1 - eps;
    if (fabs(sigma) < eps) {
        C = 1;
        if (smallrot) {
            f = 0.5;
            A = 1. / 2.;
            B = 1. / 6.;
        } else {
            const double theta = acos(d);
            const double theta2 = theta * theta;
            f = theta / (2 * sqrt(1 - d * d));
            A = (1 - cos(theta)) / (theta2);
            B = (theta - sin(theta)) / (theta2 * theta);
        }
    } else {
        C = (S.s - 1) / sigma;
        if (smallrot) {
            const double sigma2 = sigma * sigma;
            f = 0.5;
            A = ((sigma - 1) * S.s + 1) / (sigma2);
            B = ((0.5 * sigma2 - sigma + 1) * S.s) / (sigma2 * sigma);
        } else {
            const double theta = acos(d);
            f = theta / (2 * sqrt(1 - d * d));
            const double theta2 = theta * theta;
            const double a = S.s * sin(theta);
            const double b = S.s * cos(theta);
            const double c = theta2 + sigma * sigma;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / (c)) * 1. / (theta2);
        }
    }
    const double w0 = f * dR[0], w1 = f * dR[1], w2 = f * dR[2];
    const double O[9] = {0, -w2, w1, w2, 0, -w0, -w1, w0, 0};
    double BO[9], W[9];
#pragma unroll
    for (int i = 0; i < 9; i++) BO[i] = B * O[i];
    // W = A*Omega + B*Omega*Omega + C*I, the product evaluated as (B*Omega)*Omega
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const double boo = BO[3 * i] * O[j] + BO[3 * i + 1] * O[3 + j] + BO[3 * i + 2] * O[6 + j];
            W[3 * i + j] = (A * O[3 * i + j] + boo) + C * (i == j ? 1.0 : 0.0);
        }
    lu3_solve(W, S.t, res + 3);
    res[0] = w0;
    res[1] = w1;
    res[2] = w2;
    res[6] = sigma;
}

// EdgeSim3::computeError: (C * v1->estimate() * v2->estimate().inverse()).log()
SE3_HD void edge_error(const Sim3& C, const Sim3& v1, const Sim3& v2, double* e) {
    sim3_log(sim3_mul(sim3_mul(C, v1), sim3_inverse(v2)), e);
}

}  // namespace
}  // namespace gfess
