// Optimizer::OptimizeSim3 core (see sim3opt.hip): g2o::Sim3 arithmetic
// (Thirdparty/g2o/g2o/types/sim3/sim3.h) and the one-wave Levenberg-Marquardt
// over one VertexSim3Expmap, written to the operation order of the reference's
// g2o/Eigen expressions like se3.h.
#pragma once
#include <cfloat>

#include "common.h"
#include "se3.h"

namespace gfsim3opt {
namespace {

using gfse3::Quat;

// g2o::Sim3: quaternion (not normalised by any of its operations), t, s
struct Sim3 {
    Quat r;
    double t[3];
    double s;
};

// Sim3(const Vector7d& update) (sim3.h:70-142), all four eps branches
SE3_HD Sim3 sim3_exp(const double* u) {
    const double w0 = u[0], w1 = u[1], w2 = u[2];
    const double sigma = u[6];
    const double theta = sqrt((w0 * w0 + w1 * w1) + w2 * w2);
    const double O[9] = {0, -w2, w1, w2, 0, -w0, -w1, w0, 0};
    Sim3 S;
    S.s = exp(sigma);
    double O2[9];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) O2[3 * i + j] = O[3 * i] * O[j] + O[3 * i + 1] * O[3 + j] + O[3 * i + 2] * O[6 + j];
    const double eps = 0.00001;
    double A, B, C, ra = 1.0, rb = 1.0;  // R = (I + ra Omega) + rb Omega2
    if (fabs(sigma) < eps) {
        C = 1;
        if (theta < eps) {
            A = 1. / 2.;
            B = 1. / 6.;
        } else {
            const double theta2 = theta * theta;
            A = (1 - cos(theta)) / (theta2);
            B = (theta - sin(theta)) / (theta2 * theta);
            ra = sin(theta) / theta;
            rb = (1 - cos(theta)) / (theta * theta);
        }
    } else {
        C = (S.s - 1) / sigma;
        if (theta < eps) {
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1) * S.s + 1) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1) * S.s) / (sigma2 * sigma);
        } else {
            ra = sin(theta) / theta;
            rb = (1 - cos(theta)) / (theta * theta);
            const double a = S.s * sin(theta);
            const double b = S.s * cos(theta);
            const double theta2 = theta * theta;
            const double sigma2 = sigma * sigma;
            const double c = theta2 + sigma2;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / (c)) * 1. / (theta2);
        }
    }
    double R[9], W[9];
    const bool small = theta < eps;  // R = I + Omega + Omega2 without the factors
#pragma unroll
    for (int i = 0; i < 9; i++) {
        const double I = i % 4 == 0 ? 1.0 : 0.0;
        R[i] = small ? (I + O[i]) + O2[i] : (I + ra * O[i]) + rb * O2[i];
        W[i] = (A * O[i] + B * O2[i]) + C * I;
    }
    S.r = gfse3::from_R(R);
#pragma unroll
    for (int i = 0; i < 3; i++) S.t[i] = (W[3 * i] * u[3] + W[3 * i + 1] * u[4]) + W[3 * i + 2] * u[5];
    return S;
}

// Sim3::operator* (:266-272)
SE3_HD Sim3 sim3_mul(const Sim3& a, const Sim3& b) {
    Sim3 r;
    r.r = gfse3::mul(a.r, b.r);
    double rt[3];
    gfse3::rotate(a.r, b.t, rt);
#pragma unroll
    for (int i = 0; i < 3; i++) r.t[i] = a.s * rt[i] + a.t[i];
    r.s = a.s * b.s;
    return r;
}

// Sim3::map (:144-146): s*(r*xyz) + t
SE3_HD void sim3_map(const Sim3& S, const double* p, double* o) {
    double rp[3];
    gfse3::rotate(S.r, p, rp);
#pragma unroll
    for (int i = 0; i < 3; i++) o[i] = S.s * rp[i] + S.t[i];
}

// Sim3::inverse (:233-236)
SE3_HD Sim3 sim3_inverse(const Sim3& S) {
    Sim3 I;
    I.r.w = S.r.w;
    I.r.x = -S.r.x;
    I.r.y = -S.r.y;
    I.r.z = -S.r.z;
    const double f = -1. / S.s;
    const double ft[3] = {f * S.t[0], f * S.t[1], f * S.t[2]};
    gfse3::rotate(I.r, ft, I.t);
    I.s = 1. / S.s;
    return I;
}

#if defined(__HIPCC__)

constexpr int SO_T = 64;          // threads per problem: one wave
constexpr int SO_P = 64;          // pairs per pass
constexpr int SO_E = 2 * SO_P;    // edges per pass: e12_i, e21_i interleaved
constexpr int SO_TP = SO_E + 1;   // term row pitch (doubles)
constexpr int SO_NH = 28;         // lower triangle of the 7x7 H
constexpr int SO_CHI = 35;        // rows: 28 H, 7 b, robust chi2
constexpr int SO_ROWS = 36;
constexpr int SO_NSIM = 15;       // the estimate and its 14 perturbations

struct Sim3OptArgs {
    const float* X1;  // [total][3] KF1's point in camera 1
    const float* X2;  // [total][3] KF2's point in camera 2
    const float* z1;  // [total][2] keypoint of KF1
    const float* z2;  // [total][2] keypoint of KF2
    const float* w1;  // [total] information of e12
    const float* w2;  // [total] information of e21
    const int32_t* offs;  // [nprob + 1] problem p's pairs are [offs[p], offs[p + 1])
    const float* K;       // [nprob][8] fx1 fy1 cx1 cy1 fx2 fy2 cx2 cy2
    const float* th2;     // [nprob]
    double* est;          // [nprob][8] qx qy qz qw tx ty tz s, in and out
    uint8_t* inl;         // [total] in: ignored; out: 1 = the match is kept
    int32_t* nin;         // [nprob]
    int32_t* stats;       // [nprob][4] iterations and LM trials of the two rounds, or null
};

struct Pair {
    double X1[3], X2[3], z1[2], z2[2], w1, w2;
};

struct Cams {
    double f1[2], c1[2], f2[2], c2[2];
};

__device__ __forceinline__ Pair load_pair(const Sim3OptArgs& A, int g) {
    Pair P;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        P.X1[k] = (double)A.X1[3 * (size_t)g + k];
        P.X2[k] = (double)A.X2[3 * (size_t)g + k];
    }
#pragma unroll
    for (int k = 0; k < 2; k++) {
        P.z1[k] = (double)A.z1[2 * (size_t)g + k];
        P.z2[k] = (double)A.z2[2 * (size_t)g + k];
    }
    P.w1 = (double)A.w1[g];
    P.w2 = (double)A.w2[g];
    return P;
}

// EdgeSim3ProjectXYZ::computeError (types_seven_dof_expmap.h:138-145)
__device__ __forceinline__ void err12(const Pair& P, const Cams& C, const Sim3& S, double& r0, double& r1) {
    double pc[3];
    sim3_map(S, P.X2, pc);
    r0 = P.z1[0] - ((pc[0] / pc[2]) * C.f1[0] + C.c1[0]);
    r1 = P.z1[1] - ((pc[1] / pc[2]) * C.f1[1] + C.c1[1]);
}

// EdgeInverseSim3ProjectXYZ::computeError (:160-167), Sinv = estimate().inverse()
__device__ __forceinline__ void err21(const Pair& P, const Cams& C, const Sim3& Sinv, double& r0, double& r1) {
    double pc[3];
    sim3_map(Sinv, P.X1, pc);
    r0 = P.z2[0] - ((pc[0] / pc[2]) * C.f2[0] + C.c2[0]);
    r1 = P.z2[1] - ((pc[1] / pc[2]) * C.f2[1] + C.c2[1]);
}

__device__ __forceinline__ void robustify(double e, double delta, double dsqr, double& rho0, double& rho1) {
    if (e <= dsqr) {
        rho0 = e;
        rho1 = 1.;
    } else {
        const double s = sqrt(e);
        rho0 = 2 * s * delta - dsqr;
        rho1 = delta / s;
    }
}

__device__ __forceinline__ Sim3 lds_sim(const double* p) {
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

__device__ __forceinline__ void sim_lds(const Sim3& S, double* p) {
    p[0] = S.r.x;
    p[1] = S.r.y;
    p[2] = S.r.z;
    p[3] = S.r.w;
    p[4] = S.t[0];
    p[5] = S.t[1];
    p[6] = S.t[2];
    p[7] = S.s;
}

struct Problem {
    int base, n, l;
    double th2, delta, dsqr;
    Cams C;
};

// One edge's terms at column `col`: robust chi2, and (build) the 28 + 7 terms
// of H and b from the central-difference Jacobian (base_binary_edge.hpp:147-196)
// over the shared perturbed similarities sims[1 + 2 d] (+delta), sims[2 + 2 d]
// (-delta); INV selects EdgeInverseSim3ProjectXYZ and the inverse table.
template <bool INV>
__device__ __forceinline__ void edge_terms(const Problem& Q, const Pair& P, const double (*sims)[8], bool build,
                                           double (*term)[SO_TP], int col) {
    double r0, r1;
    const Sim3 S0 = lds_sim(sims[0]);
    if (INV)
        err21(P, Q.C, S0, r0, r1);
    else
        err12(P, Q.C, S0, r0, r1);
    const double info = INV ? P.w2 : P.w1;
    const double chi2 = r0 * (info * r0) + r1 * (info * r1);
    double rho0, rho1;
    robustify(chi2, Q.delta, Q.dsqr, rho0, rho1);
    term[SO_CHI][col] = rho0;
    if (!build) return;
    const double scalar = 1.0 / (2 * 1e-9);
    double J0[7], J1[7];
#pragma unroll
    for (int d = 0; d < 7; d++) {
        double p0, p1, m0, m1;
        const Sim3 Sp = lds_sim(sims[1 + 2 * d]), Sm = lds_sim(sims[2 + 2 * d]);
        if (INV) {
            err21(P, Q.C, Sp, p0, p1);
            err21(P, Q.C, Sm, m0, m1);
        } else {
            err12(P, Q.C, Sp, p0, p1);
            err12(P, Q.C, Sm, m0, m1);
        }
        J0[d] = scalar * (p0 - m0);
        J1[d] = scalar * (p1 - m1);
    }
    const double w = rho1 * info;
    const double o0 = -(info * r0) * rho1, o1 = -(info * r1) * rho1;
    int k = 0;
#pragma unroll
    for (int a = 0; a < 7; a++)
#pragma unroll
        for (int b = 0; b <= a; b++) term[k++][col] = (J0[a] * w) * J0[b] + (J1[a] * w) * J1[b];
#pragma unroll
    for (int a = 0; a < 7; a++) term[SO_NH + a][col] = J0[a] * o0 + J1[a] * o1;
}

// computeActiveErrors + activeRobustChi2 (+ buildSystem when `build`) at T over
// the active pairs; the sums land in sh_sum: [0,28) lower H, [28,35) b, 35 chi2.
// One term per edge, added in the active-edge order e12_0, e21_0, e12_1, ...
// (an inactive pair's terms are zeros, which leave every partial sum as it is).
__device__ __forceinline__ void pass(const Sim3OptArgs& A, const Problem& Q, const Sim3& T, bool build,
                                     double (*term)[SO_TP], double (*sims)[8], double (*sinv)[8], double* sh_sum) {
    // the 15 similarities of this linearisation and their inverses, shared by every edge
    if (Q.l < (build ? SO_NSIM : 1)) {
        Sim3 S = T;
        if (Q.l > 0) {
            double u[7] = {0, 0, 0, 0, 0, 0, 0};
            const int d = (Q.l - 1) >> 1;
            const double dv = (Q.l & 1) ? 1e-9 : -1e-9;
#pragma unroll
            for (int k = 0; k < 7; k++)
                if (k == d) u[k] = dv;
            S = sim3_mul(sim3_exp(u), T);
        }
        sim_lds(S, sims[Q.l]);
        sim_lds(sim3_inverse(S), sinv[Q.l]);
    }
    __syncthreads();
    double acc = 0.0;
    const int nrows = build ? SO_ROWS : 1;
    for (int b0 = 0; b0 < Q.n; b0 += SO_P) {
        const int e = b0 + Q.l;
        if (e < Q.n) {
            if (A.inl[Q.base + e]) {
                const Pair P = load_pair(A, Q.base + e);
                edge_terms<false>(Q, P, sims, build, term, 2 * Q.l);
                edge_terms<true>(Q, P, sinv, build, term, 2 * Q.l + 1);
            } else {
                for (int r = build ? 0 : SO_CHI; r < SO_ROWS; r++) term[r][2 * Q.l] = term[r][2 * Q.l + 1] = 0.0;
            }
        }
        __syncthreads();
        const int m = 2 * min(SO_P, Q.n - b0);
        const int row = build ? Q.l : SO_CHI;
        if (Q.l < nrows) {
            const double* tr = term[row];
            for (int j = 0; j < m; j++) acc += tr[j];
        }
        __syncthreads();
    }
    if (Q.l < nrows) sh_sum[build ? Q.l : SO_CHI] = acc;
    __syncthreads();
}

// SparseOptimizer::optimize(its) with OptimizationAlgorithmLevenberg
// (optimization_algorithm_levenberg.cpp:61-164) on the active pairs. T is the
// estimate; last_eval the estimate of the last trial evaluated, whose errors
// the edges are left holding. xs is Solver::_x (kept when a factorisation fails).
__device__ __forceinline__ void optimize(const Sim3OptArgs& A, const Problem& Q, int its, Sim3& T, Sim3& last_eval,
                                         double (&xs)[7], int& iters, int& trials, double (*term)[SO_TP],
                                         double (*sims)[8], double (*sinv)[8], double* sh_sum) {
    double lambda = 0, ni = 2;
    int nBad = 0;
    for (int iter = 0; iter < its; iter++) {
        iters++;
        pass(A, Q, T, true, term, sims, sinv, sh_sum);
        double H[49], b[7];
        for (int a = 0, k = 0; a < 7; a++)
            for (int c = 0; c <= a; c++, k++) H[7 * a + c] = H[7 * c + a] = sh_sum[k];
        for (int a = 0; a < 7; a++) b[a] = sh_sum[SO_NH + a];
        double currentChi = sh_sum[SO_CHI];
        const double iniChi = currentChi;
        __syncthreads();  // sh_sum is read before the trials overwrite its chi2
        if (iter == 0) {
            double md = 0;
            for (int j = 0; j < 7; j++) md = fmax(fabs(H[8 * j]), md);
            lambda = 1e-5 * md;
            ni = 2;
            nBad = 0;
        }
        double rho = 0;
        int q = 0;
        do {
            trials++;
            double Hl[49];
            for (int i = 0; i < 49; i++) Hl[i] = H[i];
            for (int j = 0; j < 7; j++) Hl[8 * j] += lambda;
            double xn[7];
            const bool ok = gfse3::ldlt7(Hl, b, xn);
            if (ok)
                for (int j = 0; j < 7; j++) xs[j] = xn[j];
            const Sim3 Tn = sim3_mul(sim3_exp(xs), T);  // oplus: Sim3(update) * estimate
            pass(A, Q, Tn, false, term, sims, sinv, sh_sum);
            double tempChi = sh_sum[SO_CHI];
            __syncthreads();
            last_eval = Tn;
            if (!ok) tempChi = DBL_MAX;
            rho = currentChi - tempChi;
            double scale = 0;
            for (int j = 0; j < 7; j++) scale += xs[j] * (lambda * xs[j] + b[j]);
            scale += 1e-3;
            rho /= scale;
            if (rho > 0 && isfinite(tempChi)) {
                double alpha = 1. - pow((2 * rho - 1), 3.0);
                alpha = fmin(alpha, 2. / 3.);
                const double sf = fmax(1. / 3., alpha);
                lambda *= sf;
                ni = 2;
                currentChi = tempChi;
                T = Tn;
            } else {
                lambda *= ni;
                ni *= 2;
            }
            q++;
        } while (rho < 0 && q < 10);
        if (q == 10 || rho == 0) break;
        if ((iniChi - currentChi) * 1e3 < iniChi)
            nBad++;
        else
            nBad = 0;
        if (nBad >= 3) break;
    }
}

// The inlier check of Optimizer.cc:2158-2177 / :2193-2208 over the active
// pairs. OptimizeSim3 does not call computeError() before chi2(): the errors
// tested are those of the last trial evaluated (`ev`), which is the rejected
// estimate when that trial was popped. Returns the number of pairs dropped.
__device__ __forceinline__ int classify(const Sim3OptArgs& A, const Problem& Q, const Sim3& ev) {
    const Sim3 evi = sim3_inverse(ev);
    int nb = 0;
    for (int b0 = 0; b0 < Q.n; b0 += SO_T) {
        const int e = b0 + Q.l;
        bool bad = false;
        if (e < Q.n && A.inl[Q.base + e]) {
            const Pair P = load_pair(A, Q.base + e);
            double r0, r1;
            err12(P, Q.C, ev, r0, r1);
            const double c12 = r0 * (P.w1 * r0) + r1 * (P.w1 * r1);
            err21(P, Q.C, evi, r0, r1);
            const double c21 = r0 * (P.w2 * r0) + r1 * (P.w2 * r1);
            if (c12 > Q.th2 || c21 > Q.th2) {
                A.inl[Q.base + e] = 0;
                bad = true;
            }
        }
        nb += __syncthreads_count(bad);
    }
    return nb;
}

// Optimizer::OptimizeSim3 (Optimizer.cc:2019-2215) for problem p by one wave.
__device__ __forceinline__ void sim3_opt_problem(const Sim3OptArgs& A, int p) {
    __shared__ double term[SO_ROWS][SO_TP];
    __shared__ double sh_sum[SO_ROWS];
    __shared__ double sims[SO_NSIM][8], sinv[SO_NSIM][8];
    Problem Q;
    Q.l = threadIdx.x;
    Q.base = A.offs[p];
    Q.n = max(A.offs[p + 1] - Q.base, 0);
    const float th2f = A.th2[p];
    Q.th2 = (double)th2f;
    Q.delta = (double)sqrtf(th2f);  // const float deltaHuber = sqrt(th2)
    Q.dsqr = Q.delta * Q.delta;
    const float* K = A.K + 8 * (size_t)p;
    for (int k = 0; k < 2; k++) {
        Q.C.f1[k] = (double)K[k];
        Q.C.c1[k] = (double)K[2 + k];
        Q.C.f2[k] = (double)K[4 + k];
        Q.C.c2[k] = (double)K[6 + k];
    }
    double* est = A.est + 8 * (size_t)p;
    Sim3 T = lds_sim(est);
    for (int e = Q.l; e < Q.n; e += SO_T) A.inl[Q.base + e] = 1;
    __syncthreads();
    int it[2] = {0, 0}, tr[2] = {0, 0}, nIn = 0;
    if (Q.n > 0) {  // no edge: optimize() returns at once and 0 - 0 < 10
        double xs[7] = {0, 0, 0, 0, 0, 0, 0};
        Sim3 last_eval = T;
        optimize(A, Q, 5, T, last_eval, xs, it[0], tr[0], term, sims, sinv, sh_sum);
        const int nBad = classify(A, Q, last_eval);
        __syncthreads();
        if (Q.n - nBad >= 10) {
            optimize(A, Q, nBad > 0 ? 10 : 5, T, last_eval, xs, it[1], tr[1], term, sims, sinv, sh_sum);
            nIn = Q.n - nBad - classify(A, Q, last_eval);
            // g2oS12 = vSim3_recov->estimate(): written on this path only
            if (Q.l == 0) sim_lds(T, est);
        }
    }
    if (Q.l == 0) {
        A.nin[p] = nIn;
        if (A.stats) {
            int32_t* st = A.stats + 4 * (size_t)p;
            st[0] = it[0];
            st[1] = it[1];
            st[2] = tr[0];
            st[3] = tr[1];
        }
    }
}

#endif  // __HIPCC__

}  // namespace
}  // namespace gfsim3opt
