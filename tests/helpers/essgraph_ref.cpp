// CPU restatement of Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:
// 1768-2017) for the tests (tests/test_essgraph_cpu.py, test_essgraph_gpu.py):
// plain scalar C++ written from the reference's text, nothing shared with the
// library's sources. g2o::Sim3 (types/sim3/sim3.h) with exp, log, *, inverse
// and map; EdgeSim3 (types_seven_dof_expmap.h:99-126); BaseBinaryEdge's
// central differences and quadratic form (base_binary_edge.hpp:55-196); the
// modified OptimizationAlgorithmLevenberg::solve (:61-164) with
// setUserLambdaInit(1e-16) and optimize(20). The linear solve is dense: LLt
// (solver 0) or LDLt without pivoting (solver 1). Sets and maps keyed by
// KeyFrame* are walked in keyframe-id order.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <set>
#include <utility>
#include <vector>

#include "../../include/gfslam/abi.h"

namespace {

struct S3 {
    double q[4];  // x y z w
    double t[3];
    double s;
};

S3 load(const double* p) {
    S3 S;
    for (int i = 0; i < 4; i++) S.q[i] = p[i];
    for (int i = 0; i < 3; i++) S.t[i] = p[4 + i];
    S.s = p[7];
    return S;
}
void store(const S3& S, double* p) {
    for (int i = 0; i < 4; i++) p[i] = S.q[i];
    for (int i = 0; i < 3; i++) p[4 + i] = S.t[i];
    p[7] = S.s;
}

// Eigen Quaterniond(Matrix3d)
void quat_of(const double R[3][3], double q[4]) {
    double tr = R[0][0] + (R[1][1] + R[2][2]);  // trace(): Eigen's unrolled reduction splits 3 as 1 + 2
    if (tr > 0) {
        double t = std::sqrt(tr + 1.0);
        q[3] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (R[2][1] - R[1][2]) * t;
        q[1] = (R[0][2] - R[2][0]) * t;
        q[2] = (R[1][0] - R[0][1]) * t;
    } else {
        int i = 0;
        if (R[1][1] > R[0][0]) i = 1;
        if (R[2][2] > R[i][i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        double t = std::sqrt(R[i][i] - R[j][j] - R[k][k] + 1.0);
        q[i] = 0.5 * t;
        t = 0.5 / t;
        q[3] = (R[k][j] - R[j][k]) * t;
        q[j] = (R[j][i] + R[i][j]) * t;
        q[k] = (R[k][i] + R[i][k]) * t;
    }
}

// Eigen toRotationMatrix
void rot_of(const double q[4], double R[3][3]) {
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    const double tx = 2 * x, ty = 2 * y, tz = 2 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w;
    const double txx = tx * x, txy = ty * x, txz = tz * x;
    const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
    R[0][0] = 1 - (tyy + tzz);
    R[0][1] = txy - twz;
    R[0][2] = txz + twy;
    R[1][0] = txy + twz;
    R[1][1] = 1 - (txx + tzz);
    R[1][2] = tyz - twx;
    R[2][0] = txz - twy;
    R[2][1] = tyz + twx;
    R[2][2] = 1 - (txx + tyy);
}

// Eigen quaternion * vector: v + w * 2(q x v) + q x 2(q x v)
void qrot(const double q[4], const double v[3], double o[3]) {
    double u[3] = {q[1] * v[2] - q[2] * v[1], q[2] * v[0] - q[0] * v[2], q[0] * v[1] - q[1] * v[0]};
    for (int i = 0; i < 3; i++) u[i] += u[i];
    o[0] = v[0] + q[3] * u[0] + (q[1] * u[2] - q[2] * u[1]);
    o[1] = v[1] + q[3] * u[1] + (q[2] * u[0] - q[0] * u[2]);
    o[2] = v[2] + q[3] * u[2] + (q[0] * u[1] - q[1] * u[0]);
}

void qmul(const double a[4], const double b[4], double r[4]) {
    r[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
    r[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
    r[1] = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
    r[2] = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
}

S3 mul(const S3& a, const S3& b) {  // sim3.h:266-272
    S3 r;
    qmul(a.q, b.q, r.q);
    double rt[3];
    qrot(a.q, b.t, rt);
    for (int i = 0; i < 3; i++) r.t[i] = a.s * rt[i] + a.t[i];
    r.s = a.s * b.s;
    return r;
}

S3 inverse(const S3& a) {  // :233-236
    S3 r;
    r.q[0] = -a.q[0];
    r.q[1] = -a.q[1];
    r.q[2] = -a.q[2];
    r.q[3] = a.q[3];
    const double f = -1. / a.s;
    const double ft[3] = {f * a.t[0], f * a.t[1], f * a.t[2]};
    qrot(r.q, ft, r.t);
    r.s = 1. / a.s;
    return r;
}

void map(const S3& S, const double p[3], double o[3]) {  // :144-146
    double rp[3];
    qrot(S.q, p, rp);
    for (int i = 0; i < 3; i++) o[i] = S.s * rp[i] + S.t[i];
}

void skew(const double w[3], double O[3][3]) {
    O[0][0] = 0, O[0][1] = -w[2], O[0][2] = w[1];
    O[1][0] = w[2], O[1][1] = 0, O[1][2] = -w[0];
    O[2][0] = -w[1], O[2][1] = w[0], O[2][2] = 0;
}

void mm(const double A[3][3], const double B[3][3], double C[3][3]) {
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) C[i][j] = A[i][0] * B[0][j] + A[i][1] * B[1][j] + A[i][2] * B[2][j];
}

S3 sim_exp(const double u[7]) {  // Sim3(const Vector7d&), :70-142
    const double w[3] = {u[0], u[1], u[2]};
    const double sigma = u[6];
    const double theta = std::sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
    double O[3][3], O2[3][3], R[3][3], W[3][3];
    skew(w, O);
    mm(O, O, O2);
    S3 S;
    S.s = std::exp(sigma);
    const double eps = 0.00001;
    double A, B, C;
    bool plainR = false;
    double ra = 0, rb = 0;
    if (std::fabs(sigma) < eps) {
        C = 1;
        if (theta < eps) {
            A = 1. / 2.;
            B = 1. / 6.;
            plainR = true;
        } else {
            const double theta2 = theta * theta;
            A = (1 - std::cos(theta)) / (theta2);
            B = (theta - std::sin(theta)) / (theta2 * theta);
            ra = std::sin(theta) / theta;
            rb = (1 - std::cos(theta)) / (theta * theta);
        }
    } else {
        C = (S.s - 1) / sigma;
        if (theta < eps) {
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1) * S.s + 1) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1) * S.s) / (sigma2 * sigma);
            plainR = true;
        } else {
            ra = std::sin(theta) / theta;
            rb = (1 - std::cos(theta)) / (theta * theta);
            const double a = S.s * std::sin(theta);
            const double b = S.s * std::cos(theta);
            const double theta2 = theta * theta;
            const double sigma2 = sigma * sigma;
            const double c = theta2 + sigma2;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / (c)) * 1. / (theta2);
        }
    }
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            const double I = i == j ? 1.0 : 0.0;
            R[i][j] = plainR ? (I + O[i][j]) + O2[i][j] : (I + ra * O[i][j]) + rb * O2[i][j];
            W[i][j] = (A * O[i][j] + B * O2[i][j]) + C * I;
        }
    quat_of(R, S.q);
    for (int i = 0; i < 3; i++) S.t[i] = (W[i][0] * u[3] + W[i][1] * u[4]) + W[i][2] * u[5];
    return S;
}

// Eigen PartialPivLU of a 3x3 and its solve
void lu3_solve(double M[3][3], const double b[3], double x[3]) {
    int perm[3] = {0, 1, 2};
    for (int k = 0; k < 3; k++) {
        int piv = k;
        double big = std::fabs(M[k][k]);
        for (int i = k + 1; i < 3; i++)
            if (std::fabs(M[i][k]) > big) big = std::fabs(M[i][k]), piv = i;
        if (piv != k) {
            for (int j = 0; j < 3; j++) std::swap(M[k][j], M[piv][j]);
            std::swap(perm[k], perm[piv]);
        }
        for (int i = k + 1; i < 3; i++) M[i][k] /= M[k][k];
        for (int i = k + 1; i < 3; i++)
            for (int j = k + 1; j < 3; j++) M[i][j] -= M[i][k] * M[k][j];
    }
    double y[3];
    for (int i = 0; i < 3; i++) y[i] = b[perm[i]];
    for (int i = 1; i < 3; i++)
        for (int j = 0; j < i; j++) y[i] -= M[i][j] * y[j];
    for (int i = 2; i >= 0; i--) {
        for (int j = i + 1; j < 3; j++) y[i] -= M[i][j] * y[j];
        y[i] /= M[i][i];
    }
    for (int i = 0; i < 3; i++) x[i] = y[i];
}

void sim_log(const S3& S, double res[7]) {  // :148-230
    const double sigma = std::log(S.s);
    double R[3][3];
    rot_of(S.q, R);
    const double d = 0.5 * (R[0][0] + R[1][1] + R[2][2] - 1);
    const double dR[3] = {R[2][1] - R[1][2], R[0][2] - R[2][0], R[1][0] - R[0][1]};
    double omega[3];
    const double eps = 0.00001;
    double A, B, C;
    if (std::fabs(sigma) < eps) {
        C = 1;
        if (d > 1 - eps) {
            for (int i = 0; i < 3; i++) omega[i] = 0.5 * dR[i];
            A = 1. / 2.;
            B = 1. / 6.;
        } else {
            const double theta = std::acos(d);
            const double theta2 = theta * theta;
            const double f = theta / (2 * std::sqrt(1 - d * d));
            for (int i = 0; i < 3; i++) omega[i] = f * dR[i];
            A = (1 - std::cos(theta)) / (theta2);
            B = (theta - std::sin(theta)) / (theta2 * theta);
        }
    } else {
        C = (S.s - 1) / sigma;
        if (d > 1 - eps) {
            const double sigma2 = sigma * sigma;
            for (int i = 0; i < 3; i++) omega[i] = 0.5 * dR[i];
            A = ((sigma - 1) * S.s + 1) / (sigma2);
            B = ((0.5 * sigma2 - sigma + 1) * S.s) / (sigma2 * sigma);
        } else {
            const double theta = std::acos(d);
            const double f = theta / (2 * std::sqrt(1 - d * d));
            for (int i = 0; i < 3; i++) omega[i] = f * dR[i];
            const double theta2 = theta * theta;
            const double a = S.s * std::sin(theta);
            const double b = S.s * std::cos(theta);
            const double c = theta2 + sigma * sigma;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / (c)) * 1. / (theta2);
        }
    }
    double O[3][3], BO[3][3], BOO[3][3], W[3][3];
    skew(omega, O);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) BO[i][j] = B * O[i][j];
    mm(BO, O, BOO);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) W[i][j] = (A * O[i][j] + BOO[i][j]) + C * (i == j ? 1.0 : 0.0);
    double ups[3];
    lu3_solve(W, S.t, ups);
    for (int i = 0; i < 3; i++) res[i] = omega[i], res[3 + i] = ups[i];
    res[6] = sigma;
}

S3 from_pose(const float* T) {  // g2o::Sim3(Converter::toMatrix3d(R), toVector3d(t), 1.0)
    double R[3][3];
    S3 S;
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) R[i][j] = (double)T[4 * i + j];
        S.t[i] = (double)T[4 * i + 3];
    }
    quat_of(R, S.q);
    S.s = 1.0;
    return S;
}

// EdgeSim3::computeError
void edge_error(const S3& C, const S3& v1, const S3& v2, double e[7]) { sim_log(mul(mul(C, v1), inverse(v2)), e); }

S3 oplus(const S3& est, const double u[7]) { return mul(sim_exp(u), est); }

// linearizeOplus: J[r][d], 7 x 7 each; a fixed vertex keeps zeros
void edge_jac(const S3& C, const S3& v1, const S3& v2, bool fix1, bool fix2, double Ji[49], double Jj[49]) {
    const double delta = 1e-9;
    const double scalar = 1.0 / (2 * delta);
    std::memset(Ji, 0, 49 * sizeof(double));
    std::memset(Jj, 0, 49 * sizeof(double));
    for (int side = 0; side < 2; side++) {
        if (side == 0 ? fix1 : fix2) continue;
        double add[7] = {0, 0, 0, 0, 0, 0, 0};
        for (int d = 0; d < 7; d++) {
            double ep[7], em[7];
            add[d] = delta;
            if (side == 0)
                edge_error(C, oplus(v1, add), v2, ep);
            else
                edge_error(C, v1, oplus(v2, add), ep);
            add[d] = -delta;
            if (side == 0)
                edge_error(C, oplus(v1, add), v2, em);
            else
                edge_error(C, v1, oplus(v2, add), em);
            add[d] = 0.0;
            double* J = side == 0 ? Ji : Jj;
            for (int r = 0; r < 7; r++) J[7 * r + d] = scalar * (ep[r] - em[r]);
        }
    }
}

struct Edge {
    int i, j, kind;
};

int weight_of(const gf_essgraph_problem& P, int i, int j) {
    for (int k = P.cov_start[i]; k < P.cov_start[i + 1]; k++)
        if (P.cov_nbr[k] == j) return P.cov_weight[k];
    return 0;
}

// Optimizer.cc:1832-1957, integer logic only
std::vector<Edge> build_edges(const gf_essgraph_problem& P) {
    const int minFeat = 100;
    std::vector<Edge> E;
    std::set<std::pair<int, int>> inserted;
    std::vector<std::pair<int, std::vector<int>>> lc;
    for (int k = 0; k < P.nlc; k++) {
        std::vector<int> nb(P.lc_nbr + P.lc_start[k], P.lc_nbr + P.lc_start[k + 1]);
        std::set<int> s(nb.begin(), nb.end());
        lc.push_back({P.lc_key[k], std::vector<int>(s.begin(), s.end())});
    }
    std::sort(lc.begin(), lc.end());
    for (auto& kv : lc) {
        const int i = kv.first;
        for (int j : kv.second) {
            if ((i != P.cur_kf || j != P.loop_kf) && weight_of(P, i, j) < minFeat) continue;
            E.push_back({i, j, 0});
            inserted.insert({std::min(i, j), std::max(i, j)});
        }
    }
    for (int i = 0; i < P.nkf; i++) {
        const int par = P.parent[i];
        if (par >= 0) E.push_back({i, par, 1});
        std::set<int> le(P.le_nbr + P.le_start[i], P.le_nbr + P.le_start[i + 1]);
        for (int l : le)
            if (l < i) E.push_back({i, l, 2});
        for (int k = P.cov_start[i]; k < P.cov_start[i + 1] && P.cov_weight[k] >= minFeat; k++) {
            const int n = P.cov_nbr[k];
            if (n != par && P.parent[n] != i && !le.count(n)) {
                if (n < i) {
                    if (inserted.count({std::min(i, n), std::max(i, n)})) continue;
                    E.push_back({i, n, 3});
                }
            }
        }
    }
    return E;
}

bool llt_solve(std::vector<double>& A, int n, const std::vector<double>& b, std::vector<double>& x) {
    for (int j = 0; j < n; j++) {
        double d = A[(size_t)j * n + j];
        for (int k = 0; k < j; k++) d -= A[(size_t)j * n + k] * A[(size_t)j * n + k];
        if (!(d > 0) || !std::isfinite(d)) return false;
        d = std::sqrt(d);
        A[(size_t)j * n + j] = d;
        for (int i = j + 1; i < n; i++) {
            double s = A[(size_t)i * n + j];
            const double *ri = &A[(size_t)i * n], *rj = &A[(size_t)j * n];
            for (int k = 0; k < j; k++) s -= ri[k] * rj[k];
            A[(size_t)i * n + j] = s / d;
        }
    }
    std::vector<double> y(n);
    for (int i = 0; i < n; i++) {
        double s = b[i];
        for (int k = 0; k < i; k++) s -= A[(size_t)i * n + k] * y[k];
        y[i] = s / A[(size_t)i * n + i];
    }
    for (int i = n - 1; i >= 0; i--) {
        double s = y[i];
        for (int k = i + 1; k < n; k++) s -= A[(size_t)k * n + i] * y[k];
        y[i] = s / A[(size_t)i * n + i];
    }
    x = y;
    return true;
}

bool ldlt_solve(std::vector<double>& A, int n, const std::vector<double>& b, std::vector<double>& x) {
    std::vector<double> D(n), v(n);
    for (int j = 0; j < n; j++) {
        double* rj = &A[(size_t)j * n];
        for (int k = 0; k < j; k++) v[k] = rj[k] * D[k];
        double d = rj[j];
        for (int k = 0; k < j; k++) d -= rj[k] * v[k];
        if (!(d > 0) || !std::isfinite(d)) return false;
        D[j] = d;
        for (int i = j + 1; i < n; i++) {
            double* ri = &A[(size_t)i * n];
            double s = ri[j];
            for (int k = 0; k < j; k++) s -= ri[k] * v[k];
            ri[j] = s / d;
        }
    }
    std::vector<double> y(n);
    for (int i = 0; i < n; i++) {
        double s = b[i];
        for (int k = 0; k < i; k++) s -= A[(size_t)i * n + k] * y[k];
        y[i] = s;
    }
    for (int i = 0; i < n; i++) y[i] /= D[i];
    for (int i = n - 1; i >= 0; i--) {
        double s = y[i];
        for (int k = i + 1; k < n; k++) s -= A[(size_t)k * n + i] * y[k];
        y[i] = s;
    }
    x = y;
    return true;
}

}  // namespace

extern "C" {

void egref_exp(const double* u, double* S) { store(sim_exp(u), S); }
void egref_log(const double* S, double* u) { sim_log(load(S), u); }
void egref_mul(const double* a, const double* b, double* r) { store(mul(load(a), load(b)), r); }
void egref_inverse(const double* a, double* r) { store(inverse(load(a)), r); }
void egref_from_pose(const float* T, double* S) { store(from_pose(T), S); }
void egref_edge_error(const double* C, const double* v1, const double* v2, double* e) {
    edge_error(load(C), load(v1), load(v2), e);
}
void egref_edge_jacobian(const double* C, const double* v1, const double* v2, double* Ji, double* Jj) {
    edge_jac(load(C), load(v1), load(v2), false, false, Ji, Jj);
}

int egref_edges(const gf_essgraph_problem* P, int32_t* rows, int cap) {
    const std::vector<Edge> E = build_edges(*P);
    for (size_t e = 0; e < E.size() && (int)e < cap; e++) {
        rows[3 * e] = E[e].i;
        rows[3 * e + 1] = E[e].j;
        rows[3 * e + 2] = E[e].kind;
    }
    return (int)E.size();
}

// solver: 0 LLt, 1 LDLt; reverse: sum chi2 / H / b over the edges last to
// first. jac_edge >= 0: J (98 doubles, Ji then Jj) of that edge at the first
// linearisation. Returns 0.
int egref_solve(const gf_essgraph_problem* Pp, int solver, int reverse, float* Tcw_out, float* pos_out,
                gf_essgraph_stats* st, double* tr_lambda, double* tr_chi, uint8_t* tr_acc, int jac_edge, double* jac) {
    const gf_essgraph_problem& P = *Pp;
    const int N = P.nkf;
    std::vector<int> corr(N, -1);
    for (int c = 0; c < P.ncorr; c++) corr[P.corr_idx[c]] = c;
    std::vector<S3> vScw(N), est(N);
    for (int i = 0; i < N; i++) {
        vScw[i] = corr[i] >= 0 ? load(P.corrected + 8 * corr[i]) : from_pose(P.kf_Tcw + 16 * i);
        est[i] = vScw[i];
    }
    const std::vector<Edge> E = build_edges(P);
    const int ne = (int)E.size();
    std::vector<S3> meas(ne);
    for (int e = 0; e < ne; e++) {
        const int i = E[e].i, j = E[e].j;
        if (E[e].kind == 0) {
            meas[e] = mul(vScw[j], inverse(vScw[i]));
        } else {
            const S3 Swi = inverse(corr[i] >= 0 ? load(P.noncorrected + 8 * corr[i]) : vScw[i]);
            const S3 Sjw = corr[j] >= 0 ? load(P.noncorrected + 8 * corr[j]) : vScw[j];
            meas[e] = mul(Sjw, Swi);
        }
    }
    std::vector<int> hidx(N);
    int nf = 0;
    for (int i = 0; i < N; i++) hidx[i] = i == P.loop_kf ? -1 : nf++;
    const int n = 7 * nf;

    auto chi2_of = [&](const std::vector<S3>& v) {
        double chi = 0;
        for (int k = 0; k < ne; k++) {
            const int e = reverse ? ne - 1 - k : k;
            double r[7];
            edge_error(meas[e], v[E[e].i], v[E[e].j], r);
            double c = 0;
            for (int a = 0; a < 7; a++) c += r[a] * r[a];
            chi += c;
        }
        return chi;
    };

    std::vector<double> H((size_t)n * n), b(n), x(n, 0.0), Hl;
    double lambda = 0, ni = 2;
    int nBad = 0, iters = 0, trials = 0, stop = 0, ntr = 0;
    double chi_first = 0, currentChi = 0;
    for (int iter = 0; iter < 20; iter++) {
        iters++;
        currentChi = chi2_of(est);
        if (iter == 0) chi_first = currentChi;
        const double iniChi = currentChi;
        std::fill(H.begin(), H.end(), 0.0);
        std::fill(b.begin(), b.end(), 0.0);
        for (int k = 0; k < ne; k++) {
            const int e = reverse ? ne - 1 - k : k;
            const int i = E[e].i, j = E[e].j;
            double r[7], Ji[49], Jj[49];
            edge_error(meas[e], est[i], est[j], r);
            edge_jac(meas[e], est[i], est[j], hidx[i] < 0, hidx[j] < 0, Ji, Jj);
            if (iter == 0 && e == jac_edge && jac) {
                std::memcpy(jac, Ji, sizeof(Ji));
                std::memcpy(jac + 49, Jj, sizeof(Jj));
            }
            const double* J[2] = {Ji, Jj};
            const int h[2] = {hidx[i], hidx[j]};
            for (int a = 0; a < 2; a++) {
                if (h[a] < 0) continue;
                for (int p = 0; p < 7; p++) {
                    double s = 0;
                    for (int q = 0; q < 7; q++) s += J[a][7 * q + p] * -r[q];
                    b[7 * h[a] + p] += s;
                }
                for (int c = 0; c < 2; c++) {
                    if (h[c] < 0) continue;
                    for (int p = 0; p < 7; p++)
                        for (int q = 0; q < 7; q++) {
                            double s = 0;
                            for (int m = 0; m < 7; m++) s += J[a][7 * m + p] * J[c][7 * m + q];
                            H[(size_t)(7 * h[a] + p) * n + 7 * h[c] + q] += s;
                        }
                }
            }
        }
        if (iter == 0) {
            lambda = 1e-16;  // setUserLambdaInit
            ni = 2;
            nBad = 0;
        }
        double rho = 0;
        int q = 0;
        do {
            trials++;
            Hl = H;
            for (int k = 0; k < n; k++) Hl[(size_t)k * n + k] += lambda;
            const bool ok = solver == 0 ? llt_solve(Hl, n, b, x) : ldlt_solve(Hl, n, b, x);
            std::vector<S3> trial = est;
            for (int i = 0; i < N; i++)
                if (hidx[i] >= 0) trial[i] = oplus(est[i], &x[7 * hidx[i]]);
            double tempChi = chi2_of(trial);
            if (!ok) tempChi = DBL_MAX;
            rho = currentChi - tempChi;
            double scale = 0;
            for (int k = 0; k < n; k++) scale += x[k] * (lambda * x[k] + b[k]);
            scale += 1e-3;
            rho /= scale;
            const bool good = rho > 0 && std::isfinite(tempChi);
            if (ntr < GF_ESSGRAPH_TRACE) {
                if (tr_lambda) tr_lambda[ntr] = lambda;
                if (tr_chi) tr_chi[ntr] = tempChi;
                if (tr_acc) tr_acc[ntr] = good;
                ntr++;
            }
            if (good) {
                double alpha = 1. - std::pow((2 * rho - 1), 3);
                alpha = std::min(alpha, 2. / 3.);
                const double sf = std::max(1. / 3., alpha);
                lambda *= sf;
                ni = 2;
                currentChi = tempChi;
                est = trial;
            } else {
                lambda *= ni;
                ni *= 2;
            }
            q++;
        } while (rho < 0 && q < 10);
        if (q == 10 || rho == 0) {
            stop = rho == 0 ? 1 : 2;
            break;
        }
        if ((iniChi - currentChi) * 1e3 < iniChi)
            nBad++;
        else
            nBad = 0;
        if (nBad >= 3) {
            stop = 3;
            break;
        }
    }
    if (st) {
        st->iterations = iters;
        st->trials = trials;
        st->stop = stop;
        st->ntrace = ntr;
        st->chi2_initial = chi_first;
        st->chi2_final = currentChi;
    }
    // :1964-1983
    for (int i = 0; i < N; i++) {
        double R[3][3];
        rot_of(est[i].q, R);
        const double is = 1. / est[i].s;
        float* T = Tcw_out + 16 * i;
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) T[4 * r + c] = (float)R[r][c];
            T[4 * r + 3] = (float)(est[i].t[r] * is);
        }
        T[12] = T[13] = T[14] = 0.f;
        T[15] = 1.f;
    }
    // :1985-2016
    for (int m = 0; m < P.npts; m++) {
        for (int k = 0; k < 3; k++) pos_out[3 * m + k] = P.pt_pos[3 * m + k];
        if (P.pt_bad[m]) continue;
        const int r = P.pt_corrected_ref[m] >= 0 ? P.pt_corrected_ref[m] : P.pt_ref[m];
        if (r < 0) continue;
        const double p[3] = {(double)P.pt_pos[3 * m], (double)P.pt_pos[3 * m + 1], (double)P.pt_pos[3 * m + 2]};
        double a[3], c[3];
        map(vScw[r], p, a);
        map(inverse(est[r]), a, c);
        for (int k = 0; k < 3; k++) pos_out[3 * m + k] = (float)c[k];
    }
    return 0;
}

}  // extern "C"
