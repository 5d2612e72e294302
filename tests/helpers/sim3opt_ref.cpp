// CPU restatement of Optimizer::OptimizeSim3 (src/Optimizer.cc:2019-2215) and
// of ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th)
// (src/ORBmatcher.cc:855-977) for the tests (tests/test_sim3_optimize.py),
// written from the reference and its g2o directly: scalar C++, a vertex with
// a push/pop stack, edge objects that keep their own _error and Jacobian as
// g2o's do, an optimizer that walks its active-edge vector. No project header
// but abi.h (struct layouts). The Eigen readings (quaternion from matrix,
// quaternion * vector, 7x7 LDLT) follow docs/ORACLE_ASSUMPTIONS.md A23.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <set>
#include <vector>

#include "../../include/gfslam/abi.h"

namespace {

struct V3 {
    double v[3];
    double& operator[](int i) { return v[i]; }
    double operator[](int i) const { return v[i]; }
};
struct M3 {
    double m[3][3];
};

M3 mat_mul(const M3& a, const M3& b) {
    M3 r;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) r.m[i][j] = a.m[i][0] * b.m[0][j] + a.m[i][1] * b.m[1][j] + a.m[i][2] * b.m[2][j];
    return r;
}

// Eigen::Quaterniond: coefficients x y z w
struct Quat {
    double x, y, z, w;
    // QuaternionBase::operator=(Matrix3): the trace branch
    static Quat fromMatrix(const M3& mat) {
        Quat q;
        double t = mat.m[0][0] + (mat.m[1][1] + mat.m[2][2]);  // trace() of a fixed 3x3: redux order
        if (t > 0) {
            t = std::sqrt(t + 1.0);
            q.w = 0.5 * t;
            t = 0.5 / t;
            q.x = (mat.m[2][1] - mat.m[1][2]) * t;
            q.y = (mat.m[0][2] - mat.m[2][0]) * t;
            q.z = (mat.m[1][0] - mat.m[0][1]) * t;
        } else {
            int i = 0;
            if (mat.m[1][1] > mat.m[0][0]) i = 1;
            if (mat.m[2][2] > mat.m[i][i]) i = 2;
            int j = (i + 1) % 3, k = (j + 1) % 3;
            t = std::sqrt(mat.m[i][i] - mat.m[j][j] - mat.m[k][k] + 1.0);
            double c[3];
            c[i] = 0.5 * t;
            t = 0.5 / t;
            q.w = (mat.m[k][j] - mat.m[j][k]) * t;
            c[j] = (mat.m[j][i] + mat.m[i][j]) * t;
            c[k] = (mat.m[k][i] + mat.m[i][k]) * t;
            q.x = c[0], q.y = c[1], q.z = c[2];
        }
        return q;
    }
    Quat conjugate() const { return Quat{-x, -y, -z, w}; }
    // QuaternionBase::_transformVector: uv = 2 * vec x v; v + w * uv + vec x uv
    V3 operator*(const V3& v) const {
        V3 uv = {{y * v[2] - z * v[1], z * v[0] - x * v[2], x * v[1] - y * v[0]}};
        uv[0] += uv[0], uv[1] += uv[1], uv[2] += uv[2];
        V3 c = {{y * uv[2] - z * uv[1], z * uv[0] - x * uv[2], x * uv[1] - y * uv[0]}};
        return V3{{v[0] + w * uv[0] + c[0], v[1] + w * uv[1] + c[1], v[2] + w * uv[2] + c[2]}};
    }
    // quat_product<double>
    Quat operator*(const Quat& b) const {
        return Quat{w * b.x + x * b.w + y * b.z - z * b.y, w * b.y + y * b.w + z * b.x - x * b.z,
                    w * b.z + z * b.w + x * b.y - y * b.x, w * b.w - x * b.x - y * b.y - z * b.z};
    }
};

// g2o::Sim3 (types/sim3/sim3.h)
struct Sim3 {
    Quat r;
    V3 t;
    double s;
    Sim3() : r{0, 0, 0, 1}, t{{0, 0, 0}}, s(1.) {}
    Sim3(const Quat& r_, const V3& t_, double s_) : r(r_), t(t_), s(s_) {}
    explicit Sim3(const double* update) {  // :70-142
        V3 omega = {{update[0], update[1], update[2]}}, upsilon = {{update[3], update[4], update[5]}};
        double sigma = update[6];
        double theta = std::sqrt((omega[0] * omega[0] + omega[1] * omega[1]) + omega[2] * omega[2]);
        M3 Omega = {{{0, -omega[2], omega[1]}, {omega[2], 0, -omega[0]}, {-omega[1], omega[0], 0}}};
        s = std::exp(sigma);
        M3 Omega2 = mat_mul(Omega, Omega);
        M3 I = {{{1, 0, 0}, {0, 1, 0}, {0, 0, 1}}};
        M3 R;
        double eps = 0.00001;
        double A, B, C;
        auto lin = [&](double a, double b) {  // I + a*Omega + b*Omega2
            M3 o;
            for (int i = 0; i < 3; i++)
                for (int j = 0; j < 3; j++) o.m[i][j] = (I.m[i][j] + a * Omega.m[i][j]) + b * Omega2.m[i][j];
            return o;
        };
        auto plain = [&]() {  // I + Omega + Omega*Omega
            M3 o;
            for (int i = 0; i < 3; i++)
                for (int j = 0; j < 3; j++) o.m[i][j] = (I.m[i][j] + Omega.m[i][j]) + Omega2.m[i][j];
            return o;
        };
        if (std::fabs(sigma) < eps) {
            C = 1;
            if (theta < eps) {
                A = 1. / 2.;
                B = 1. / 6.;
                R = plain();
            } else {
                double theta2 = theta * theta;
                A = (1 - std::cos(theta)) / (theta2);
                B = (theta - std::sin(theta)) / (theta2 * theta);
                R = lin(std::sin(theta) / theta, (1 - std::cos(theta)) / (theta * theta));
            }
        } else {
            C = (s - 1) / sigma;
            if (theta < eps) {
                double sigma2 = sigma * sigma;
                A = ((sigma - 1) * s + 1) / sigma2;
                B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma);
                R = plain();
            } else {
                R = lin(std::sin(theta) / theta, (1 - std::cos(theta)) / (theta * theta));
                double a = s * std::sin(theta);
                double b = s * std::cos(theta);
                double theta2 = theta * theta;
                double sigma2 = sigma * sigma;
                double c = theta2 + sigma2;
                A = (a * sigma + (1 - b) * theta) / (theta * c);
                B = (C - ((b - 1) * sigma + a * theta) / (c)) * 1. / (theta2);
            }
        }
        r = Quat::fromMatrix(R);
        for (int i = 0; i < 3; i++) {
            double W[3];
            for (int j = 0; j < 3; j++) W[j] = (A * Omega.m[i][j] + B * Omega2.m[i][j]) + C * I.m[i][j];
            t[i] = (W[0] * upsilon[0] + W[1] * upsilon[1]) + W[2] * upsilon[2];
        }
    }
    V3 map(const V3& xyz) const {
        V3 q = r * xyz;
        return V3{{s * q[0] + t[0], s * q[1] + t[1], s * q[2] + t[2]}};
    }
    Sim3 inverse() const {
        double f = -1. / s;
        return Sim3(r.conjugate(), r.conjugate() * V3{{f * t[0], f * t[1], f * t[2]}}, 1. / s);
    }
    Sim3 operator*(const Sim3& o) const {
        Sim3 ret;
        ret.r = r * o.r;
        V3 q = r * o.t;
        for (int i = 0; i < 3; i++) ret.t[i] = s * q[i] + t[i];
        ret.s = s * o.s;
        return ret;
    }
};

// VertexSim3Expmap with BaseVertex's backup stack
struct Vertex {
    Sim3 est;
    std::vector<Sim3> stack;
    double f1[2], c1[2], f2[2], c2[2];
    void push() { stack.push_back(est); }
    void pop() {
        est = stack.back();
        stack.pop_back();
    }
    void discardTop() { stack.pop_back(); }
    void oplus(const double* u) { est = Sim3(u) * est; }
};

// EdgeSim3ProjectXYZ (inverse == false) / EdgeInverseSim3ProjectXYZ, point vertex fixed
struct Edge {
    bool inverse;
    V3 X;
    double obs[2], info;
    double err[2];
    double J[2][7];
    void computeError(const Vertex& v) {
        V3 p = inverse ? v.est.inverse().map(X) : v.est.map(X);
        double px = p[0] / p[2], py = p[1] / p[2];
        if (inverse) {
            err[0] = obs[0] - (px * v.f2[0] + v.c2[0]);
            err[1] = obs[1] - (py * v.f2[1] + v.c2[1]);
        } else {
            err[0] = obs[0] - (px * v.f1[0] + v.c1[0]);
            err[1] = obs[1] - (py * v.f1[1] + v.c1[1]);
        }
    }
    double chi2() const { return err[0] * (info * err[0]) + err[1] * (info * err[1]); }
    // BaseBinaryEdge::linearizeOplus (base_binary_edge.hpp:147-196)
    void linearizeOplus(Vertex& v) {
        const double delta = 1e-9;
        const double scalar = 1.0 / (2 * delta);
        double before[2] = {err[0], err[1]};
        double add[7] = {0, 0, 0, 0, 0, 0, 0};
        for (int d = 0; d < 7; ++d) {
            v.push();
            add[d] = delta;
            v.oplus(add);
            computeError(v);
            double bak[2] = {err[0], err[1]};
            v.pop();
            v.push();
            add[d] = -delta;
            v.oplus(add);
            computeError(v);
            bak[0] -= err[0];
            bak[1] -= err[1];
            v.pop();
            add[d] = 0.0;
            J[0][d] = scalar * bak[0];
            J[1][d] = scalar * bak[1];
        }
        err[0] = before[0];
        err[1] = before[1];
    }
};

void huber(double e, double delta, double* rho) {  // RobustKernelHuber::robustify
    double dsqr = delta * delta;
    if (e <= dsqr) {
        rho[0] = e;
        rho[1] = 1.;
        rho[2] = 0.;
    } else {
        double sqrte = std::sqrt(e);
        rho[0] = 2 * sqrte * delta - dsqr;
        rho[1] = delta / sqrte;
        rho[2] = -0.5 * rho[1] / e;
    }
}

// Eigen::LDLT<MatrixXd> (lower, diagonal pivoting) of the N x N matrix + solve
struct LDLT {
    int N;
    std::vector<double> A;
    std::vector<int> tr;
    int sign;  // 0 zero, 1 psd, 2 nsd, 3 indefinite
    double& at(int i, int j) { return A[i * N + j]; }
    void compute(const double* H, int n) {
        N = n;
        A.assign(H, H + n * n);
        tr.assign(n, 0);
        sign = 0;
        std::vector<double> temp(n);
        for (int k = 0; k < n; k++) {
            int big = k;
            double bv = std::fabs(at(k, k));
            for (int i = k + 1; i < n; i++)
                if (std::fabs(at(i, i)) > bv) bv = std::fabs(at(i, i)), big = i;
            tr[k] = big;
            if (k != big) {
                for (int j = 0; j < k; j++) std::swap(at(k, j), at(big, j));
                for (int i = big + 1; i < n; i++) std::swap(at(i, k), at(i, big));
                std::swap(at(k, k), at(big, big));
                for (int i = k + 1; i < big; i++) std::swap(at(i, k), at(big, i));
            }
            if (k > 0) {
                for (int j = 0; j < k; j++) temp[j] = at(j, j) * at(k, j);
                double s = 0;
                for (int j = 0; j < k; j++) s += at(k, j) * temp[j];
                at(k, k) -= s;
                for (int i = k + 1; i < n; i++) {
                    double t = 0;
                    for (int j = 0; j < k; j++) t += at(i, j) * temp[j];
                    at(i, k) -= t;
                }
            }
            double akk = at(k, k);
            bool valid = std::fabs(akk) > 0;
            if (k == 0 && !valid) {
                sign = 0;
                for (int j = 0; j < n; j++) tr[j] = j;
                return;
            }
            if (valid)
                for (int i = k + 1; i < n; i++) at(i, k) /= akk;
            if (sign == 1) {
                if (akk < 0) sign = 3;
            } else if (sign == 2) {
                if (akk > 0) sign = 3;
            } else if (sign == 0) {
                if (akk > 0)
                    sign = 1;
                else if (akk < 0)
                    sign = 2;
            }
        }
    }
    bool isPositive() const { return sign == 1 || sign == 0; }
    void solve(const double* b, double* x) {
        std::vector<double> y(b, b + N);
        for (int k = 0; k < N; k++) std::swap(y[k], y[tr[k]]);
        for (int j = 0; j < N; j++)
            for (int i = j + 1; i < N; i++) y[i] -= at(i, j) * y[j];
        for (int i = 0; i < N; i++) y[i] = std::fabs(at(i, i)) > std::numeric_limits<double>::min() ? y[i] / at(i, i) : 0.0;
        for (int i = N - 1; i >= 0; i--) {
            double s = 0;
            for (int k = i + 1; k < N; k++) s += at(k, i) * y[k];
            y[i] -= s;
        }
        for (int k = N - 1; k >= 0; k--) std::swap(y[k], y[tr[k]]);
        for (int i = 0; i < N; i++) x[i] = y[i];
    }
};

// SparseOptimizer + BlockSolverX + LinearSolverDense + OptimizationAlgorithmLevenberg
// over the one free vertex
struct Optimizer {
    Vertex v;
    std::vector<Edge*> active;
    double delta;  // Huber
    double H[49], b[7], x[7];
    double lambda, ni;
    int nBad;
    Optimizer() { std::memset(x, 0, sizeof x); }

    void computeActiveErrors() {
        for (Edge* e : active) e->computeError(v);
    }
    double activeRobustChi2() {
        double chi = 0.0;
        for (Edge* e : active) {
            double rho[3];
            huber(e->chi2(), delta, rho);
            chi += rho[0];
        }
        return chi;
    }
    void buildSystem() {
        std::memset(H, 0, sizeof H);
        std::memset(b, 0, sizeof b);
        for (Edge* e : active) {
            e->linearizeOplus(v);
            // constructQuadraticForm (base_binary_edge.hpp:55-122), robust branch
            double omega_r[2] = {-(e->info * e->err[0]), -(e->info * e->err[1])};
            double rho[3];
            huber(e->chi2(), delta, rho);
            double w = rho[1] * e->info;
            omega_r[0] *= rho[1];
            omega_r[1] *= rho[1];
            for (int a = 0; a < 7; a++) {
                b[a] += e->J[0][a] * omega_r[0] + e->J[1][a] * omega_r[1];
                for (int c = 0; c < 7; c++) H[7 * a + c] += (e->J[0][a] * w) * e->J[0][c] + (e->J[1][a] * w) * e->J[1][c];
            }
        }
    }
    // OptimizationAlgorithmLevenberg::solve (:61-164); true = OK, false = Terminate
    bool solve(int iteration, int& trials) {
        computeActiveErrors();
        double currentChi = activeRobustChi2();
        double tempChi = currentChi;
        double iniChi = currentChi;
        buildSystem();
        if (iteration == 0) {
            double maxDiagonal = 0.;
            for (int j = 0; j < 7; ++j) maxDiagonal = std::max(std::fabs(H[8 * j]), maxDiagonal);
            lambda = 1e-5 * maxDiagonal;
            ni = 2;
            nBad = 0;
        }
        double rho = 0;
        int qmax = 0;
        do {
            v.push();
            trials++;
            double Hl[49];
            std::memcpy(Hl, H, sizeof H);
            for (int j = 0; j < 7; j++) Hl[8 * j] += lambda;
            LDLT ch;
            ch.compute(Hl, 7);
            bool ok2 = ch.isPositive();
            if (ok2) ch.solve(b, x);
            v.oplus(x);
            computeActiveErrors();
            tempChi = activeRobustChi2();
            if (!ok2) tempChi = std::numeric_limits<double>::max();
            rho = (currentChi - tempChi);
            double scale = 0.;
            for (int j = 0; j < 7; j++) scale += x[j] * (lambda * x[j] + b[j]);
            scale += 1e-3;
            rho /= scale;
            if (rho > 0 && std::isfinite(tempChi)) {
                double alpha = 1. - std::pow((2 * rho - 1), 3);
                alpha = (std::min)(alpha, 2. / 3.);
                double scaleFactor = (std::max)(1. / 3., alpha);
                lambda *= scaleFactor;
                ni = 2;
                currentChi = tempChi;
                v.discardTop();
            } else {
                lambda *= ni;
                ni *= 2;
                v.pop();
            }
            qmax++;
        } while (rho < 0 && qmax < 10);
        if (qmax == 10 || rho == 0) return false;
        if ((iniChi - currentChi) * 1e3 < iniChi)
            nBad++;
        else
            nBad = 0;
        if (nBad >= 3) return false;
        return true;
    }
    // SparseOptimizer::optimize: nothing to do without an active vertex
    // -> true when the loop ran out of iterations (the last solve returned OK,
    // so a larger count would have run another one), false on Terminate
    bool optimize(int iterations, int& its, int& trials) {
        if (active.empty()) return false;
        bool ok = true;
        for (int i = 0; i < iterations && ok; i++) {
            its++;
            ok = solve(i, trials);
        }
        return ok;
    }
};

}  // namespace

extern "C" {

// -> nIn. stats: iterations run in round 1 / 2, LM trials of round 1 / 2, the
// iteration count asked of round 2 (0 when the routine returned before it),
// nBad of the first check, and for round 1 / 2 whether optimize() ended on its
// iteration count and not on a Terminate of the LM. chi2: n x 4 = chi2(e12), chi2(e21) at the first
// check and at the second (NaN where the pair was not tested).
int sim3optref_optimize(int n, const float* X1, const float* X2, const float* z1, const float* z2, const float* w1,
                        const float* w2, const float* K1, const float* K2, float th2, double* S12, uint8_t* inlier,
                        int32_t* stats, double* chi2) {
    Optimizer opt;
    Vertex& v = opt.v;
    v.est = Sim3(Quat{S12[0], S12[1], S12[2], S12[3]}, V3{{S12[4], S12[5], S12[6]}}, S12[7]);
    for (int k = 0; k < 2; k++) {
        v.f1[k] = K1[k], v.c1[k] = K1[2 + k];
        v.f2[k] = K2[k], v.c2[k] = K2[2 + k];
    }
    const float deltaHuber = std::sqrt(th2);
    opt.delta = deltaHuber;
    std::vector<Edge> e12(n), e21(n);
    std::vector<bool> alive(n, true);
    for (int i = 0; i < n; i++) {
        e12[i].inverse = false;
        e12[i].X = V3{{X2[3 * i], X2[3 * i + 1], X2[3 * i + 2]}};
        e12[i].obs[0] = z1[2 * i], e12[i].obs[1] = z1[2 * i + 1];
        e12[i].info = w1[i];
        e21[i].inverse = true;
        e21[i].X = V3{{X1[3 * i], X1[3 * i + 1], X1[3 * i + 2]}};
        e21[i].obs[0] = z2[2 * i], e21[i].obs[1] = z2[2 * i + 1];
        e21[i].info = w2[i];
        e12[i].err[0] = e12[i].err[1] = e21[i].err[0] = e21[i].err[1] = 0;
        inlier[i] = 1;
        for (int k = 0; k < 4; k++) chi2[4 * i + k] = std::numeric_limits<double>::quiet_NaN();
    }
    for (int k = 0; k < 8; k++) stats[k] = 0;
    auto initialize = [&]() {
        opt.active.clear();
        for (int i = 0; i < n; i++)
            if (alive[i]) {
                opt.active.push_back(&e12[i]);
                opt.active.push_back(&e21[i]);
            }
    };
    initialize();
    stats[6] = opt.optimize(5, stats[0], stats[2]);
    int nBad = 0;
    for (int i = 0; i < n; i++) {
        chi2[4 * i] = e12[i].chi2();
        chi2[4 * i + 1] = e21[i].chi2();
        if (e12[i].chi2() > th2 || e21[i].chi2() > th2) {
            inlier[i] = 0;
            alive[i] = false;
            nBad++;
        }
    }
    stats[5] = nBad;
    int nMoreIterations = nBad > 0 ? 10 : 5;
    if (n - nBad < 10) return 0;
    stats[4] = nMoreIterations;
    initialize();
    stats[7] = opt.optimize(nMoreIterations, stats[1], stats[3]);
    int nIn = 0;
    for (int i = 0; i < n; i++) {
        if (!alive[i]) continue;
        chi2[4 * i + 2] = e12[i].chi2();
        chi2[4 * i + 3] = e21[i].chi2();
        if (e12[i].chi2() > th2 || e21[i].chi2() > th2)
            inlier[i] = 0;
        else
            nIn++;
    }
    const Sim3& s = v.est;
    S12[0] = s.r.x, S12[1] = s.r.y, S12[2] = s.r.z, S12[3] = s.r.w;
    S12[4] = s.t[0], S12[5] = s.t[1], S12[6] = s.t[2], S12[7] = s.s;
    return nIn;
}

// The central-difference Jacobians (2 x 7, row-major) of the two edges of one
// pair at S12, as linearizeOplus leaves them.
void sim3optref_jacobian(const double* S12, const double* X1, const double* X2, const double* K1, const double* K2,
                         double* J12, double* J21) {
    Vertex v;
    v.est = Sim3(Quat{S12[0], S12[1], S12[2], S12[3]}, V3{{S12[4], S12[5], S12[6]}}, S12[7]);
    for (int k = 0; k < 2; k++) {
        v.f1[k] = K1[k], v.c1[k] = K1[2 + k];
        v.f2[k] = K2[k], v.c2[k] = K2[2 + k];
    }
    Edge a, b;
    a.inverse = false, a.X = V3{{X2[0], X2[1], X2[2]}}, a.obs[0] = a.obs[1] = 0, a.info = 1;
    b.inverse = true, b.X = V3{{X1[0], X1[1], X1[2]}}, b.obs[0] = b.obs[1] = 0, b.info = 1;
    a.computeError(v);
    b.computeError(v);
    a.linearizeOplus(v);
    b.linearizeOplus(v);
    std::memcpy(J12, a.J, sizeof a.J);
    std::memcpy(J21, b.J, sizeof b.J);
}

// mScw of LoopClosing.cc:343-345: gSmw(R, t, 1.0) from the keyframe's float
// pose, mg2oScw = gScm * gSmw, Converter::toCvMat(g2o::Sim3) = (s * R | t)
// with R = toRotationMatrix(), cast to float. gScw (8 doubles) may be null.
void sim3optref_scw(const double* gScm, const float* Tmw, float* Scw, double* gScw) {
    M3 Rm;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) Rm.m[i][j] = Tmw[4 * i + j];
    Sim3 a(Quat{gScm[0], gScm[1], gScm[2], gScm[3]}, V3{{gScm[4], gScm[5], gScm[6]}}, gScm[7]);
    Sim3 b(Quat::fromMatrix(Rm), V3{{Tmw[3], Tmw[7], Tmw[11]}}, 1.0);
    Sim3 g = a * b;
    // Eigen::QuaternionBase::toRotationMatrix
    const Quat& q = g.r;
    const double tx = 2 * q.x, ty = 2 * q.y, tz = 2 * q.z;
    const double twx = tx * q.w, twy = ty * q.w, twz = tz * q.w;
    const double txx = tx * q.x, txy = ty * q.x, txz = tz * q.x;
    const double tyy = ty * q.y, tyz = tz * q.y, tzz = tz * q.z;
    const double R[9] = {1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz),
                         tyz - twx,       txz - twy, tyz + twx, 1 - (txx + tyy)};
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) Scw[4 * i + j] = (float)(g.s * R[3 * i + j]);
        Scw[4 * i + 3] = (float)g.t[i];
    }
    Scw[12] = Scw[13] = Scw[14] = 0.f;
    Scw[15] = 1.f;
    if (gScw) {
        gScw[0] = q.x, gScw[1] = q.y, gScw[2] = q.z, gScw[3] = q.w;
        gScw[4] = g.t[0], gScw[5] = g.t[1], gScw[6] = g.t[2], gScw[7] = g.s;
    }
}

// Quaterniond(Matrix3d) of a row-major float rotation -> x y z w
void sim3optref_quat_from_R(const float* R, double* q) {
    M3 m;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) m.m[i][j] = R[3 * i + j];
    Quat r = Quat::fromMatrix(m);
    q[0] = r.x, q[1] = r.y, q[2] = r.z, q[3] = r.w;
}

// ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) -> nmatches.
// Map points are ids into mps; vpMatched holds ids, -1 = NULL.
int sim3optref_search_projection(const gf_frame_info* fi, const float* Scw, const gf_keypoint* kps, const uint8_t* desc,
                                 int n, const gf_map_point* mps, const uint8_t* mp_desc, const uint8_t* mp_bad,
                                 const int32_t* points, int npoints, int32_t* vpMatched, int th) {
    const float fx = fi->fx, fy = fi->fy, cx = fi->cx, cy = fi->cy;
    const int nMaxLevel = fi->nlevels - 1;
    std::vector<float> vfScaleFactors(fi->nlevels);
    vfScaleFactors[0] = 1.0f;
    for (int i = 1; i < fi->nlevels; i++) vfScaleFactors[i] = vfScaleFactors[i - 1] * fi->scale_factor;
    // the keyframe grid (KeyFrame ctor copies Frame's: 64 x 48 cells, round())
    const int COLS = 64, ROWS = 48;
    const float invW = (float)COLS / (float)(fi->max_x - fi->min_x), invH = (float)ROWS / (float)(fi->max_y - fi->min_y);
    std::vector<std::vector<size_t>> grid(COLS * ROWS);
    for (int i = 0; i < n; i++) {
        int px = (int)std::round((kps[i].x - fi->min_x) * invW), py = (int)std::round((kps[i].y - fi->min_y) * invH);
        if (px < 0 || px >= COLS || py < 0 || py >= ROWS) continue;
        grid[px * ROWS + py].push_back(i);
    }
    // Decompose Scw
    double d0 = 0;
    for (int k = 0; k < 3; k++) d0 += (double)Scw[k] * (double)Scw[k];
    const float scw = std::sqrt(d0);
    const float inv = (float)(1. / scw);  // Mat / scalar: one factor (A22)
    float Rcw[3][3], tcw[3], Ow[3];
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) Rcw[r][c] = Scw[4 * r + c] * inv;
        tcw[r] = Scw[4 * r + 3] * inv;
    }
    for (int r = 0; r < 3; r++) {
        float acc = Rcw[0][r] * tcw[0];
        acc += Rcw[1][r] * tcw[1];
        acc += Rcw[2][r] * tcw[2];
        Ow[r] = -acc;
    }
    std::set<int> spAlreadyFound(vpMatched, vpMatched + n);
    spAlreadyFound.erase(-1);
    int nmatches = 0;
    for (int iMP = 0; iMP < npoints; iMP++) {
        const int pMP = points[iMP];
        if ((mp_bad && mp_bad[pMP]) || spAlreadyFound.count(pMP)) continue;
        const gf_map_point& P = mps[pMP];
        float p3Dc[3];
        for (int r = 0; r < 3; r++) {
            float acc = Rcw[r][0] * P.pos[0];
            acc += Rcw[r][1] * P.pos[1];
            acc += Rcw[r][2] * P.pos[2];
            p3Dc[r] = acc + tcw[r];
        }
        if (p3Dc[2] < 0.0) continue;
        const float invz = 1 / p3Dc[2];
        const float x = p3Dc[0] * invz, y = p3Dc[1] * invz;
        const float u = fx * x + cx, v = fy * y + cy;
        if (!(u >= fi->min_x && u < fi->max_x && v >= fi->min_y && v < fi->max_y)) continue;
        const float maxDistance = P.max_dist, minDistance = P.min_dist;
        float PO[3] = {P.pos[0] - Ow[0], P.pos[1] - Ow[1], P.pos[2] - Ow[2]};
        double sq = 0, dot = 0;
        for (int k = 0; k < 3; k++) {
            sq += (double)PO[k] * (double)PO[k];
            dot += (double)PO[k] * (double)P.normal[k];
        }
        const float dist = std::sqrt(sq);
        if (dist < minDistance || dist > maxDistance) continue;
        if (dot < 0.5 * dist) continue;
        const float ratio = dist / minDistance;
        int lb = std::lower_bound(vfScaleFactors.begin(), vfScaleFactors.end(), ratio) - vfScaleFactors.begin();
        const int nPredictedLevel = std::min(lb, nMaxLevel);
        const float radius = th * vfScaleFactors[nPredictedLevel];
        // KeyFrame::GetFeaturesInArea
        std::vector<size_t> vIndices;
        do {
            int nMinCellX = std::max(0, (int)std::floor((u - fi->min_x - radius) * invW));
            if (nMinCellX >= COLS) break;
            int nMaxCellX = std::min(COLS - 1, (int)std::ceil((u - fi->min_x + radius) * invW));
            if (nMaxCellX < 0) break;
            int nMinCellY = std::max(0, (int)std::floor((v - fi->min_y - radius) * invH));
            if (nMinCellY >= ROWS) break;
            int nMaxCellY = std::min(ROWS - 1, (int)std::ceil((v - fi->min_y + radius) * invH));
            if (nMaxCellY < 0) break;
            for (int ix = nMinCellX; ix <= nMaxCellX; ix++)
                for (int iy = nMinCellY; iy <= nMaxCellY; iy++)
                    for (size_t j : grid[ix * ROWS + iy])
                        if (std::fabs(kps[j].x - u) <= radius && std::fabs(kps[j].y - v) <= radius) vIndices.push_back(j);
        } while (false);
        if (vIndices.empty()) continue;
        int bestDist = INT32_MAX, bestIdx = -1;
        for (size_t idx : vIndices) {
            if (vpMatched[idx] >= 0) continue;
            const int kpLevel = kps[idx].octave;
            if (kpLevel < nPredictedLevel - 1 || kpLevel > nPredictedLevel) continue;
            int d = 0;
            for (int k = 0; k < 32; k++) d += __builtin_popcount((unsigned)(mp_desc[32 * (size_t)pMP + k] ^ desc[32 * idx + k]));
            if (d < bestDist) {
                bestDist = d;
                bestIdx = (int)idx;
            }
        }
        if (bestDist <= 50) {
            vpMatched[bestIdx] = pMP;
            nmatches++;
        }
    }
    return nmatches;
}

}  // extern "C"
