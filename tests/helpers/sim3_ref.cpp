// CPU restatement of ORB_SLAM::Sim3Solver for the tests (tests/test_sim3.py),
// written from src/Sim3Solver.cc directly: scalar C++, std::vector state as
// the reference keeps it, no project header but abi.h (struct layouts). The
// OpenCV calls follow docs/ORACLE_ASSUMPTIONS.md A22. std::rand() values come
// from the caller as an array (pre-drawn with gf_rng_next) with a cursor.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/gfslam/abi.h"

namespace {

typedef float M3[3][3];

struct Rand {
    const int32_t* v;
    int n, pos;
    int next() { return pos < n ? v[pos++] : (pos++, 0); }
    // DUtils::Random::RandomInt
    int RandomInt(int mn, int mx) {
        int d = mx - mn + 1;
        return int(((double)next() / ((double)2147483647 + 1.0)) * d) + mn;
    }
};

float cv_hypot(float a, float b) {
    a = std::abs(a);
    b = std::abs(b);
    if (a > b) {
        b /= a;
        return a * std::sqrt(1 + b * b);
    }
    if (b > 0) {
        a /= b;
        return b * std::sqrt(1 + a * a);
    }
    return 0;
}

// cv::eigen(symmetric CV_32F): Jacobi, eigenvalues descending, vectors as rows
void cv_eigen(std::vector<float>& A, int n, std::vector<float>& W, std::vector<float>& V) {
    const float eps = std::numeric_limits<float>::epsilon();
    W.assign(n, 0.f);
    V.assign(n * n, 0.f);
    for (int i = 0; i < n; i++) V[i * n + i] = 1.f;
    std::vector<int> indR(n, 0), indC(n, 0);
    auto scan_row = [&](int k) {
        int m = k + 1;
        float mv = std::abs(A[n * k + m]);
        for (int i = k + 2; i < n; i++) {
            float val = std::abs(A[n * k + i]);
            if (mv < val) mv = val, m = i;
        }
        indR[k] = m;
    };
    auto scan_col = [&](int k) {
        int m = 0;
        float mv = std::abs(A[k]);
        for (int i = 1; i < k; i++) {
            float val = std::abs(A[n * i + k]);
            if (mv < val) mv = val, m = i;
        }
        indC[k] = m;
    };
    for (int k = 0; k < n; k++) {
        W[k] = A[(n + 1) * k];
        if (k < n - 1) scan_row(k);
        if (k > 0) scan_col(k);
    }
    const int maxIters = n * n * 30;
    if (n > 1)
        for (int iters = 0; iters < maxIters; iters++) {
            int k = 0;
            float mv = std::abs(A[indR[0]]);
            for (int i = 1; i < n - 1; i++) {
                float val = std::abs(A[n * i + indR[i]]);
                if (mv < val) mv = val, k = i;
            }
            int l = indR[k];
            for (int i = 1; i < n; i++) {
                float val = std::abs(A[n * indC[i] + i]);
                if (mv < val) mv = val, k = indC[i], l = i;
            }
            float p = A[n * k + l];
            if (std::abs(p) <= eps) break;
            float y = (float)((W[l] - W[k]) * 0.5);
            float t = std::abs(y) + cv_hypot(p, y);
            float s = cv_hypot(p, t);
            float c = t / s;
            s = p / s;
            t = (p / t) * p;
            if (y < 0) s = -s, t = -t;
            A[n * k + l] = 0;
            W[k] -= t;
            W[l] += t;
            auto rotate = [&](float& v0, float& v1) {
                float a0 = v0, b0 = v1;
                v0 = a0 * c - b0 * s;
                v1 = a0 * s + b0 * c;
            };
            for (int i = 0; i < k; i++) rotate(A[n * i + k], A[n * i + l]);
            for (int i = k + 1; i < l; i++) rotate(A[n * k + i], A[n * i + l]);
            for (int i = l + 1; i < n; i++) rotate(A[n * k + i], A[n * l + i]);
            for (int i = 0; i < n; i++) rotate(V[n * k + i], V[n * l + i]);
            for (int j = 0; j < 2; j++) {
                int idx = j == 0 ? k : l;
                if (idx < n - 1) scan_row(idx);
                if (idx > 0) scan_col(idx);
            }
        }
    for (int k = 0; k < n - 1; k++) {
        int m = k;
        for (int i = k + 1; i < n; i++)
            if (W[m] < W[i]) m = i;
        if (k != m) {
            std::swap(W[m], W[k]);
            for (int i = 0; i < n; i++) std::swap(V[n * m + i], V[n * k + i]);
        }
    }
}

// cv::Rodrigues, 1x3 float vector -> 3x3 float matrix (computed in double)
void cv_rodrigues(const float r[3], M3 R) {
    double rx = r[0], ry = r[1], rz = r[2];
    double theta = std::sqrt(rx * rx + ry * ry + rz * rz);
    if (theta < std::numeric_limits<double>::epsilon()) {
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) R[i][j] = i == j;
        return;
    }
    const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    double c = std::cos(theta), s = std::sin(theta), c1 = 1. - c, itheta = 1. / theta;
    rx *= itheta;
    ry *= itheta;
    rz *= itheta;
    double rrt[9] = {rx * rx, rx * ry, rx * rz, rx * ry, ry * ry, ry * rz, rx * rz, ry * rz, rz * rz};
    double r_x[9] = {0, -rz, ry, rz, 0, -rx, -ry, rx, 0};
    for (int k = 0; k < 9; k++) R[k / 3][k % 3] = (float)(c * I[k] + c1 * rrt[k] + s * r_x[k]);
}

// Mat::dot of CV_32F: double accumulator, four products per step
double cv_dot(const float* a, const float* b, int len) {
    double result = 0;
    int i = 0;
    for (; i <= len - 4; i += 4)
        result += (double)a[i] * b[i] + (double)a[i + 1] * b[i + 1] + (double)a[i + 2] * b[i + 2] +
                  (double)a[i + 3] * b[i + 3];
    for (; i < len; i++) result += (double)a[i] * b[i];
    return result;
}

// product of small float Mats: float sums, left to right (A1)
void mul33(const M3 A, const M3 B, M3 C, bool transposeB) {
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            float acc = 0;
            for (int k = 0; k < 3; k++) {
                float prod = A[i][k] * (transposeB ? B[j][k] : B[k][j]);
                acc = k == 0 ? prod : acc + prod;
            }
            C[i][j] = acc;
        }
}

float row_dot3(const float r[3], const float v[3]) {
    float acc = r[0] * v[0];
    acc = acc + r[1] * v[1];
    acc = acc + r[2] * v[2];
    return acc;
}

struct Solver {
    int N;
    const float *X1, *X2;
    std::vector<float> err1, err2;  // mvnMaxError1/2 (size_t values as compared: float)
    std::vector<float> P1im1, P2im2;
    float K1[4], K2[4];
    // hypothesis
    M3 R12;
    float t12[3], s12, T12[16], T21[16];
    std::vector<uint8_t> inl;
    int ninl;

    void FromCameraToImage(const float* X, std::vector<float>& out, const float K[4]) {
        out.resize(2 * (size_t)N);
        for (int i = 0; i < N; i++) {
            float invz = 1 / X[3 * i + 2];
            float x = X[3 * i] * invz, y = X[3 * i + 1] * invz;
            out[2 * i] = K[0] * x + K[2];
            out[2 * i + 1] = K[1] * y + K[3];
        }
    }

    void centroid(const M3 P, M3 Pr, float C[3]) {
        for (int r = 0; r < 3; r++) {
            // cv::reduce(P, C, 1, CV_REDUCE_SUM): two running sums, joined at the end
            float a0 = P[r][0], a1 = P[r][1];
            a0 = a0 + P[r][2];
            a0 = a0 + a1;
            C[r] = a0 * (float)(1. / 3);  // C/P.cols: convertTo with a float factor
        }
        for (int i = 0; i < 3; i++)
            for (int r = 0; r < 3; r++) Pr[r][i] = P[r][i] - C[r];
    }

    void computeT(const M3 P1, const M3 P2) {
        M3 Pr1, Pr2, M;
        float O1[3], O2[3];
        centroid(P1, Pr1, O1);
        centroid(P2, Pr2, O2);
        mul33(Pr2, Pr1, M, true);
        double N11, N12, N13, N14, N22, N23, N24, N33, N34, N44;
        N11 = M[0][0] + M[1][1] + M[2][2];
        N12 = M[1][2] - M[2][1];
        N13 = M[2][0] - M[0][2];
        N14 = M[0][1] - M[1][0];
        N22 = M[0][0] - M[1][1] - M[2][2];
        N23 = M[0][1] + M[1][0];
        N24 = M[2][0] + M[0][2];
        N33 = -M[0][0] + M[1][1] - M[2][2];
        N34 = M[1][2] + M[2][1];
        N44 = -M[0][0] - M[1][1] + M[2][2];
        const double Nd[16] = {N11, N12, N13, N14, N12, N22, N23, N24, N13, N23, N33, N34, N14, N24, N34, N44};
        std::vector<float> Nf(16), eval, evec;
        for (int i = 0; i < 16; i++) Nf[i] = (float)Nd[i];
        cv_eigen(Nf, 4, eval, evec);
        float vec[3] = {evec[1], evec[2], evec[3]};
        double sq = 0;  // cv::norm (L2): double accumulator, one by one below four elements
        for (int i = 0; i < 3; i++) sq += (double)vec[i] * (double)vec[i];
        double nrm = std::sqrt(sq);
        double ang = std::atan2(nrm, (double)evec[0]);
        double alpha = 2 * ang;  // (2*ang*vec)/norm(vec): the expression's factor times 1/norm
        alpha *= 1. / nrm;
        const float af = (float)alpha;
        for (int i = 0; i < 3; i++) vec[i] = vec[i] * af;
        cv_rodrigues(vec, R12);
        M3 P3;
        mul33(R12, Pr2, P3, false);
        double nom = cv_dot(&Pr1[0][0], &P3[0][0], 9);
        double den = 0;
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) {
                float sq = P3[i][j] * P3[i][j];  // cv::pow(P3, 2, aux_P3)
                den += sq;
            }
        s12 = (float)(nom / den);
        // O1 - ms12i*mR12i*O2: gemm with the scale applied in double to the float sum
        for (int i = 0; i < 3; i++) t12[i] = O1[i] - (float)((double)s12 * (double)row_dot3(R12[i], O2));
        std::memset(T12, 0, sizeof T12);
        std::memset(T21, 0, sizeof T21);
        T12[15] = T21[15] = 1.f;
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) T12[4 * i + j] = R12[i][j] * s12;  // ms12i*mR12i
            T12[4 * i + 3] = t12[i];
        }
        const float inv = (float)(1.0 / s12);
        M3 sRinv;
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) sRinv[i][j] = R12[j][i] * inv;
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) T21[4 * i + j] = sRinv[i][j];
            T21[4 * i + 3] = (float)(-1.0 * (double)row_dot3(sRinv[i], t12));
        }
    }

    void Project(const float* X, std::vector<float>& out, const float T[16], const float K[4]) {
        out.resize(2 * (size_t)N);
        for (int i = 0; i < N; i++) {
            float c[3];
            for (int r = 0; r < 3; r++) c[r] = row_dot3(&T[4 * r], &X[3 * i]) + T[4 * r + 3];
            float invz = 1 / c[2];
            float x = c[0] * invz, y = c[1] * invz;
            out[2 * i] = K[0] * x + K[2];
            out[2 * i + 1] = K[1] * y + K[3];
        }
    }

    void CheckInliers() {
        std::vector<float> vP2im1, vP1im2;
        Project(X2, vP2im1, T12, K1);
        Project(X1, vP1im2, T21, K2);
        ninl = 0;
        for (int i = 0; i < N; i++) {
            float d1[2] = {P1im1[2 * i] - vP2im1[2 * i], P1im1[2 * i + 1] - vP2im1[2 * i + 1]};
            float d2[2] = {vP1im2[2 * i] - P2im2[2 * i], vP1im2[2 * i + 1] - P2im2[2 * i + 1]};
            float e1 = (float)cv_dot(d1, d1, 2), e2 = (float)cv_dot(d2, d2, 2);
            if (e1 < err1[i] && e2 < err2[i]) {
                inl[i] = 1;
                ninl++;
            } else
                inl[i] = 0;
        }
    }
};

// ---------------------------------------------------------------- SearchBySim3
// What ORBmatcher::SearchBySim3 reads of a KeyFrame (KeyFrame.cc): the grid of
// Frame.cc:100-131, GetFeaturesInArea (:612-652), IsInImage (:654-657).
struct RefKF {
    static const int COLS = 64, ROWS = 48;
    const gf_frame_info* fi;
    const gf_keypoint* kps;
    const uint8_t* desc;
    const int32_t* mp;
    int n;
    float Rt[3][4];
    float invW, invH;
    std::vector<float> scales;
    std::vector<std::vector<size_t>> grid;  // [ix * ROWS + iy]

    RefKF(const gf_frame_info* f, const float* Tcw, const gf_keypoint* k, const uint8_t* d, const int32_t* m, int n_)
        : fi(f), kps(k), desc(d), mp(m), n(n_), grid(COLS * ROWS) {
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 4; c++) Rt[r][c] = Tcw[4 * r + c];
        invW = (float)COLS / (float)(fi->max_x - fi->min_x);
        invH = (float)ROWS / (float)(fi->max_y - fi->min_y);
        scales.assign(fi->nlevels, 1.f);
        for (int i = 1; i < fi->nlevels; i++) scales[i] = scales[i - 1] * fi->scale_factor;
        for (int i = 0; i < n; i++) {
            int px = (int)std::round((kps[i].x - fi->min_x) * invW);
            int py = (int)std::round((kps[i].y - fi->min_y) * invH);
            if (px < 0 || px >= COLS || py < 0 || py >= ROWS) continue;
            grid[px * ROWS + py].push_back(i);
        }
    }
    bool IsInImage(float x, float y) const { return x >= fi->min_x && x < fi->max_x && y >= fi->min_y && y < fi->max_y; }
    std::vector<size_t> GetFeaturesInArea(float x, float y, float r) const {
        std::vector<size_t> v;
        int nMinCellX = (int)std::floor((x - fi->min_x - r) * invW);
        nMinCellX = std::max(0, nMinCellX);
        if (nMinCellX >= COLS) return v;
        int nMaxCellX = (int)std::ceil((x - fi->min_x + r) * invW);
        nMaxCellX = std::min(COLS - 1, nMaxCellX);
        if (nMaxCellX < 0) return v;
        int nMinCellY = (int)std::floor((y - fi->min_y - r) * invH);
        nMinCellY = std::max(0, nMinCellY);
        if (nMinCellY >= ROWS) return v;
        int nMaxCellY = (int)std::ceil((y - fi->min_y + r) * invH);
        nMaxCellY = std::min(ROWS - 1, nMaxCellY);
        if (nMaxCellY < 0) return v;
        for (int ix = nMinCellX; ix <= nMaxCellX; ix++)
            for (int iy = nMinCellY; iy <= nMaxCellY; iy++)
                for (size_t j : grid[ix * ROWS + iy])
                    if (std::abs(kps[j].x - x) <= r && std::abs(kps[j].y - y) <= r) v.push_back(j);
        return v;
    }
    int index_of(int id) const {  // MapPoint::GetIndexInKeyFrame
        for (int i = 0; i < n; i++)
            if (mp[i] == id) return i;
        return -1;
    }
};

int descriptor_distance(const uint8_t* a, const uint8_t* b) {
    int d = 0;
    for (int i = 0; i < 32; i++) d += __builtin_popcount((unsigned)(a[i] ^ b[i]));
    return d;
}

void mat_vec_add(const float M[3][3], const float v[3], const float t[3], float out[3]) {
    for (int r = 0; r < 3; r++) out[r] = row_dot3(M[r], v) + t[r];
}

// one projection pass (:1893-1973 / :1976-2058): points of `from` searched in `to`
void search_pass(const RefKF& from, const RefKF& to, const float sR[3][3], const float t[3],
                 const std::vector<bool>& already, const gf_map_point* mps, const uint8_t* mp_desc,
                 const uint8_t* mp_bad, float th, std::vector<int>& vnMatch) {
    const int nMaxLevel = to.fi->nlevels - 1;
    for (int i = 0; i < from.n; i++) {
        const int id = from.mp[i];
        if (id < 0 || already[i]) continue;
        if (mp_bad && mp_bad[id]) continue;
        const gf_map_point& P = mps[id];
        float Rw[3][3], tw[3], pa[3], pb[3];
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) Rw[r][c] = from.Rt[r][c];
            tw[r] = from.Rt[r][3];
        }
        mat_vec_add(Rw, P.pos, tw, pa);
        mat_vec_add(sR, pa, t, pb);
        if (pb[2] < 0.0) continue;
        float invz = 1.0 / pb[2];
        float x = pb[0] * invz, y = pb[1] * invz;
        float u = to.fi->fx * x + to.fi->cx, v = to.fi->fy * y + to.fi->cy;
        if (!to.IsInImage(u, v)) continue;
        double sq = 0;
        for (int k = 0; k < 3; k++) sq += (double)pb[k] * (double)pb[k];
        float dist3D = std::sqrt(sq);  // cv::norm
        if (dist3D < P.min_dist || dist3D > P.max_dist) continue;
        float ratio = dist3D / P.min_dist;
        int lb = std::lower_bound(to.scales.begin(), to.scales.end(), ratio) - to.scales.begin();
        const int nPredictedLevel = std::min(lb, nMaxLevel);
        float radius = th * to.scales[nPredictedLevel];
        std::vector<size_t> vIndices = to.GetFeaturesInArea(u, v, radius);
        if (vIndices.empty()) continue;
        int bestDist = 2147483647, bestIdx = -1;
        for (size_t idx : vIndices) {
            if (to.kps[idx].octave < nPredictedLevel - 1 || to.kps[idx].octave > nPredictedLevel) continue;
            int dist = descriptor_distance(mp_desc + 32 * (size_t)id, to.desc + 32 * idx);
            if (dist < bestDist) {
                bestDist = dist;
                bestIdx = (int)idx;
            }
        }
        if (bestDist <= 100) vnMatch[i] = bestIdx;
    }
}

}  // namespace

extern "C" {

int sim3ref_search_by_sim3(const gf_frame_info* fi, const float* Tcw1, const gf_keypoint* kps1, const uint8_t* desc1,
                           int n1, const int32_t* kf_mp1, const float* Tcw2, const gf_keypoint* kps2,
                           const uint8_t* desc2, int n2, const int32_t* kf_mp2, const gf_map_point* mps,
                           const uint8_t* mp_desc, const uint8_t* mp_bad, int32_t* matches12, float s12,
                           const float* R12, const float* t12, float th) {
    RefKF KF1(fi, Tcw1, kps1, desc1, kf_mp1, n1), KF2(fi, Tcw2, kps2, desc2, kf_mp2, n2);
    float sR12[3][3], sR21[3][3], t21[3];
    const float inv = (float)(1.0 / s12);
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            sR12[r][c] = R12[3 * r + c] * s12;
            sR21[r][c] = R12[3 * c + r] * inv;
        }
    for (int r = 0; r < 3; r++) t21[r] = (float)(-1.0 * (double)row_dot3(sR21[r], t12));
    std::vector<bool> vbAlreadyMatched1(n1, false), vbAlreadyMatched2(n2, false);
    for (int i = 0; i < n1; i++)
        if (matches12[i] >= 0) {
            vbAlreadyMatched1[i] = true;
            int idx2 = KF2.index_of(matches12[i]);
            if (idx2 >= 0 && idx2 < n2) vbAlreadyMatched2[idx2] = true;
        }
    std::vector<int> vnMatch1(n1, -1), vnMatch2(n2, -1);
    search_pass(KF1, KF2, sR21, t21, vbAlreadyMatched1, mps, mp_desc, mp_bad, th, vnMatch1);
    search_pass(KF2, KF1, sR12, t12, vbAlreadyMatched2, mps, mp_desc, mp_bad, th, vnMatch2);
    int nFound = 0;
    for (int i1 = 0; i1 < n1; i1++) {
        int idx2 = vnMatch1[i1];
        if (idx2 >= 0 && vnMatch2[idx2] == i1) {
            matches12[i1] = kf_mp2[idx2];
            nFound++;
        }
    }
    return nFound;
}

// SetRansacParameters (:114-138); NaN / out-of-range estimates take max_iterations
int sim3ref_init(int n, const gf_sim3_params* p, gf_sim3_state* st) {
    std::memset(st, 0, sizeof *st);
    st->n = n;
    st->min_inliers = p->min_inliers;
    float epsilon = (float)p->min_inliers / n;
    int nIterations;
    if (p->min_inliers == n)
        nIterations = 1;
    else {
        double v = std::ceil(std::log(1 - p->probability) / std::log(1 - std::pow(epsilon, 3)));
        if (std::isnan(v) || v >= 2147483647.0 || v <= -2147483648.0)
            nIterations = p->max_iterations;
        else
            nIterations = (int)v;
    }
    st->max_iterations = std::max(1, std::min(nIterations, p->max_iterations));
    st->iterations = 0;
    return 0;
}

// iterate (:140-207). rand_vals[*cursor...] are the std::rand() values; *cursor advances.
int sim3ref_iterate(const float* X1, const float* X2, const float* sigma2_1, const float* sigma2_2, const float* K1,
                    const float* K2, gf_sim3_state* st, uint8_t* best_mask, int nIterations, const int32_t* rand_vals,
                    int nrand, int32_t* cursor, float* T12, uint8_t* inliers, int32_t* ninliers, int32_t* flags) {
    const int N = st->n;
    std::memset(T12, 0, 16 * sizeof(float));
    if (N > 0) std::memset(inliers, 0, N);
    *ninliers = 0;
    *flags = 0;
    // fewer than three correspondences index an empty vector in the reference: no iteration here
    if (N < st->min_inliers || N < 3) {
        *flags = GF_SIM3_NOMORE;
        return 0;
    }
    Solver S;
    S.N = N;
    S.X1 = X1;
    S.X2 = X2;
    for (int i = 0; i < 4; i++) S.K1[i] = K1[i], S.K2[i] = K2[i];
    S.err1.resize(N);
    S.err2.resize(N);
    for (int i = 0; i < N; i++) {
        size_t m1 = 9.210 * sigma2_1[i], m2 = 9.210 * sigma2_2[i];  // vector<size_t>::push_back(double)
        S.err1[i] = m1;  // err<mvnMaxError: the size_t converts to float
        S.err2[i] = m2;
    }
    S.FromCameraToImage(X1, S.P1im1, K1);
    S.FromCameraToImage(X2, S.P2im2, K2);
    S.inl.assign(N, 0);
    Rand rnd{rand_vals, nrand, *cursor};

    std::vector<size_t> all(N), avail;
    for (int i = 0; i < N; i++) all[i] = i;
    int nCurrent = 0;
    bool found = false;
    while (st->iterations < st->max_iterations && nCurrent < nIterations) {
        nCurrent++;
        st->iterations++;
        avail = all;
        size_t size = avail.size();  // pop_back keeps the storage: a write past the new end stays inside it
        M3 P1, P2;
        for (short i = 0; i < 3; ++i) {
            int randi = rnd.RandomInt(0, (int)size - 1);
            int idx = avail[randi];
            for (int r = 0; r < 3; r++) {
                P1[r][i] = X1[3 * idx + r];
                P2[r][i] = X2[3 * idx + r];
            }
            avail[idx] = avail[size - 1];
            size--;
        }
        S.computeT(P1, P2);
        S.CheckInliers();
        if (S.ninl >= st->best_inliers) {
            std::memcpy(best_mask, S.inl.data(), N);
            st->best_inliers = S.ninl;
            std::memcpy(st->best_T12, S.T12, sizeof S.T12);
            std::memcpy(st->best_R, S.R12, sizeof S.R12);
            std::memcpy(st->best_t, S.t12, sizeof S.t12);
            st->best_scale = S.s12;
            if (S.ninl > st->min_inliers) {
                *ninliers = S.ninl;
                std::memcpy(inliers, S.inl.data(), N);
                std::memcpy(T12, S.T12, sizeof S.T12);
                found = true;
                break;
            }
        }
    }
    *cursor = rnd.pos;
    if (found)
        *flags = GF_SIM3_FOUND;
    else if (st->iterations >= st->max_iterations)
        *flags = GF_SIM3_NOMORE;
    return 0;
}

}  // extern "C"
