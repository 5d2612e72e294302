// Serial CPU restatement of LocalMapping::CreateNewMapPoints for the tests
// (tests/localmap_ref.py, tests/test_localmap_cpu.py, tests/test_localmap_gpu.py),
// written from the reference: src/LocalMapping.cc:213-241 (MapPointCulling),
// :243-409 (CreateNewMapPoints), :490-507 (ComputeF12) and
// src/KeyFrame.cc:659-689 (ComputeSceneMedianDepth). It shares no header with
// the library. SearchForTriangulation is the CPU oracle's, called between
// lm_setup and lm_triangulate from the Python side, which owns the neighbour
// loop. OpenCV readings: docs/ORACLE_ASSUMPTIONS.md A27.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <vector>

namespace {

struct KeyPoint {  // cv::KeyPoint, 28 bytes
    float x, y, size, angle, response;
    int32_t octave, class_id;
};

struct Camera {
    float fx, fy, cx, cy, scale_factor;
    int32_t nlevels;
};

struct NewPoint {
    int32_t neighbour, idx1, idx2;
    float pos[3];
};

enum { EXIT_PARALLAX, EXIT_W0, EXIT_Z1, EXIT_Z2, EXIT_REPROJ1, EXIT_REPROJ2, EXIT_DIST0, EXIT_SCALE, EXIT_ACCEPTED };
enum { ST_OK, ST_BASELINE, ST_NODEPTH };

// cv::SVD::compute on a square CV_32F matrix (JacobiSVDImpl_<float>): the
// one-sided Jacobi on the columns of A (rows of its transpose), float
// rotations, double inner products, eps = 2 FLT_EPSILON, then the singular
// values sorted descending by selection. Only w and vt are produced.
void svd_square(int n, const float* A, float* w, float* vt) {
    std::vector<float> At(n * n), V(n * n, 0.f);
    std::vector<double> W(n);
    for (int i = 0; i < n; i++)
        for (int k = 0; k < n; k++) At[i * n + k] = A[k * n + i];
    const float eps = FLT_EPSILON * 2;
    for (int i = 0; i < n; i++) {
        double sd = 0;
        for (int k = 0; k < n; k++) sd += (double)At[i * n + k] * (double)At[i * n + k];
        W[i] = sd;
        V[i * n + i] = 1.f;
    }
    const int max_iter = std::max(n, 30);
    for (int iter = 0; iter < max_iter; iter++) {
        bool changed = false;
        for (int i = 0; i < n - 1; i++)
            for (int j = i + 1; j < n; j++) {
                float *Ai = &At[i * n], *Aj = &At[j * n];
                double a = W[i], p = 0, b = W[j];
                for (int k = 0; k < n; k++) p += (double)Ai[k] * (double)Aj[k];
                if (std::fabs(p) <= (double)eps * std::sqrt(a * b)) continue;
                p *= 2;
                const double beta = a - b, gamma = std::sqrt(p * p + beta * beta);
                float c, s;
                if (beta < 0) {
                    const double delta = (gamma - beta) * 0.5;
                    s = (float)std::sqrt(delta / gamma);
                    c = (float)(p / (gamma * (double)s * 2));
                } else {
                    c = (float)std::sqrt((gamma + beta) / (gamma * 2));
                    s = (float)(p / (gamma * (double)c * 2));
                }
                a = b = 0;
                for (int k = 0; k < n; k++) {
                    const float t0 = c * Ai[k] + s * Aj[k];
                    const float t1 = -s * Ai[k] + c * Aj[k];
                    Ai[k] = t0;
                    Aj[k] = t1;
                    a += (double)t0 * (double)t0;
                    b += (double)t1 * (double)t1;
                }
                W[i] = a;
                W[j] = b;
                changed = true;
                float *Vi = &V[i * n], *Vj = &V[j * n];
                for (int k = 0; k < n; k++) {
                    const float t0 = c * Vi[k] + s * Vj[k];
                    const float t1 = -s * Vi[k] + c * Vj[k];
                    Vi[k] = t0;
                    Vj[k] = t1;
                }
            }
        if (!changed) break;
    }
    for (int i = 0; i < n; i++) {
        double sd = 0;
        for (int k = 0; k < n; k++) sd += (double)At[i * n + k] * (double)At[i * n + k];
        W[i] = std::sqrt(sd);
    }
    for (int i = 0; i < n - 1; i++) {
        int j = i;
        for (int k = i + 1; k < n; k++)
            if (W[j] < W[k]) j = k;
        if (i != j) {
            std::swap(W[i], W[j]);
            for (int k = 0; k < n; k++) {
                std::swap(At[i * n + k], At[j * n + k]);
                std::swap(V[i * n + k], V[j * n + k]);
            }
        }
    }
    for (int i = 0; i < n; i++) w[i] = (float)W[i];
    for (int i = 0; i < n * n; i++) vt[i] = V[i];
}

// small Mat product (A1): float products, float sums left to right
void mul33(const float* A, const float* B, float* D) {
    float out[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) out[3 * i + j] = (A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j];
    for (int i = 0; i < 9; i++) D[i] = out[i];
}

double det33(const float* m) {
    return m[0] * ((double)m[4] * m[8] - (double)m[5] * m[7]) - m[1] * ((double)m[3] * m[8] - (double)m[5] * m[6]) +
           m[2] * ((double)m[3] * m[7] - (double)m[4] * m[6]);
}

// Mat::inv() of a 3x3 CV_32F (A17): the closed form in double
void inv33(const float* S, float* D) {
    double d = det33(S);
    if (d == 0.) {
        for (int i = 0; i < 9; i++) D[i] = 0.f;
        return;
    }
    d = 1. / d;
    D[0] = (float)(((double)S[4] * S[8] - (double)S[5] * S[7]) * d);
    D[1] = (float)(((double)S[2] * S[7] - (double)S[1] * S[8]) * d);
    D[2] = (float)(((double)S[1] * S[5] - (double)S[2] * S[4]) * d);
    D[3] = (float)(((double)S[5] * S[6] - (double)S[3] * S[8]) * d);
    D[4] = (float)(((double)S[0] * S[8] - (double)S[2] * S[6]) * d);
    D[5] = (float)(((double)S[2] * S[3] - (double)S[0] * S[5]) * d);
    D[6] = (float)(((double)S[3] * S[7] - (double)S[4] * S[6]) * d);
    D[7] = (float)(((double)S[1] * S[6] - (double)S[0] * S[7]) * d);
    D[8] = (float)(((double)S[0] * S[4] - (double)S[1] * S[3]) * d);
}

void rot_of(const float* T, float* R, float* t) {
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) R[3 * r + c] = T[4 * r + c];
        t[r] = T[4 * r + 3];
    }
}

void transpose33(const float* A, float* B) {
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) B[3 * j + i] = A[3 * i + j];
}

// GetCameraCenter: Ow = -Rcw^T tcw
void centre_of(const float* T, float* Ow) {
    for (int c = 0; c < 3; c++) Ow[c] = -((T[c] * T[3] + T[4 + c] * T[7]) + T[8 + c] * T[11]);
}

double norm3(const float* v) {  // cv::norm: double accumulation
    double s = 0;
    for (int i = 0; i < 3; i++) s += (double)v[i] * (double)v[i];
    return std::sqrt(s);
}

double dot3(const float* a, const float* b) {  // Mat::dot: double accumulation
    double s = 0;
    for (int i = 0; i < 3; i++) s += (double)a[i] * (double)b[i];
    return s;
}

void level_tables(const Camera& cam, float* sf, float* sigma2) {
    sf[0] = 1.f;
    for (int l = 1; l < cam.nlevels; l++) sf[l] = sf[l - 1] * cam.scale_factor;
    for (int l = 0; l < cam.nlevels; l++) sigma2[l] = sf[l] * sf[l];
}

// ComputeF12 (LocalMapping.cc:490-507)
void compute_f12(const Camera& cam, const float* T1, const float* T2, float* F) {
    float R1[9], t1[3], R2[9], t2[3], R2t[9], R12[9], t12[3];
    rot_of(T1, R1, t1);
    rot_of(T2, R2, t2);
    transpose33(R2, R2t);
    mul33(R1, R2t, R12);
    for (int r = 0; r < 3; r++) {  // -R1w*R2w.t()*t2w+t1w: the scale -1 negates the product's entries
        const float m0 = -R12[3 * r], m1 = -R12[3 * r + 1], m2 = -R12[3 * r + 2];
        t12[r] = ((m0 * t2[0] + m1 * t2[1]) + m2 * t2[2]) + t1[r];
    }
    const float tx[9] = {0.f, -t12[2], t12[1], t12[2], 0.f, -t12[0], -t12[1], t12[0], 0.f};
    const float K[9] = {cam.fx, 0.f, cam.cx, 0.f, cam.fy, cam.cy, 0.f, 0.f, 1.f};
    float Kt[9], Kti[9], Ki[9], A[9], B[9];
    transpose33(K, Kt);
    inv33(Kt, Kti);
    inv33(K, Ki);
    mul33(Kti, tx, A);
    mul33(A, R12, B);
    mul33(B, Ki, F);
}

// the depths of ComputeSceneMedianDepth (KeyFrame.cc:670-684), slot order
void scene_depths(const float* T, const int32_t* mp, int n, const float* mp_pos, int nmp, std::vector<float>& d) {
    for (int i = 0; i < n; i++) {
        if (mp[i] < 0 || mp[i] >= nmp) continue;
        const float z = (float)(dot3(T + 8, mp_pos + 3 * (size_t)mp[i]) + (double)T[11]);
        d.push_back(z);
    }
}

// one match of :307-390
int match_body(const Camera& cam, const float* T1, const float* T2, const KeyPoint& kp1, const KeyPoint& kp2,
               float* x3D) {
    float sf[16], sigma2[16], Ow1[3], Ow2[3];
    level_tables(cam, sf, sigma2);
    centre_of(T1, Ow1);
    centre_of(T2, Ow2);
    const float invfx = 1.0f / cam.fx, invfy = 1.0f / cam.fy;
    const float xn1[3] = {(kp1.x - cam.cx) * invfx, (kp1.y - cam.cy) * invfy, 1.f};
    const float xn2[3] = {(kp2.x - cam.cx) * invfx, (kp2.y - cam.cy) * invfy, 1.f};
    float ray1[3], ray2[3];
    for (int r = 0; r < 3; r++) {
        ray1[r] = (T1[r] * xn1[0] + T1[4 + r] * xn1[1]) + T1[8 + r] * xn1[2];
        ray2[r] = (T2[r] * xn2[0] + T2[4 + r] * xn2[1]) + T2[8 + r] * xn2[2];
    }
    const float cosParallaxRays = (float)(dot3(ray1, ray2) / (norm3(ray1) * norm3(ray2)));
    if (cosParallaxRays < 0 || cosParallaxRays > 0.9998) return EXIT_PARALLAX;
    float A[16];
    const float* Ts[2] = {T1, T2};
    const float* xs[2] = {xn1, xn2};
    for (int v = 0; v < 2; v++)
        for (int r = 0; r < 2; r++)
            for (int c = 0; c < 4; c++)  // x*Tcw.row(2) - Tcw.row(r): addWeighted in double
                A[4 * (2 * v + r) + c] =
                    (float)((double)Ts[v][8 + c] * (double)xs[v][r] + (double)Ts[v][4 * r + c] * -1.0 + 0.0);
    float w[4], vt[16];
    svd_square(4, A, w, vt);
    if (vt[15] == 0) return EXIT_W0;
    const float inv = (float)(1.0 / (double)vt[15]);  // x3D.rowRange(0,3)/x3D(3): one float factor
    for (int r = 0; r < 3; r++) x3D[r] = vt[12 + r] * inv;
    const float z1 = (float)(dot3(T1 + 8, x3D) + (double)T1[11]);
    if (z1 <= 0) return EXIT_Z1;
    const float z2 = (float)(dot3(T2 + 8, x3D) + (double)T2[11]);
    if (z2 <= 0) return EXIT_Z2;
    const int o1 = std::min(std::max(kp1.octave, 0), cam.nlevels - 1);
    const int o2 = std::min(std::max(kp2.octave, 0), cam.nlevels - 1);
    const float sigmaSquare1 = sigma2[o1];
    const float x1 = (float)(dot3(T1, x3D) + (double)T1[3]);
    const float y1 = (float)(dot3(T1 + 4, x3D) + (double)T1[7]);
    const float invz1 = (float)(1.0 / (double)z1);
    const float u1 = cam.fx * x1 * invz1 + cam.cx;
    const float v1 = cam.fy * y1 * invz1 + cam.cy;
    const float errX1 = u1 - kp1.x, errY1 = v1 - kp1.y;
    if ((errX1 * errX1 + errY1 * errY1) > 5.991 * sigmaSquare1) return EXIT_REPROJ1;
    const float sigmaSquare2 = sigma2[o2];
    const float x2 = (float)(dot3(T2, x3D) + (double)T2[3]);
    const float y2 = (float)(dot3(T2 + 4, x3D) + (double)T2[7]);
    const float invz2 = (float)(1.0 / (double)z2);
    const float u2 = cam.fx * x2 * invz2 + cam.cx;
    const float v2 = cam.fy * y2 * invz2 + cam.cy;
    const float errX2 = u2 - kp2.x, errY2 = v2 - kp2.y;
    if ((errX2 * errX2 + errY2 * errY2) > 5.991 * sigmaSquare2) return EXIT_REPROJ2;
    const float normal1[3] = {x3D[0] - Ow1[0], x3D[1] - Ow1[1], x3D[2] - Ow1[2]};
    const float dist1 = (float)norm3(normal1);
    const float normal2[3] = {x3D[0] - Ow2[0], x3D[1] - Ow2[1], x3D[2] - Ow2[2]};
    const float dist2 = (float)norm3(normal2);
    if (dist1 == 0 || dist2 == 0) return EXIT_DIST0;
    const float ratioDist = dist1 / dist2;
    const float ratioOctave = sf[o1] / sf[o2];
    const float ratioFactor = 1.5f * cam.scale_factor;
    if (ratioDist * ratioFactor < ratioOctave || ratioDist > ratioOctave * ratioFactor) return EXIT_SCALE;
    return EXIT_ACCEPTED;
}

}  // namespace

extern "C" {

void lm_svd4(const float* A, float* w, float* vt) { svd_square(4, A, w, vt); }

void lm_compute_f12(const Camera* cam, const float* T1, const float* T2, float* F) { compute_f12(*cam, T1, T2, F); }

// ComputeSceneMedianDepth(2): depths[] receives the unsorted list (capacity n); returns the count
int lm_median_depth(const float* T, const int32_t* mp, int n, const float* mp_pos, int nmp, float* depths,
                    float* median) {
    std::vector<float> d;
    scene_depths(T, mp, n, mp_pos, nmp, d);
    for (size_t i = 0; i < d.size(); i++) depths[i] = d[i];
    *median = 0.f;
    if (d.empty()) return 0;
    std::sort(d.begin(), d.end());
    *median = d[(d.size() - 1) / 2];
    return (int)d.size();
}

// the median of a given list, as ComputeSceneMedianDepth takes it
float lm_median_of(const float* depths, int n) {
    std::vector<float> d(depths, depths + n);
    std::sort(d.begin(), d.end());
    return d[(d.size() - 1) / 2];
}

// :270-284 for one neighbour: status, median depth, F12 (zeros when skipped)
int lm_setup(const Camera* cam, const float* T1, const float* T2, const int32_t* mp2, int n2, const float* mp_pos,
             int nmp, float* F12, float* median) {
    for (int i = 0; i < 9; i++) F12[i] = 0.f;
    *median = 0.f;
    std::vector<float> d;
    scene_depths(T2, mp2, n2, mp_pos, nmp, d);
    if (d.empty()) return ST_NODEPTH;
    std::sort(d.begin(), d.end());
    const float medianDepthKF2 = d[(d.size() - 1) / 2];
    *median = medianDepthKF2;
    float Ow1[3], Ow2[3], vBaseline[3];
    centre_of(T1, Ow1);
    centre_of(T2, Ow2);
    for (int r = 0; r < 3; r++) vBaseline[r] = Ow2[r] - Ow1[r];
    const float baseline = (float)norm3(vBaseline);
    const float ratioBaselineDepth = baseline / medianDepthKF2;
    if (ratioBaselineDepth < 0.01) return ST_BASELINE;
    compute_f12(*cam, T1, T2, F12);
    return ST_OK;
}

int lm_match_body(const Camera* cam, const float* T1, const float* T2, const KeyPoint* kp1, const KeyPoint* kp2,
                  float* x3D) {
    x3D[0] = x3D[1] = x3D[2] = 0.f;
    return match_body(*cam, T1, T2, *kp1, *kp2, x3D);
}

// :307-407 for one neighbour: matches12[n1] = vMatches12 (idx2 or -1), walked
// in ascending idx1 (vMatchedIndices). exits[n1]: -1 without a match. An
// accepted match appends a record and writes next_id + (its rank) into both
// slot tables. Returns the accepted count; *nmatches the match count.
int lm_triangulate(const Camera* cam, const float* T1, const float* T2, const KeyPoint* kps1, int n1,
                   const KeyPoint* kps2, int n2, const int32_t* matches12, int neighbour, int32_t* mp1, int32_t* mp2,
                   int next_id, int32_t* exits, NewPoint* out, int* nmatches) {
    int na = 0, nm = 0;
    for (int idx1 = 0; idx1 < n1; idx1++) {
        exits[idx1] = -1;
        const int idx2 = matches12[idx1];
        if (idx2 < 0 || idx2 >= n2) continue;
        nm++;
        float x3D[3];
        const int e = match_body(*cam, T1, T2, kps1[idx1], kps2[idx2], x3D);
        exits[idx1] = e;
        if (e != EXIT_ACCEPTED) continue;
        NewPoint& P = out[na];
        P.neighbour = neighbour;
        P.idx1 = idx1;
        P.idx2 = idx2;
        for (int r = 0; r < 3; r++) P.pos[r] = x3D[r];
        mp1[idx1] = next_id + na;  // AddMapPoint (:398-399)
        mp2[idx2] = next_id + na;
        na++;
    }
    *nmatches = nm;
    return na;
}

// MapPointCulling (:213-241) over the recent list: action per entry —
// 0 kept, 1 erased (already bad), 2 SetBadFlag (found ratio < 0.25),
// 3 SetBadFlag (>= 2 keyframes old with <= 2 observations), 4 erased (>= 3
// keyframes old). The ids are unsigned long in the reference; mnFirstKFid is
// never above the current keyframe's id, so the difference does not wrap.
void lm_map_point_culling(int n, const uint8_t* bad, const int32_t* found, const int32_t* visible,
                          const int64_t* first_kf_id, const int32_t* nobs, int64_t cur_kf_id, int32_t* action) {
    for (int i = 0; i < n; i++) {
        const unsigned long age = (unsigned long)cur_kf_id - (unsigned long)first_kf_id[i];
        const float ratio = static_cast<float>(found[i]) / visible[i];
        if (bad[i]) action[i] = 1;
        else if (ratio < 0.25f) action[i] = 2;
        else if (age >= 2 && nobs[i] <= 2) action[i] = 3;
        else if (age >= 3) action[i] = 4;
        else action[i] = 0;
    }
}

}  // extern "C"
