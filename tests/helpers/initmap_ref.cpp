// CPU restatement of Tracking::CreateInitialMap (src/Tracking.cc:1199-1322)
// behind the filter of Tracking::Initialize (:1126-1133), without the solver:
// imr_points is everything up to the bundle adjustment (:1126-1133,
// :1206-1249, and the graph of Optimizer.cc:51-115 as gf_ba_problem arrays),
// imr_finish everything after optimize() (Optimizer.cc:125-140,
// Tracking.cc:1268-1299). Written sequentially from the reference's lines on a
// small world of two keyframes (slot tables, observation maps keyed by
// keyframe index, docs/ORACLE_ASSUMPTIONS.md A26); it shares no header with
// the library. OpenCV readings: A1 (float products left to right), A22
// (cv::norm a double sum cast to float; Mat / s one float factor (float)(1 /
// s)), A33 (Mat * s one float product per element).
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <vector>

namespace {

struct KP {
    float x, y, size, angle, response;
    int32_t octave, class_id;
};
struct MP {
    float pos[3], normal[3], min_dist, max_dist;
};

struct KeyFrame {
    float Tcw[16];
    const KP* kps;
    const uint8_t* desc;
    int n;
    std::vector<int> slots;  // mvpMapPoints, -1 = NULL
    void center(float* Ow) const {  // Ow = -Rcw.t() * tcw
        for (int c = 0; c < 3; c++) {
            float s = Tcw[c] * Tcw[3];
            s = s + Tcw[4 + c] * Tcw[7];
            s = s + Tcw[8 + c] * Tcw[11];
            Ow[c] = -s;
        }
    }
};

struct MapPoint {
    float pos[3];
    std::map<int, int> obs;  // keyframe -> keypoint
    int ref;
    uint8_t desc[32];
    float normal[3], min_dist, max_dist;
};

struct Pyramid {
    int nlevels;
    float sf;
    float scale[16], inv_sigma2[16];
    Pyramid(int n, float f) : nlevels(n), sf(f) {
        scale[0] = 1.0f;
        for (int l = 1; l < 16; l++) scale[l] = l < n ? scale[l - 1] * f : 1.0f;
        for (int l = 0; l < 16; l++) inv_sigma2[l] = 1.0f / (scale[l] * scale[l]);
    }
    int level(int octave) const { return std::min(std::max(octave, 0), nlevels - 1); }
};

float cvnorm(const float* v) {
    return (float)std::sqrt(((double)v[0] * v[0] + (double)v[1] * v[1]) + (double)v[2] * v[2]);
}

int hamming(const uint8_t* a, const uint8_t* b) {
    int d = 0;
    for (int i = 0; i < 32; i++) d += __builtin_popcount((unsigned)(a[i] ^ b[i]));
    return d;
}

// MapPoint::ComputeDistinctiveDescriptors (MapPoint.cc:197-262)
void distinctive(MapPoint& P, const KeyFrame* kf) {
    std::vector<const uint8_t*> v;
    for (auto& o : P.obs) v.push_back(kf[o.first].desc + 32 * (size_t)o.second);
    if (v.empty()) return;
    const size_t N = v.size();
    std::vector<std::vector<float>> D(N, std::vector<float>(N, 0.f));
    for (size_t i = 0; i < N; i++)
        for (size_t j = i + 1; j < N; j++) D[i][j] = D[j][i] = (float)hamming(v[i], v[j]);
    int best = INT_MAX, idx = 0;
    for (size_t i = 0; i < N; i++) {
        std::vector<int> d(D[i].begin(), D[i].end());
        std::sort(d.begin(), d.end());
        const int median = d[(size_t)(0.5 * (N - 1))];
        if (median < best) {
            best = median;
            idx = (int)i;
        }
    }
    std::memcpy(P.desc, v[idx], 32);
}

// MapPoint::UpdateNormalAndDepth (MapPoint.cc:285-324)
void update_normal_and_depth(MapPoint& P, const KeyFrame* kf, const Pyramid& py) {
    float normal[3] = {0.f, 0.f, 0.f};
    int n = 0;
    for (auto& o : P.obs) {
        float Ow[3], d[3];
        kf[o.first].center(Ow);
        for (int c = 0; c < 3; c++) d[c] = P.pos[c] - Ow[c];
        const float f = (float)(1.0 / (double)cvnorm(d));
        for (int c = 0; c < 3; c++) normal[c] = normal[c] + d[c] * f;
        n++;
    }
    float Ow[3], PC[3];
    kf[P.ref].center(Ow);
    for (int c = 0; c < 3; c++) PC[c] = P.pos[c] - Ow[c];
    const float dist = cvnorm(PC);
    const int level = py.level(kf[P.ref].kps[P.obs[P.ref]].octave);
    P.min_dist = (1.0f / py.sf) * dist / py.scale[level];
    P.max_dist = py.sf * dist * py.scale[py.nlevels - 1 - level];
    const float fn = (float)(1.0 / (double)n);
    for (int c = 0; c < 3; c++) P.normal[c] = normal[c] * fn;
}

void put(MP& o, const MapPoint& P) {
    for (int c = 0; c < 3; c++) o.pos[c] = P.pos[c], o.normal[c] = P.normal[c];
    o.min_dist = P.min_dist;
    o.max_dist = P.max_dist;
}

}  // namespace

extern "C" {

// -> the number of map points; *status 0 (ok) or 1 (not initialised). Output
// arrays are sized for n1 points / 2 n1 edges; slots1 [n1], slots2 [n2].
int imr_points(const float* cam, int nlevels, float scale_factor, const KP* kps1, const uint8_t* desc1, int n1,
               const KP* kps2, const uint8_t* desc2, int n2, const int32_t* matches12, int ok, const float* R21,
               const float* t21, const float* p3d, const uint8_t* tri, int32_t* status, int32_t* pt_kp, MP* mps,
               uint8_t* mp_desc, int32_t* slots1, int32_t* slots2, float* kf_Tcw, uint8_t* kf_kind, float* kf_cam,
               float* pt_pos, int32_t* edge_pt, int32_t* edge_kf, float* edge_z, float* edge_inv_sigma2) {
    const Pyramid py(nlevels, scale_factor);
    KeyFrame kf[2];
    for (int k = 0; k < 2; k++) {  // :1207-1214
        for (int q = 0; q < 16; q++) kf[k].Tcw[q] = (q % 5 == 0) ? 1.f : 0.f;
        kf[k].kps = k ? kps2 : kps1;
        kf[k].desc = k ? desc2 : desc1;
        kf[k].n = k ? n2 : n1;
        kf[k].slots.assign(kf[k].n, -1);
    }
    if (ok)
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) kf[1].Tcw[4 * i + j] = R21[3 * i + j];
            kf[1].Tcw[4 * i + 3] = t21[i];
        }
    std::vector<MapPoint> pts;
    if (ok) {
        std::vector<int32_t> m(matches12, matches12 + n1);
        for (int i = 0; i < n1; i++)  // :1126-1133 (and a match outside the frame is no match)
            if (m[i] >= 0 && (!tri[i] || m[i] >= n2)) m[i] = -1;
        for (int i = 0; i < n1; i++) {  // :1224-1249
            if (m[i] < 0) continue;
            MapPoint P;
            for (int c = 0; c < 3; c++) P.pos[c] = p3d[3 * i + c];
            P.ref = 1;  // new MapPoint(worldPos, pKFcur, mpMap)
            std::memset(P.desc, 0, 32);
            const int id = (int)pts.size();
            kf[0].slots[i] = id;     // pKFini->AddMapPoint(pMP, i)
            kf[1].slots[m[i]] = id;  // pKFcur->AddMapPoint(pMP, mvIniMatches[i])
            P.obs[0] = i;
            P.obs[1] = m[i];
            distinctive(P, kf);
            update_normal_and_depth(P, kf, py);
            pts.push_back(P);
        }
    }
    *status = ok ? 0 : 1;
    for (int i = 0; i < n1; i++) slots1[i] = kf[0].slots[i];
    for (int i = 0; i < n2; i++) slots2[i] = kf[1].slots[i];
    // the graph (Optimizer.cc:51-115): keyframes by mnId, points by mnId, a point's observations in map order
    for (int k = 0; k < 2; k++) {
        std::memcpy(kf_Tcw + 16 * k, kf[k].Tcw, 64);
        kf_kind[k] = k == 0 ? 1 : 0;  // setFixed(pKF->mnId == 0)
        for (int q = 0; q < 4; q++) kf_cam[4 * k + q] = cam[q];
    }
    int e = 0;
    for (size_t j = 0; j < pts.size(); j++) {
        MapPoint& P = pts[j];
        pt_kp[2 * j] = P.obs[0];
        pt_kp[2 * j + 1] = P.obs[1];
        put(mps[j], P);
        std::memcpy(mp_desc + 32 * j, P.desc, 32);
        for (int c = 0; c < 3; c++) pt_pos[3 * j + c] = P.pos[c];
        for (auto& o : P.obs) {
            const KP& kp = kf[o.first].kps[o.second];
            edge_pt[e] = (int)j;
            edge_kf[e] = o.first;
            edge_z[2 * e] = kp.x;
            edge_z[2 * e + 1] = kp.y;
            edge_inv_sigma2[e] = py.inv_sigma2[py.level(kp.octave)];
            e++;
        }
    }
    return (int)pts.size();
}

// The world after BundleAdjustment wrote ba_Tcw (2 x 16) and ba_pos (npts x 3)
// back. -> status: 0 ok, 2 median depth < 0, 3 too few tracked points (or no
// point at all, where the reference indexes an empty vector).
int imr_finish(int nlevels, float scale_factor, const KP* kps1, int n1, const KP* kps2, int n2, int npts,
               const int32_t* pt_kp, const int32_t* slots1, const int32_t* slots2, const float* ba_Tcw,
               const float* ba_pos, int thres, int32_t* tracked, float* median, float* Tcw_out, MP* mps_out) {
    const Pyramid py(nlevels, scale_factor);
    KeyFrame kf[2];
    for (int k = 0; k < 2; k++) {
        std::memcpy(kf[k].Tcw, ba_Tcw + 16 * k, 64);  // pKF->SetPose (Optimizer.cc:130)
        kf[k].kps = k ? kps2 : kps1;
        kf[k].desc = nullptr;
        kf[k].n = k ? n2 : n1;
        kf[k].slots.assign(k ? slots2 : slots1, (k ? slots2 : slots1) + kf[k].n);
    }
    std::vector<MapPoint> pts(npts);
    for (int j = 0; j < npts; j++) {  // Optimizer.cc:134-140
        MapPoint& P = pts[j];
        P.ref = 1;
        P.obs[0] = pt_kp[2 * j];
        P.obs[1] = pt_kp[2 * j + 1];
        for (int c = 0; c < 3; c++) P.pos[c] = ba_pos[3 * j + c];
        update_normal_and_depth(P, kf, py);
    }
    // pKFini->ComputeSceneMedianDepth(2) (KeyFrame.cc:659-689)
    std::vector<float> depths;
    for (int i = 0; i < n1; i++) {
        const int id = kf[0].slots[i];
        if (id < 0) continue;
        const float* x = pts[id].pos;
        const double d = (double)kf[0].Tcw[8] * (double)x[0] + (double)kf[0].Tcw[9] * (double)x[1] +
                         (double)kf[0].Tcw[10] * (double)x[2];
        depths.push_back((float)(d + (double)kf[0].Tcw[11]));
    }
    std::sort(depths.begin(), depths.end());
    int nt = 0;  // pKFcur->TrackedMapPoints()
    for (int i = 0; i < n2; i++) nt += kf[1].slots[i] >= 0;
    *tracked = nt;
    *median = depths.empty() ? 0.f : depths[(depths.size() - 1) / 2];
    int status = 0;
    if (depths.empty()) status = 3;
    else if (*median < 0) status = 2;
    else if (nt < thres) status = 3;
    if (status == 0) {  // :1282-1299
        const float inv = 1.0f / *median;
        for (int r = 0; r < 3; r++) kf[1].Tcw[4 * r + 3] = kf[1].Tcw[4 * r + 3] * inv;
        for (int i = 0; i < n1; i++) {  // pKFini->GetMapPointMatches()
            const int id = kf[0].slots[i];
            if (id < 0) continue;
            for (int c = 0; c < 3; c++) pts[id].pos[c] = pts[id].pos[c] * inv;
        }
    }
    for (int k = 0; k < 2; k++) std::memcpy(Tcw_out + 16 * k, kf[k].Tcw, 64);
    for (int j = 0; j < npts; j++) put(mps_out[j], pts[j]);
    return status;
}

}  // extern "C"
