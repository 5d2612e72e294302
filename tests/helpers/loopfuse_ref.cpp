// Serial CPU restatement, for the tests, of the map surgery of
// LoopClosing::CorrectLoop: ORBmatcher::Fuse(pKF, Scw, vpPoints, th)
// (ORBmatcher.cc:1710-1839), LoopClosing::SearchAndFuse (LoopClosing.cc:572-585),
// the loop fusion block and the LoopConnections loop (:508-525, :533-552),
// MapPoint::AddObservation / Replace / ComputeDistinctiveDescriptors /
// UpdateNormalAndDepth (MapPoint.cc:77-81, :136-170, :197-262, :285-324),
// KeyFrame::AddConnection / UpdateBestCovisibles / UpdateConnections
// (KeyFrame.cc:126-160, :332-421) and the KeyFrame slot calls they make
// (KeyFrame.cc:200-251, :612-657), over plain arrays. Map points and keyframes
// are indices; every pointer-ordered container is walked in index order
// (docs/ORACLE_ASSUMPTIONS.md A26). Written from the reference, one candidate
// and one keyframe at a time; shares nothing with the code under test.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <set>
#include <vector>

namespace {

enum Exit {
    X_FUSED = 0,
    X_BAD = 1,
    X_FOUND = 2,
    X_DEPTH = 3,
    X_IMAGE = 4,
    X_RANGE = 5,
    X_ANGLE = 6,
    X_WINDOW = 7,
    X_LEVEL = 8,
    X_DIST = 9
};
enum Action { A_NONE = 0, A_ADD = 1, A_REPLACE = 2, A_KEEP = 3 };

const int COLS = 64, ROWS = 48, TH_LOW = 50;

struct KeyFrame {
    std::vector<float> x, y;
    std::vector<int> octave;
    std::vector<uint8_t> desc;  // n x 32
    std::vector<int> slot;      // mvpMapPoints, -1 = NULL
    bool bad = false;
    std::vector<int> grid[COLS][ROWS];
    std::map<int, int> weights;            // mConnectedKeyFrameWeights
    std::vector<int> ordered, ordered_w;   // mvpOrderedConnectedKeyFrames, mvOrderedWeights
    int parent = -1;
    bool first_connection = true;
    float Ow[3] = {0.f, 0.f, 0.f};  // KeyFrame::GetCameraCenter of the pose set last (identity at first)
};

struct MapPoint {
    float pos[3], normal[3], min_dist, max_dist;
    uint8_t desc[32];
    bool bad = false;
    std::map<int, int> obs;  // mObservations: keyframe -> slot
    int ref = -1;            // mpRefKF
};

struct World {
    int min_x, max_x, min_y, max_y;
    float fx, fy, cx, cy;
    float inv_w, inv_h;
    std::vector<float> scales;
    float scale_factor = 1.2f;
    std::vector<KeyFrame> kfs;
    std::vector<MapPoint> mps;
    long erase_branch = 0, same_id = 0;
};

int hamming(const uint8_t* a, const uint8_t* b) {
    int d = 0;
    for (int k = 0; k < 32; k++) d += __builtin_popcount((unsigned)(a[k] ^ b[k]));
    return d;
}

// MapPoint::ComputeDistinctiveDescriptors
void distinctive(World& w, int p) {
    MapPoint& mp = w.mps[p];
    if (mp.bad || mp.obs.empty()) return;
    std::vector<const uint8_t*> rows;
    for (auto& o : mp.obs)
        if (!w.kfs[o.first].bad) rows.push_back(&w.kfs[o.first].desc[(size_t)o.second * 32]);
    if (rows.empty()) return;
    const size_t N = rows.size();
    std::vector<float> D(N * N, 0.f);
    for (size_t i = 0; i < N; i++)
        for (size_t j = i + 1; j < N; j++) D[i * N + j] = D[j * N + i] = (float)hamming(rows[i], rows[j]);
    int best_median = INT_MAX, best = 0;
    for (size_t i = 0; i < N; i++) {
        std::vector<int> v(D.begin() + i * N, D.begin() + (i + 1) * N);
        std::sort(v.begin(), v.end());
        const int median = v[(size_t)(0.5 * (N - 1))];
        if (median < best_median) {
            best_median = median;
            best = (int)i;
        }
    }
    uint8_t tmp[32];
    std::memcpy(tmp, rows[best], 32);
    std::memcpy(mp.desc, tmp, 32);
}

// a.Replace(b)
void replace(World& w, int a, int b) {
    if (a == b) {
        w.same_id++;
        return;
    }
    std::map<int, int> obs;
    obs.swap(w.mps[a].obs);
    w.mps[a].bad = true;
    for (auto& o : obs) {
        KeyFrame& kf = w.kfs[o.first];
        if (!w.mps[b].obs.count(o.first)) {
            kf.slot[o.second] = b;             // ReplaceMapPointMatch
            w.mps[b].obs[o.first] = o.second;  // AddObservation
        } else {
            kf.slot[o.second] = -1;  // EraseMapPointMatch
            w.erase_branch++;
        }
    }
    distinctive(w, b);
}

float norm3(const float* d) {  // cv::norm: a double sum
    return (float)std::sqrt(((double)d[0] * d[0] + (double)d[1] * d[1]) + (double)d[2] * d[2]);
}

// MapPoint::UpdateNormalAndDepth; Mat / scalar is one float factor (float)(1 / scalar) (A22)
void update_normal_and_depth(World& w, int p) {
    MapPoint& mp = w.mps[p];
    if (mp.bad) return;
    // the reference divides by zero without observations: left alone (A26)
    if (mp.obs.empty() || mp.ref < 0 || w.kfs[mp.ref].octave.empty()) return;
    float normal[3] = {0.f, 0.f, 0.f};
    int n = 0;
    for (auto& o : mp.obs) {
        const float* O = w.kfs[o.first].Ow;
        const float d[3] = {mp.pos[0] - O[0], mp.pos[1] - O[1], mp.pos[2] - O[2]};
        const float f = (float)(1.0 / (double)norm3(d));
        for (int c = 0; c < 3; c++) normal[c] = normal[c] + d[c] * f;
        n++;
    }
    const KeyFrame& ref = w.kfs[mp.ref];
    const float pc[3] = {mp.pos[0] - ref.Ow[0], mp.pos[1] - ref.Ow[1], mp.pos[2] - ref.Ow[2]};
    const float dist = norm3(pc);
    auto it = mp.obs.find(mp.ref);
    const int level = ref.octave[it == mp.obs.end() ? 0 : it->second];
    const int nlevels = (int)w.scales.size();
    mp.min_dist = (1.0f / w.scale_factor) * dist / w.scales[level];
    mp.max_dist = w.scale_factor * dist * w.scales[nlevels - 1 - level];
    const float fn = (float)(1.0 / (double)n);
    for (int c = 0; c < 3; c++) mp.normal[c] = normal[c] * fn;
}

// KeyFrame::UpdateBestCovisibles
void update_best_covisibles(KeyFrame& kf) {
    std::vector<std::pair<int, int>> pairs;
    for (auto& e : kf.weights) pairs.push_back({e.second, e.first});
    std::sort(pairs.begin(), pairs.end());
    kf.ordered.clear();
    kf.ordered_w.clear();
    for (size_t i = pairs.size(); i-- > 0;) {  // push_front of the ascending list
        kf.ordered.push_back(pairs[i].second);
        kf.ordered_w.push_back(pairs[i].first);
    }
}

// KeyFrame::AddConnection
void add_connection(KeyFrame& kf, int other, int weight) {
    auto it = kf.weights.find(other);
    if (it != kf.weights.end() && it->second == weight) return;
    kf.weights[other] = weight;
    update_best_covisibles(kf);
}

// KeyFrame::UpdateConnections
void update_connections(World& w, int k) {
    KeyFrame& kf = w.kfs[k];
    std::map<int, int> counter;
    const std::vector<int> slots = kf.slot;
    for (int p : slots) {
        if (p < 0 || w.mps[p].bad) continue;
        for (auto& o : w.mps[p].obs)
            if (o.first != k) counter[o.first]++;
    }
    if (counter.empty()) return;
    int nmax = 0, kmax = -1;
    const int th = 15;
    std::vector<std::pair<int, int>> pairs;
    for (auto& e : counter) {
        if (e.second > nmax) nmax = e.second, kmax = e.first;
        if (e.second >= th) {
            pairs.push_back({e.second, e.first});
            add_connection(w.kfs[e.first], k, e.second);
        }
    }
    if (pairs.empty()) {
        pairs.push_back({nmax, kmax});
        add_connection(w.kfs[kmax], k, nmax);
    }
    std::sort(pairs.begin(), pairs.end());
    kf.weights = counter;
    kf.ordered.clear();
    kf.ordered_w.clear();
    for (size_t i = pairs.size(); i-- > 0;) {
        kf.ordered.push_back(pairs[i].second);
        kf.ordered_w.push_back(pairs[i].first);
    }
    if (kf.first_connection && k != 0) {
        kf.parent = kf.ordered.front();
        kf.first_connection = false;
    }
}

// KeyFrame::GetFeaturesInArea
std::vector<int> features_in_area(const World& w, const KeyFrame& kf, float x, float y, float r) {
    std::vector<int> out;
    int x0 = (int)std::floor((x - w.min_x - r) * w.inv_w);
    x0 = std::max(0, x0);
    if (x0 >= COLS) return out;
    int x1 = (int)std::ceil((x - w.min_x + r) * w.inv_w);
    x1 = std::min(COLS - 1, x1);
    if (x1 < 0) return out;
    int y0 = (int)std::floor((y - w.min_y - r) * w.inv_h);
    y0 = std::max(0, y0);
    if (y0 >= ROWS) return out;
    int y1 = (int)std::ceil((y - w.min_y + r) * w.inv_h);
    y1 = std::min(ROWS - 1, y1);
    if (y1 < 0) return out;
    for (int ix = x0; ix <= x1; ix++)
        for (int iy = y0; iy <= y1; iy++)
            for (int k : kf.grid[ix][iy])
                if (std::fabs(kf.x[k] - x) <= r && std::fabs(kf.y[k] - y) <= r) out.push_back(k);
    return out;
}

struct Pose {
    float R[9], t[3], O[3];
};

// Decompose Scw (:1719-1723), A23's reading
Pose decompose(const float* S) {
    Pose p;
    const double dot = ((double)S[0] * S[0] + (double)S[1] * S[1]) + (double)S[2] * S[2];
    const float scw = (float)std::sqrt(dot);
    const float f = (float)(1.0 / (double)scw);
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) p.R[3 * r + c] = S[4 * r + c] * f;
        p.t[r] = S[4 * r + 3] * f;
    }
    for (int c = 0; c < 3; c++) {
        float acc = p.R[c] * p.t[0];
        acc = acc + p.R[3 + c] * p.t[1];
        acc = acc + p.R[6 + c] * p.t[2];
        p.O[c] = -acc;
    }
    return p;
}

// the search of one candidate (:1739-1816) with descriptor `d`; found = the
// call's spAlreadyFound. Returns the exit; kp / dist set when X_FUSED.
int search(const World& w, const KeyFrame& kf, const Pose& P, const std::set<int>& found, int p, const uint8_t* d,
           float th, int& kp, int& dist) {
    kp = -1;
    dist = -1;
    const MapPoint& mp = w.mps[p];
    if (mp.bad) return X_BAD;
    if (found.count(p)) return X_FOUND;
    float c[3];
    for (int r = 0; r < 3; r++) {
        float acc = P.R[3 * r] * mp.pos[0];
        acc = acc + P.R[3 * r + 1] * mp.pos[1];
        acc = acc + P.R[3 * r + 2] * mp.pos[2];
        c[r] = acc + P.t[r];
    }
    if (c[2] < 0.0f) return X_DEPTH;
    const float invz = (float)(1.0 / (double)c[2]);
    const float xn = c[0] * invz, yn = c[1] * invz;
    const float u = w.fx * xn + w.cx, v = w.fy * yn + w.cy;
    if (!(u >= w.min_x && u < w.max_x && v >= w.min_y && v < w.max_y)) return X_IMAGE;
    const float PO[3] = {mp.pos[0] - P.O[0], mp.pos[1] - P.O[1], mp.pos[2] - P.O[2]};
    const float dist3D = (float)std::sqrt((double)PO[0] * PO[0] + (double)PO[1] * PO[1] + (double)PO[2] * PO[2]);
    if (dist3D < mp.min_dist || dist3D > mp.max_dist) return X_RANGE;
    const double pn = (double)PO[0] * mp.normal[0] + (double)PO[1] * mp.normal[1] + (double)PO[2] * mp.normal[2];
    if (pn < 0.5 * dist3D) return X_ANGLE;
    const float ratio = dist3D / mp.min_dist;
    const int nmax = (int)w.scales.size() - 1;
    const int level = std::min((int)(std::lower_bound(w.scales.begin(), w.scales.end(), ratio) - w.scales.begin()), nmax);
    const float radius = th * w.scales[level];
    const std::vector<int> idx = features_in_area(w, kf, u, v, radius);
    if (idx.empty()) return X_WINDOW;
    int best_dist = INT_MAX, best = -1;
    for (int k : idx) {
        if (kf.octave[k] < level - 1 || kf.octave[k] > level) continue;
        const int dd = hamming(d, &kf.desc[(size_t)k * 32]);
        if (dd < best_dist) {
            best_dist = dd;
            best = k;
        }
    }
    if (best < 0) return X_LEVEL;
    if (best_dist > TH_LOW) return X_DIST;
    kp = best;
    dist = best_dist;
    return X_FUSED;
}

// One Fuse call. stale (optional): descriptors as they were before
// SearchAndFuse began; stale_kp[i] = what the search would pick with them.
int fuse(World& w, int k, const float* Scw, const int* pts, int m, float th, int apply, int* kp, int* dist, int* exit_,
         int* action, int* replaced, const uint8_t* stale, int* stale_kp) {
    KeyFrame& kf = w.kfs[k];
    const Pose P = decompose(Scw);
    std::set<int> found;  // KeyFrame::GetMapPoints
    for (int s : kf.slot)
        if (s >= 0 && !w.mps[s].bad) found.insert(s);
    int nfused = 0;
    for (int i = 0; i < m; i++) {
        const int p = pts[i];
        action[i] = A_NONE;
        replaced[i] = -1;
        if (stale_kp) {
            int sd;
            search(w, kf, P, found, p, stale + (size_t)p * 32, th, stale_kp[i], sd);
        }
        uint8_t d[32];
        std::memcpy(d, w.mps[p].desc, 32);  // GetDescriptor().clone()
        exit_[i] = search(w, kf, P, found, p, d, th, kp[i], dist[i]);
        if (exit_[i] != X_FUSED) continue;
        nfused++;
        if (!apply) continue;
        const int in_kf = kf.slot[kp[i]];
        if (in_kf >= 0) {
            if (!w.mps[in_kf].bad) {
                action[i] = A_REPLACE;
                replaced[i] = in_kf;
                replace(w, in_kf, p);
            } else {
                action[i] = A_KEEP;
                replaced[i] = in_kf;
            }
        } else {
            w.mps[p].obs[k] = kp[i];
            kf.slot[kp[i]] = p;
            action[i] = A_ADD;
        }
    }
    return nfused;
}

}  // namespace

extern "C" {

void* lf_create(const int* bounds, const float* K, int nlevels, const float* scales, int nkf, const int* kf_off,
                const float* kx, const float* ky, const int* koct, const uint8_t* kdesc, const int* slots,
                const uint8_t* kf_bad, int nmp, const float* pos, const float* normal, const float* min_dist,
                const float* max_dist, const uint8_t* mp_desc, const uint8_t* mp_bad, int nobs, const int* obs_pt,
                const int* obs_kf, const int* obs_slot) {
    World* w = new World;
    w->min_x = bounds[0], w->max_x = bounds[1], w->min_y = bounds[2], w->max_y = bounds[3];
    w->fx = K[0], w->fy = K[1], w->cx = K[2], w->cy = K[3];
    w->inv_w = (float)COLS / (float)(w->max_x - w->min_x);
    w->inv_h = (float)ROWS / (float)(w->max_y - w->min_y);
    w->scales.assign(scales, scales + nlevels);
    w->kfs.resize(nkf);
    for (int k = 0; k < nkf; k++) {
        KeyFrame& kf = w->kfs[k];
        const int a = kf_off[k], b = kf_off[k + 1];
        kf.x.assign(kx + a, kx + b);
        kf.y.assign(ky + a, ky + b);
        kf.octave.assign(koct + a, koct + b);
        kf.desc.assign(kdesc + (size_t)a * 32, kdesc + (size_t)b * 32);
        kf.slot.assign(slots + a, slots + b);
        kf.bad = kf_bad && kf_bad[k];
        for (int i = 0; i < b - a; i++) {  // Frame::PosInGrid
            const int px = (int)std::round((kf.x[i] - w->min_x) * w->inv_w);
            const int py = (int)std::round((kf.y[i] - w->min_y) * w->inv_h);
            if (px < 0 || px >= COLS || py < 0 || py >= ROWS) continue;
            kf.grid[px][py].push_back(i);
        }
    }
    w->mps.resize(nmp);
    for (int p = 0; p < nmp; p++) {
        MapPoint& mp = w->mps[p];
        for (int c = 0; c < 3; c++) mp.pos[c] = pos[3 * p + c], mp.normal[c] = normal[3 * p + c];
        mp.min_dist = min_dist[p], mp.max_dist = max_dist[p];
        std::memcpy(mp.desc, mp_desc + (size_t)p * 32, 32);
        mp.bad = mp_bad && mp_bad[p];
    }
    for (int o = 0; o < nobs; o++) w->mps[obs_pt[o]].obs[obs_kf[o]] = obs_slot[o];
    return w;
}

void lf_destroy(void* h) { delete (World*)h; }

int lf_fuse(void* h, int kf, const float* Scw, const int* pts, int m, float th, int apply, int* kp, int* dist,
            int* exit_, int* action, int* replaced) {
    return fuse(*(World*)h, kf, Scw, pts, m, th, apply, kp, dist, exit_, action, replaced, nullptr, nullptr);
}

// LoopClosing::SearchAndFuse: the keyframes of CorrectedSim3 in index order,
// every output [nk][m]
void lf_search_and_fuse(void* h, int nk, const int* kfs, const float* Scw, const int* pts, int m, float th, int* kp,
                        int* dist, int* exit_, int* action, int* replaced, int* stale_kp, int* nfused) {
    World& w = *(World*)h;
    std::vector<uint8_t> stale((size_t)w.mps.size() * 32);
    for (size_t p = 0; p < w.mps.size(); p++) std::memcpy(&stale[p * 32], w.mps[p].desc, 32);
    for (int j = 0; j < nk; j++) {
        const size_t o = (size_t)j * m;
        nfused[j] = fuse(w, kfs[j], Scw + 16 * j, pts, m, th, 1, kp + o, dist + o, exit_ + o, action + o, replaced + o,
                         stale.data(), stale_kp + o);
    }
}

void lf_replace(void* h, int a, int b) { replace(*(World*)h, a, b); }
void lf_add_observation(void* h, int p, int kf, int slot) { ((World*)h)->mps[p].obs[kf] = slot; }
void lf_add_map_point(void* h, int kf, int p, int slot) { ((World*)h)->kfs[kf].slot[slot] = p; }
void lf_distinctive(void* h, int p) { distinctive(*(World*)h, p); }
long lf_counter(void* h, int which) { return which == 0 ? ((World*)h)->erase_branch : ((World*)h)->same_id; }

void lf_set_scale_factor(void* h, float f) { ((World*)h)->scale_factor = f; }
// KeyFrame::SetPose: Ow = -Rcw^T tcw (A1)
void lf_set_pose(void* h, int kf, const float* T) {
    float* O = ((World*)h)->kfs[kf].Ow;
    for (int c = 0; c < 3; c++) {
        float acc = T[c] * T[3];
        acc = acc + T[4 + c] * T[7];
        acc = acc + T[8 + c] * T[11];
        O[c] = -acc;
    }
}
void lf_set_ref(void* h, int p, int ref) { ((World*)h)->mps[p].ref = ref; }
void lf_set_pos(void* h, int p, const float* x) {
    for (int c = 0; c < 3; c++) ((World*)h)->mps[p].pos[c] = x[c];
}
void lf_update_normal_and_depth(void* h, int p) { update_normal_and_depth(*(World*)h, p); }
// per point: pos[3], normal[3], min_dist, max_dist
void lf_get_geometry(void* h, float* out) {
    for (auto& mp : ((World*)h)->mps) {
        for (int c = 0; c < 3; c++) out[c] = mp.pos[c], out[3 + c] = mp.normal[c];
        out[6] = mp.min_dist, out[7] = mp.max_dist;
        out += 8;
    }
}

void lf_update_connections(void* h, int kf) { update_connections(*(World*)h, kf); }
// the ordered covisibles of kf as (keyframe, weight) rows, then its weight map
// as (keyframe, weight) rows in keyframe order; counts in n[0], n[1]; parent in n[2]
void lf_get_connections(void* h, int kf, int cap, int* ordered, int* weights, int* n) {
    KeyFrame& k = ((World*)h)->kfs[kf];
    n[0] = (int)k.ordered.size(), n[1] = (int)k.weights.size(), n[2] = k.parent;
    for (int i = 0; i < n[0] && i < cap; i++) ordered[2 * i] = k.ordered[i], ordered[2 * i + 1] = k.ordered_w[i];
    int i = 0;
    for (auto& e : k.weights) {
        if (i < cap) weights[2 * i] = e.first, weights[2 * i + 1] = e.second;
        i++;
    }
}
// the loop fusion block (LoopClosing.cc:508-525): matched[i] = the loop point
// matched to slot i of the current keyframe, -1 = NULL
void lf_loop_fusion(void* h, int cur, const int* matched, int n) {
    World& w = *(World*)h;
    for (int i = 0; i < n; i++) {
        if (matched[i] < 0) continue;
        const int loop_mp = matched[i], cur_mp = w.kfs[cur].slot[i];
        if (cur_mp >= 0) {
            replace(w, cur_mp, loop_mp);
        } else {
            w.kfs[cur].slot[i] = loop_mp;
            w.mps[loop_mp].obs[cur] = i;
            distinctive(w, loop_mp);
        }
    }
}
// the LoopConnections loop (LoopClosing.cc:533-552) over mvpCurrentConnectedKFs;
// (keyframe, new neighbour) rows in keyframe order; returns the count
int lf_loop_connections(void* h, int nk, const int* connected, int cap, int* out) {
    World& w = *(World*)h;
    std::map<int, std::set<int>> lc;
    for (int j = 0; j < nk; j++) {
        const int k = connected[j];
        const std::vector<int> previous = w.kfs[k].ordered;
        update_connections(w, k);
        std::set<int>& sset = lc[k];
        for (auto& e : w.kfs[k].weights) sset.insert(e.first);
        for (int q : previous) sset.erase(q);
        for (int j2 = 0; j2 < nk; j2++) sset.erase(connected[j2]);
    }
    int n = 0;
    for (auto& e : lc)
        for (int q : e.second) {
            if (n < cap) out[2 * n] = e.first, out[2 * n + 1] = q;
            n++;
        }
    return n;
}

void lf_get_slots(void* h, int* out) {
    for (auto& kf : ((World*)h)->kfs) out = std::copy(kf.slot.begin(), kf.slot.end(), out);
}
void lf_get_points(void* h, uint8_t* bad, uint8_t* desc) {
    World& w = *(World*)h;
    for (size_t p = 0; p < w.mps.size(); p++) {
        bad[p] = w.mps[p].bad;
        std::memcpy(desc + p * 32, w.mps[p].desc, 32);
    }
}
// observation maps as (point, keyframe, slot) rows, point-major, keyframe order; returns the count
int lf_get_obs(void* h, int cap, int* out) {
    World& w = *(World*)h;
    int n = 0;
    for (size_t p = 0; p < w.mps.size(); p++)
        for (auto& o : w.mps[p].obs) {
            if (n < cap) out[3 * n] = (int)p, out[3 * n + 1] = o.first, out[3 * n + 2] = o.second;
            n++;
        }
    return n;
}

}  // extern "C"
