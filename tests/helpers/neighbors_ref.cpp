// Serial CPU restatement, for the tests, of LocalMapping::SearchInNeighbors
// (LocalMapping.cc:411-488) and what it calls: ORBmatcher::Fuse(pKF,
// vpMapPoints, th) (ORBmatcher.cc:1590-1707), MapPoint::AddObservation /
// Replace / ComputeDistinctiveDescriptors / UpdateNormalAndDepth
// (MapPoint.cc:77-81, :136-170, :197-262, :285-324), KeyFrame::AddConnection /
// UpdateBestCovisibles / UpdateConnections (KeyFrame.cc:126-160, :332-421),
// KeyFrame::GetFeaturesInArea / IsInImage (KeyFrame.cc:612-657), over plain
// arrays. Map points and keyframes are indices; every pointer-ordered
// container is walked in index order (docs/ORACLE_ASSUMPTIONS.md A26); the two
// fuse markers start at -1 (A28). Written from the reference, one candidate and
// one keyframe at a time; shares nothing with the code under test.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <vector>

namespace {

enum Exit {
    X_FUSED = 0,
    X_NULL = 1,
    X_BAD = 2,
    X_INKF = 3,
    X_DEPTH = 4,
    X_IMAGE = 5,
    X_RANGE = 6,
    X_ANGLE = 7,
    X_WINDOW = 8,
    X_LEVEL = 9,
    X_DIST = 10
};
enum Action { A_NONE = 0, A_ADD = 1, A_REPLACE = 2, A_KEEP = 3 };

const int COLS = 64, ROWS = 48, TH_LOW = 50;

struct KeyFrame {
    long id = 0;  // mnId
    std::vector<float> x, y;
    std::vector<int> octave;
    std::vector<uint8_t> desc;  // n x 32
    std::vector<int> slot;      // mvpMapPoints, -1 = NULL
    bool bad = false;
    std::vector<int> grid[COLS][ROWS];
    std::map<int, int> weights;           // mConnectedKeyFrameWeights
    std::vector<int> ordered, ordered_w;  // mvpOrderedConnectedKeyFrames, mvOrderedWeights
    int parent = -1;
    bool first_connection = true;
    float R[9], t[3], Ow[3];       // GetRotation, GetTranslation, GetCameraCenter
    long fuse_target_for = -1;     // mnFuseTargetForKF
};

struct MapPoint {
    float pos[3], normal[3], min_dist, max_dist;
    uint8_t desc[32];
    bool bad = false;
    std::map<int, int> obs;  // mObservations: keyframe -> slot
    int ref = -1;            // mpRefKF
    long fuse_candidate_for = -1;  // mnFuseCandidateForKF
};

// what one SearchInNeighbors call did
struct Report {
    std::vector<int> targets, nfused;                                 // per target
    std::vector<int> f_kp, f_dist, f_exit, f_action, f_other, f_stale;  // [ntargets][ncand]
    std::vector<int> cand, b_kp, b_dist, b_exit, b_action, b_other, b_stale;
    std::vector<int> updated;
    // the exits on the map as it stood when the forward calls, and then the backward call, began
    std::vector<int> f_exit0, b_exit0;
    int ncand = 0, b_nfused = 0, skipped_bad_kf = 0;
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
    Report rep;
};

int hamming(const uint8_t* a, const uint8_t* b) {
    int d = 0;
    for (int k = 0; k < 32; k++) d += __builtin_popcount((unsigned)(a[k] ^ b[k]));
    return d;
}

// KeyFrame::SetPose: Ow = -Rcw^T tcw (A1)
void set_pose(KeyFrame& kf, const float* T) {
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) kf.R[3 * r + c] = T[4 * r + c];
        kf.t[r] = T[4 * r + 3];
    }
    for (int c = 0; c < 3; c++) {
        const float a = kf.R[c] * kf.t[0], b = kf.R[3 + c] * kf.t[1], d = kf.R[6 + c] * kf.t[2];
        kf.Ow[c] = -((a + b) + d);
    }
}

// MapPoint::ComputeDistinctiveDescriptors (MapPoint.cc:197-262)
void distinctive(World& w, int p) {
    MapPoint& mp = w.mps[p];
    if (mp.bad || mp.obs.empty()) return;
    std::vector<const uint8_t*> rows;
    for (auto& o : mp.obs)
        if (!w.kfs[o.first].bad) rows.push_back(&w.kfs[o.first].desc[(size_t)o.second * 32]);
    if (rows.empty()) return;
    const size_t N = rows.size();
    std::vector<int> D(N * N, 0);
    for (size_t i = 0; i < N; i++)
        for (size_t j = i + 1; j < N; j++) D[i * N + j] = D[j * N + i] = hamming(rows[i], rows[j]);
    int best_median = INT_MAX;
    size_t best = 0;
    for (size_t i = 0; i < N; i++) {
        std::vector<int> v(D.begin() + i * N, D.begin() + (i + 1) * N);
        std::sort(v.begin(), v.end());
        const int median = v[(size_t)(0.5 * (N - 1))];
        if (median < best_median) {
            best_median = median;
            best = i;
        }
    }
    uint8_t tmp[32];
    std::memcpy(tmp, rows[best], 32);
    std::memcpy(mp.desc, tmp, 32);
}

// a.Replace(b) (MapPoint.cc:136-170)
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

// MapPoint::UpdateNormalAndDepth (MapPoint.cc:285-324); Mat / scalar is one float factor (A22)
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

// KeyFrame::UpdateBestCovisibles (KeyFrame.cc:141-160)
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

// KeyFrame::AddConnection (KeyFrame.cc:126-139)
void add_connection(KeyFrame& kf, int other, int weight) {
    auto it = kf.weights.find(other);
    if (it != kf.weights.end() && it->second == weight) return;
    kf.weights[other] = weight;
    update_best_covisibles(kf);
}

// KeyFrame::UpdateConnections (KeyFrame.cc:332-421)
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
    std::vector<std::pair<int, int>> pairs;
    for (auto& e : counter) {
        if (e.second > nmax) nmax = e.second, kmax = e.first;
        if (e.second >= 15) {
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

// KeyFrame::GetFeaturesInArea (KeyFrame.cc:612-652)
std::vector<int> features_in_area(const World& w, const KeyFrame& kf, float x, float y, float r) {
    std::vector<int> out;
    const int x0 = std::max(0, (int)std::floor((x - w.min_x - r) * w.inv_w));
    if (x0 >= COLS) return out;
    const int x1 = std::min(COLS - 1, (int)std::ceil((x - w.min_x + r) * w.inv_w));
    if (x1 < 0) return out;
    const int y0 = std::max(0, (int)std::floor((y - w.min_y - r) * w.inv_h));
    if (y0 >= ROWS) return out;
    const int y1 = std::min(ROWS - 1, (int)std::ceil((y - w.min_y + r) * w.inv_h));
    if (y1 < 0) return out;
    for (int ix = x0; ix <= x1; ix++)
        for (int iy = y0; iy <= y1; iy++)
            for (int k : kf.grid[ix][iy])
                if (std::fabs(kf.x[k] - x) <= r && std::fabs(kf.y[k] - y) <= r) out.push_back(k);
    return out;
}

// the body of one candidate of Fuse (:1609-1690) with descriptor d: the exit;
// kp / dist set when X_FUSED
int search(const World& w, int k, int p, const uint8_t* d, float th, int& kp, int& dist) {
    kp = -1;
    dist = -1;
    if (p < 0) return X_NULL;
    const KeyFrame& kf = w.kfs[k];
    const MapPoint& mp = w.mps[p];
    if (mp.bad) return X_BAD;
    if (mp.obs.count(k)) return X_INKF;
    float c[3];
    for (int r = 0; r < 3; r++) {  // Rcw * p3Dw + tcw
        const float a = kf.R[3 * r] * mp.pos[0], b = kf.R[3 * r + 1] * mp.pos[1], e = kf.R[3 * r + 2] * mp.pos[2];
        c[r] = ((a + b) + e) + kf.t[r];
    }
    if (c[2] < 0.0f) return X_DEPTH;
    const float invz = 1 / c[2];
    const float xn = c[0] * invz, yn = c[1] * invz;
    const float u = w.fx * xn + w.cx, v = w.fy * yn + w.cy;
    if (!(u >= w.min_x && u < w.max_x && v >= w.min_y && v < w.max_y)) return X_IMAGE;
    const float PO[3] = {mp.pos[0] - kf.Ow[0], mp.pos[1] - kf.Ow[1], mp.pos[2] - kf.Ow[2]};
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
    for (int i : idx) {
        if (kf.octave[i] < level - 1 || kf.octave[i] > level) continue;
        const int dd = hamming(d, &kf.desc[(size_t)i * 32]);
        if (dd < best_dist) {
            best_dist = dd;
            best = i;
        }
    }
    if (best < 0) return X_LEVEL;
    if (best_dist > TH_LOW) return X_DIST;
    kp = best;
    dist = best_dist;
    return X_FUSED;
}

// One Fuse(k, pts) call. stale (optional): descriptors saved earlier;
// stale_kp[i] = what the search picks with them on the map as it is at i's turn.
int fuse(World& w, int k, const int* pts, int m, float th, int apply, int* kp, int* dist, int* exit_, int* action,
         int* other, const uint8_t* stale, int* stale_kp) {
    KeyFrame& kf = w.kfs[k];
    int nfused = 0;
    for (int i = 0; i < m; i++) {
        const int p = pts[i];
        action[i] = A_NONE;
        other[i] = -1;
        if (stale_kp) {
            int sd;
            search(w, k, p, p >= 0 ? stale + (size_t)p * 32 : nullptr, th, stale_kp[i], sd);
        }
        uint8_t d[32] = {0};
        if (p >= 0) std::memcpy(d, w.mps[p].desc, 32);
        exit_[i] = search(w, k, p, d, th, kp[i], dist[i]);
        if (exit_[i] != X_FUSED) continue;
        nfused++;
        if (!apply) continue;
        const int in_kf = kf.slot[kp[i]];
        if (in_kf >= 0) {
            other[i] = in_kf;
            if (!w.mps[in_kf].bad) {
                action[i] = A_REPLACE;
                replace(w, p, in_kf);  // pMP->Replace(pMPinKF)
            } else {
                action[i] = A_KEEP;
            }
        } else {
            w.mps[p].obs[k] = kp[i];  // AddObservation
            kf.slot[kp[i]] = p;       // AddMapPoint
            action[i] = A_ADD;
        }
    }
    return nfused;
}

std::vector<uint8_t> all_descriptors(const World& w) {
    std::vector<uint8_t> d((size_t)w.mps.size() * 32);
    for (size_t p = 0; p < w.mps.size(); p++) std::memcpy(&d[p * 32], w.mps[p].desc, 32);
    return d;
}

// LocalMapping::SearchInNeighbors
void search_in_neighbors(World& w, int cur, float th) {
    Report& R = w.rep;
    R = Report();
    KeyFrame& C = w.kfs[cur];
    std::vector<int> first(C.ordered.begin(), C.ordered.begin() + std::min<size_t>(20, C.ordered.size()));
    for (int k : first) {
        KeyFrame& kf = w.kfs[k];
        if (kf.bad) R.skipped_bad_kf++;
        if (kf.bad || kf.fuse_target_for == C.id) continue;
        R.targets.push_back(k);
        kf.fuse_target_for = C.id;
        std::vector<int> second(kf.ordered.begin(), kf.ordered.begin() + std::min<size_t>(5, kf.ordered.size()));
        for (int k2 : second) {
            const KeyFrame& kf2 = w.kfs[k2];
            if (kf2.bad) R.skipped_bad_kf++;
            if (kf2.bad || kf2.fuse_target_for == C.id || kf2.id == C.id) continue;
            R.targets.push_back(k2);
        }
    }
    const size_t nt = R.targets.size();
    // from the current keyframe into the targets
    const std::vector<int> matches = C.slot;  // taken once (:438)
    const int m = R.ncand = (int)matches.size();
    for (auto* v : {&R.f_kp, &R.f_dist, &R.f_exit, &R.f_action, &R.f_other, &R.f_stale}) v->assign(nt * (size_t)m, -1);
    R.nfused.assign(nt, 0);
    const std::vector<uint8_t> stale = all_descriptors(w);
    R.f_exit0.assign(nt * (size_t)m, -1);
    {
        std::vector<int> t0(m), t1(m), t2(m), t3(m);
        for (size_t j = 0; j < nt; j++)
            fuse(w, R.targets[j], matches.data(), m, th, 0, t0.data(), t1.data(), R.f_exit0.data() + j * (size_t)m,
                 t2.data(), t3.data(), nullptr, nullptr);
    }
    for (size_t j = 0; j < nt; j++) {
        const size_t o = j * (size_t)m;
        R.nfused[j] = fuse(w, R.targets[j], matches.data(), m, th, 1, R.f_kp.data() + o, R.f_dist.data() + o,
                           R.f_exit.data() + o, R.f_action.data() + o, R.f_other.data() + o, stale.data(),
                           R.f_stale.data() + o);
    }
    // from the targets into the current keyframe
    for (size_t j = 0; j < nt; j++) {
        const std::vector<int> slots = w.kfs[R.targets[j]].slot;
        for (int p : slots) {
            if (p < 0) continue;
            MapPoint& mp = w.mps[p];
            if (mp.bad || mp.fuse_candidate_for == C.id) continue;
            mp.fuse_candidate_for = C.id;
            R.cand.push_back(p);
        }
    }
    const int nc = (int)R.cand.size();
    for (auto* v : {&R.b_kp, &R.b_dist, &R.b_exit, &R.b_action, &R.b_other, &R.b_stale}) v->assign((size_t)nc, -1);
    const std::vector<uint8_t> stale2 = all_descriptors(w);
    R.b_exit0.assign((size_t)nc, -1);
    {
        std::vector<int> t0(nc), t1(nc), t2(nc), t3(nc);
        fuse(w, cur, R.cand.data(), nc, th, 0, t0.data(), t1.data(), R.b_exit0.data(), t2.data(), t3.data(), nullptr,
             nullptr);
    }
    R.b_nfused = fuse(w, cur, R.cand.data(), nc, th, 1, R.b_kp.data(), R.b_dist.data(), R.b_exit.data(),
                      R.b_action.data(), R.b_other.data(), stale2.data(), R.b_stale.data());
    // update points
    const std::vector<int> after = C.slot;
    for (int p : after) {
        if (p < 0 || w.mps[p].bad) continue;
        distinctive(w, p);
        update_normal_and_depth(w, p);
        R.updated.push_back(p);
    }
    update_connections(w, cur);
}

}  // namespace

extern "C" {

void* nr_create(const int* bounds, const float* K, int nlevels, const float* scales, float scale_factor, int nkf,
                const int* kf_off, const float* kx, const float* ky, const int* koct, const uint8_t* kdesc,
                const int* slots, const uint8_t* kf_bad, const float* kf_Tcw, const int* kf_id, int nmp,
                const float* pos, const float* normal, const float* min_dist, const float* max_dist,
                const uint8_t* mp_desc, const uint8_t* mp_bad, const int* ref_kf, int nobs, const int* obs_pt,
                const int* obs_kf, const int* obs_slot) {
    World* w = new World;
    w->min_x = bounds[0], w->max_x = bounds[1], w->min_y = bounds[2], w->max_y = bounds[3];
    w->fx = K[0], w->fy = K[1], w->cx = K[2], w->cy = K[3];
    w->inv_w = (float)COLS / (float)(w->max_x - w->min_x);
    w->inv_h = (float)ROWS / (float)(w->max_y - w->min_y);
    w->scales.assign(scales, scales + nlevels);
    w->scale_factor = scale_factor;
    w->kfs.resize(nkf);
    for (int k = 0; k < nkf; k++) {
        KeyFrame& kf = w->kfs[k];
        const int a = kf_off[k], b = kf_off[k + 1];
        kf.id = kf_id[k];
        kf.x.assign(kx + a, kx + b);
        kf.y.assign(ky + a, ky + b);
        kf.octave.assign(koct + a, koct + b);
        kf.desc.assign(kdesc + (size_t)a * 32, kdesc + (size_t)b * 32);
        kf.slot.assign(slots + a, slots + b);
        kf.bad = kf_bad && kf_bad[k];
        set_pose(kf, kf_Tcw + 16 * (size_t)k);
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
        mp.ref = ref_kf[p];
    }
    for (int o = 0; o < nobs; o++) w->mps[obs_pt[o]].obs[obs_kf[o]] = obs_slot[o];
    return w;
}

void nr_destroy(void* h) { delete (World*)h; }

int nr_fuse(void* h, int kf, const int* pts, int m, float th, int apply, int* kp, int* dist, int* exit_, int* action,
            int* other) {
    return fuse(*(World*)h, kf, pts, m, th, apply, kp, dist, exit_, action, other, nullptr, nullptr);
}

void nr_replace(void* h, int a, int b) { replace(*(World*)h, a, b); }
void nr_set_bad_kf(void* h, int kf, int bad) { ((World*)h)->kfs[kf].bad = bad != 0; }
void nr_update_normal_and_depth(void* h, int p) { update_normal_and_depth(*(World*)h, p); }
void nr_update_connections(void* h, int kf) { update_connections(*(World*)h, kf); }
void nr_search_in_neighbors(void* h, int cur, float th) { search_in_neighbors(*(World*)h, cur, th); }
long nr_counter(void* h, int which) { return which == 0 ? ((World*)h)->erase_branch : ((World*)h)->same_id; }

// a field of the last SearchInNeighbors report; returns its length (out may be null)
int nr_report(void* h, int which, int* out) {
    const Report& R = ((World*)h)->rep;
    const std::vector<int> scalars = {R.ncand, R.b_nfused, R.skipped_bad_kf};
    const std::vector<int>* f[] = {&R.targets, &R.nfused, &R.f_kp,  &R.f_dist,   &R.f_exit,  &R.f_action,
                                   &R.f_other, &R.f_stale, &R.cand, &R.b_kp,     &R.b_dist,  &R.b_exit,
                                   &R.b_action, &R.b_other, &R.b_stale, &R.updated, &scalars, &R.f_exit0, &R.b_exit0};
    if (which < 0 || which >= (int)(sizeof(f) / sizeof(f[0]))) return -1;
    if (out) std::copy(f[which]->begin(), f[which]->end(), out);
    return (int)f[which]->size();
}

// per point: pos[3], normal[3], min_dist, max_dist
void nr_get_geometry(void* h, float* out) {
    for (auto& mp : ((World*)h)->mps) {
        for (int c = 0; c < 3; c++) out[c] = mp.pos[c], out[3 + c] = mp.normal[c];
        out[6] = mp.min_dist, out[7] = mp.max_dist;
        out += 8;
    }
}
// the ordered covisibles of kf as (keyframe, weight) rows, then its weight map
// as (keyframe, weight) rows in keyframe order; counts in n[0], n[1]; parent in n[2]
void nr_get_connections(void* h, int kf, int cap, int* ordered, int* weights, int* n) {
    KeyFrame& k = ((World*)h)->kfs[kf];
    n[0] = (int)k.ordered.size(), n[1] = (int)k.weights.size(), n[2] = k.parent;
    for (int i = 0; i < n[0] && i < cap; i++) ordered[2 * i] = k.ordered[i], ordered[2 * i + 1] = k.ordered_w[i];
    int i = 0;
    for (auto& e : k.weights) {
        if (i < cap) weights[2 * i] = e.first, weights[2 * i + 1] = e.second;
        i++;
    }
}
void nr_get_slots(void* h, int* out) {
    for (auto& kf : ((World*)h)->kfs) out = std::copy(kf.slot.begin(), kf.slot.end(), out);
}
void nr_get_points(void* h, uint8_t* bad, uint8_t* desc) {
    World& w = *(World*)h;
    for (size_t p = 0; p < w.mps.size(); p++) {
        bad[p] = w.mps[p].bad;
        std::memcpy(desc + p * 32, w.mps[p].desc, 32);
    }
}
void nr_get_markers(void* h, long* kf_marker, long* mp_marker) {
    World& w = *(World*)h;
    for (size_t k = 0; k < w.kfs.size(); k++) kf_marker[k] = w.kfs[k].fuse_target_for;
    for (size_t p = 0; p < w.mps.size(); p++) mp_marker[p] = w.mps[p].fuse_candidate_for;
}
// observation maps as (point, keyframe, slot) rows, point-major, keyframe order; returns the count
int nr_get_obs(void* h, int cap, int* out) {
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
