// The tests' serial restatement of Optimizer::LocalBundleAdjustment on a map
// (src/Optimizer.cc:1515-1764) without the solver: the breadth-first gather
// (:1517-1566), the vertices and edges (:1584-1675) as the arrays gf_ba_problem
// takes, and the outlier erasure and write-back (:1681-1763) applied from a
// given result, with KeyFrame::EraseMapPointMatch, MapPoint::EraseObservation
// (src/MapPoint.cc:83-103), SetBadFlag (:117-131) and UpdateNormalAndDepth
// (:285-324).
//
// Written from the reference's behaviour with std::list / std::map keyed by
// keyframe index (docs/ORACLE_ASSUMPTIONS.md A26, A30) on a world copied from
// the LoopMap; it shares no code with gf_orb_slam_amd/localmapping.py,
// loopmap.py or csrc/lbagraph.hip.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <list>
#include <map>
#include <set>
#include <vector>

namespace {

struct KeyFrame {
    int id = 0, off = 0;
    bool bad = false;
    std::vector<int> octave, slots;
    std::vector<float> xy;
    float T[16];
    long local_for = -1, fixed_for = -1;  // mnBALocalForKF, mnBAFixedForKF
};

struct MapPoint {
    bool bad = false;
    std::map<int, int> obs;  // keyframe -> slot
    int ref = -1;
    float pos[3], normal[3], min_dist = 0.f, max_dist = 0.f;
    long local_for = -1;  // mnBALocalForKF
};

struct World {
    std::vector<KeyFrame> kf;
    std::vector<MapPoint> mp;
    float cam[4];
    std::vector<float> inv_sigma2, scales;
    float scale_factor = 1.2f;
    // the graph of the last lr_graph, in gf_ba_problem's orders
    std::vector<int> local_kfs, fixed_kfs, local_pts;  // lLocalKeyFrames, lFixedCameras, lLocalMapPoints
    std::vector<int> prob_kf, kf_kind, prob_pt, edge_pt, edge_kf, edge_gkp;
    std::vector<int> edge_map_pt, edge_map_kf;  // vpMapPointEdge, vpEdgeKF
    std::vector<float> kf_Tcw, kf_cam, pt_pos, edge_z, edge_inv_sigma2;
    // what the last lr_apply did
    std::vector<int> erased1, erased2, points_bad, bad_round2, stale;
};

// MapPoint.cc:117-131
void set_bad_point(World& w, int p) {
    MapPoint& P = w.mp[p];
    P.bad = true;
    std::map<int, int> obs;
    obs.swap(P.obs);
    for (auto& e : obs) w.kf[e.first].slots[e.second] = -1;  // EraseMapPointMatch(idx)
    w.points_bad.push_back(p);
}

// MapPoint.cc:83-103; begin() of an empty map is not dereferenced: mpRefKF stays (A30)
bool erase_observation(World& w, int p, int k) {
    MapPoint& P = w.mp[p];
    bool bad = false;
    if (P.obs.count(k)) {
        P.obs.erase(k);
        if (P.ref == k && !P.obs.empty()) P.ref = P.obs.begin()->first;
        if (P.obs.size() <= 2) bad = true;
    }
    if (bad) set_bad_point(w, p);
    return bad;
}

// KeyFrame::EraseMapPointMatch(MapPoint*): through GetIndexInKeyFrame
void erase_map_point_match(World& w, int k, int p) {
    auto it = w.mp[p].obs.find(k);
    if (it != w.mp[p].obs.end()) w.kf[k].slots[it->second] = -1;
}

void camera_centre(const float* T, float* O) {  // -Rcw^T tcw in float
    for (int c = 0; c < 3; c++) {
        const float a = T[c] * T[3], b = T[4 + c] * T[7], d = T[8 + c] * T[11];
        O[c] = -((a + b) + d);
    }
}

float norm3(const float* d) {  // cv::norm: a double sum
    return (float)std::sqrt(((double)d[0] * d[0] + (double)d[1] * d[1]) + (double)d[2] * d[2]);
}

// MapPoint.cc:285-324; Mat / scalar is one float factor (A22)
void update_normal_and_depth(World& w, int p) {
    MapPoint& mp = w.mp[p];
    if (mp.bad) return;
    // the reference divides by zero without observations: left alone (A26)
    if (mp.obs.empty() || mp.ref < 0 || w.kf[mp.ref].octave.empty()) return;
    float normal[3] = {0.f, 0.f, 0.f}, O[3];
    int n = 0;
    for (auto& o : mp.obs) {
        camera_centre(w.kf[o.first].T, O);
        const float d[3] = {mp.pos[0] - O[0], mp.pos[1] - O[1], mp.pos[2] - O[2]};
        const float f = (float)(1.0 / (double)norm3(d));
        for (int c = 0; c < 3; c++) normal[c] = normal[c] + d[c] * f;
        n++;
    }
    const KeyFrame& ref = w.kf[mp.ref];
    camera_centre(ref.T, O);
    const float pc[3] = {mp.pos[0] - O[0], mp.pos[1] - O[1], mp.pos[2] - O[2]};
    const float dist = norm3(pc);
    auto it = mp.obs.find(mp.ref);
    const int level = ref.octave[it == mp.obs.end() ? 0 : it->second];
    const int nlevels = (int)w.scales.size();
    mp.min_dist = (1.0f / w.scale_factor) * dist / w.scales[level];
    mp.max_dist = w.scale_factor * dist * w.scales[nlevels - 1 - level];
    const float fn = (float)(1.0 / (double)n);
    for (int c = 0; c < 3; c++) mp.normal[c] = normal[c] * fn;
}

// Optimizer.cc:1517-1675
void build_graph(World& w, int cur, int ncov, const int32_t* cov) {
    const long stamp = w.kf[cur].id;
    const int nmp = (int)w.mp.size();
    // the stamps of an earlier call with the same keyframe would hide everything
    for (auto& K : w.kf) K.local_for = K.fixed_for = -1;
    for (auto& P : w.mp) P.local_for = -1;
    std::list<int> lLocalKeyFrames, lLocalMapPoints, lFixedCameras;
    lLocalKeyFrames.push_back(cur);  // :1520-1521
    w.kf[cur].local_for = stamp;
    for (int i = 0; i < ncov; i++) {  // :1523-1530
        KeyFrame& K = w.kf[cov[i]];
        K.local_for = stamp;
        if (!K.bad) lLocalKeyFrames.push_back(cov[i]);
    }
    for (int k : lLocalKeyFrames)  // :1534-1548
        for (int p : w.kf[k].slots) {
            if (p < 0 || p >= nmp) continue;  // NULL; an id past the map is no point
            MapPoint& P = w.mp[p];
            if (P.bad || P.local_for == stamp) continue;
            lLocalMapPoints.push_back(p);
            P.local_for = stamp;
        }
    for (int p : lLocalMapPoints)  // :1552-1566
        for (auto& o : w.mp[p].obs) {
            KeyFrame& K = w.kf[o.first];
            if (K.local_for != stamp && K.fixed_for != stamp) {
                K.fixed_for = stamp;
                if (!K.bad) lFixedCameras.push_back(o.first);
            }
        }
    w.local_kfs.assign(lLocalKeyFrames.begin(), lLocalKeyFrames.end());
    w.fixed_kfs.assign(lFixedCameras.begin(), lFixedCameras.end());
    w.local_pts.assign(lLocalMapPoints.begin(), lLocalMapPoints.end());
    // vertices in id order (:1584-1608, :1627-1635): g2o keeps them by id, gf_ba_problem wants that order
    std::map<int, int> kind;  // keyframe -> 0 local, 1 local and fixed (mnId == 0), 2 fixed camera
    for (int k : lLocalKeyFrames) kind[k] = w.kf[k].id == 0 ? 1 : 0;
    for (int k : lFixedCameras) kind[k] = 2;
    std::map<int, int> kf_index, pt_index;
    w.prob_kf.clear(), w.kf_kind.clear(), w.kf_Tcw.clear(), w.kf_cam.clear();
    for (auto& e : kind) {
        kf_index[e.first] = (int)w.prob_kf.size();
        w.prob_kf.push_back(e.first);
        w.kf_kind.push_back(e.second);
        w.kf_Tcw.insert(w.kf_Tcw.end(), w.kf[e.first].T, w.kf[e.first].T + 16);
        w.kf_cam.insert(w.kf_cam.end(), w.cam, w.cam + 4);
    }
    std::set<int> pts(lLocalMapPoints.begin(), lLocalMapPoints.end());
    w.prob_pt.clear(), w.pt_pos.clear();
    for (int p : pts) {
        pt_index[p] = (int)w.prob_pt.size();
        w.prob_pt.push_back(p);
        w.pt_pos.insert(w.pt_pos.end(), w.mp[p].pos, w.mp[p].pos + 3);
    }
    // edges in insertion order (:1627-1674)
    w.edge_pt.clear(), w.edge_kf.clear(), w.edge_gkp.clear(), w.edge_z.clear(), w.edge_inv_sigma2.clear();
    w.edge_map_pt.clear(), w.edge_map_kf.clear();
    for (int p : lLocalMapPoints)
        for (auto& o : w.mp[p].obs) {
            const KeyFrame& K = w.kf[o.first];
            if (K.bad) continue;  // :1644
            w.edge_pt.push_back(pt_index[p]);
            w.edge_kf.push_back(kf_index[o.first]);
            w.edge_gkp.push_back(K.off + o.second);
            w.edge_z.push_back(K.xy[2 * o.second]);
            w.edge_z.push_back(K.xy[2 * o.second + 1]);
            w.edge_inv_sigma2.push_back(w.inv_sigma2[K.octave[o.second]]);
            w.edge_map_pt.push_back(p);
            w.edge_map_kf.push_back(o.first);
        }
}

// Optimizer.cc:1681-1763 from a given result
void apply(World& w, const uint8_t* flags, const float* kf_Tcw, const float* pt_pos) {
    w.erased1.clear(), w.erased2.clear(), w.points_bad.clear(), w.bad_round2.clear(), w.stale.clear();
    const size_t ne = w.edge_pt.size();
    for (size_t i = 0; i < ne; i++) {  // :1681-1698
        const int p = w.edge_map_pt[i], k = w.edge_map_kf[i];
        if (w.mp[p].bad) {
            if (flags[i] == 1) w.stale.push_back((int)i);  // stays in optimize(10) in the reference
            continue;
        }
        if (flags[i] == 1) {
            erase_map_point_match(w, k, p);
            erase_observation(w, p, k);
            w.erased1.push_back((int)i);
        }
    }
    for (size_t i = 0; i < ne; i++) {  // :1725-1743
        if (flags[i] == 1) continue;  // vpEdges[i] == NULL, or a stale outlier of a bad point
        const int p = w.edge_map_pt[i], k = w.edge_map_kf[i];
        if (w.mp[p].bad) continue;
        if (flags[i] == 2) {
            erase_map_point_match(w, k, p);
            if (erase_observation(w, p, k)) w.bad_round2.push_back(p);
            w.erased2.push_back((int)i);
        }
    }
    for (size_t q = 0; q < w.prob_kf.size(); q++)  // :1748-1754
        if (w.kf_kind[q] != 2) std::copy(kf_Tcw + 16 * q, kf_Tcw + 16 * q + 16, w.kf[w.prob_kf[q]].T);
    for (size_t q = 0; q < w.prob_pt.size(); q++)  // SetWorldPos (:1761) has no bad test
        std::copy(pt_pos + 3 * q, pt_pos + 3 * q + 3, w.mp[w.prob_pt[q]].pos);
    for (int p : w.local_pts) update_normal_and_depth(w, p);  // :1762
}

template <typename T, typename U>
int give(const std::vector<T>& v, U* out) {
    if (out) std::copy(v.begin(), v.end(), out);
    return (int)v.size();
}

}  // namespace

extern "C" {

void* lr_create(int nkf, const int32_t* kf_off, const int32_t* octave, const int32_t* slots, const float* kp_xy,
                const uint8_t* kf_bad, const int32_t* kf_id, const float* kf_Tcw, int nmp, const uint8_t* mp_bad,
                const int32_t* ref_kf, const float* mp_pos, const float* mp_normal, const float* mp_min,
                const float* mp_max, int nobs, const int32_t* obs_p, const int32_t* obs_kf, const int32_t* obs_idx,
                const float* cam, int nlevels, const float* inv_sigma2, const float* scales, float scale_factor) {
    World* w = new World;
    w->kf.resize(nkf);
    w->mp.resize(nmp);
    for (int k = 0; k < nkf; k++) {
        KeyFrame& K = w->kf[k];
        K.id = kf_id[k], K.off = kf_off[k], K.bad = kf_bad[k];
        K.octave.assign(octave + kf_off[k], octave + kf_off[k + 1]);
        K.slots.assign(slots + kf_off[k], slots + kf_off[k + 1]);
        K.xy.assign(kp_xy + 2 * (size_t)kf_off[k], kp_xy + 2 * (size_t)kf_off[k + 1]);
        std::copy(kf_Tcw + 16 * k, kf_Tcw + 16 * k + 16, K.T);
    }
    for (int p = 0; p < nmp; p++) {
        MapPoint& P = w->mp[p];
        P.bad = mp_bad[p], P.ref = ref_kf[p], P.min_dist = mp_min[p], P.max_dist = mp_max[p];
        for (int c = 0; c < 3; c++) P.pos[c] = mp_pos[3 * p + c], P.normal[c] = mp_normal[3 * p + c];
    }
    for (int o = 0; o < nobs; o++) w->mp[obs_p[o]].obs[obs_kf[o]] = obs_idx[o];
    std::copy(cam, cam + 4, w->cam);
    w->inv_sigma2.assign(inv_sigma2, inv_sigma2 + nlevels);
    w->scales.assign(scales, scales + nlevels);
    w->scale_factor = scale_factor;
    return w;
}

void lr_destroy(void* h) { delete (World*)h; }

// cov: GetVectorCovisibleKeyFrames() of cur as it stands, the bad ones included
void lr_graph(void* h, int cur, int ncov, const int32_t* cov) { build_graph(*(World*)h, cur, ncov, cov); }

void lr_apply(void* h, const uint8_t* flags, const float* kf_Tcw, const float* pt_pos) {
    apply(*(World*)h, flags, kf_Tcw, pt_pos);
}

int lr_get(void* h, int field, int32_t* out) {
    World& w = *(World*)h;
    std::vector<int> v;
    const int nmp = (int)w.mp.size();
    switch (field) {
    case 0: return give(w.prob_kf, out);
    case 1: return give(w.kf_kind, out);
    case 2: return give(w.prob_pt, out);
    case 3: return give(w.edge_pt, out);
    case 4: return give(w.edge_kf, out);
    case 5: return give(w.edge_gkp, out);
    case 6: return give(w.local_kfs, out);
    case 7: return give(w.fixed_kfs, out);
    case 8: return give(w.local_pts, out);
    case 9: for (int p = 0; p < nmp; p++) v.push_back(w.mp[p].bad); break;
    case 10: for (auto& K : w.kf) v.insert(v.end(), K.slots.begin(), K.slots.end()); break;
    case 11:
        for (int p = 0; p < nmp; p++)
            for (auto& e : w.mp[p].obs) v.push_back(p), v.push_back(e.first), v.push_back(e.second);
        break;
    case 12: for (int p = 0; p < nmp; p++) v.push_back(w.mp[p].ref); break;
    case 13: return give(w.erased1, out);
    case 14: return give(w.erased2, out);
    case 15: return give(w.points_bad, out);
    case 16: return give(w.bad_round2, out);
    case 17: return give(w.stale, out);
    default: return -1;
    }
    return give(v, out);
}

int lr_getf(void* h, int field, float* out) {
    World& w = *(World*)h;
    std::vector<float> v;
    switch (field) {
    case 0: return give(w.kf_Tcw, out);
    case 1: return give(w.kf_cam, out);
    case 2: return give(w.pt_pos, out);
    case 3: return give(w.edge_z, out);
    case 4: return give(w.edge_inv_sigma2, out);
    case 5: for (auto& K : w.kf) v.insert(v.end(), K.T, K.T + 16); break;
    case 6: for (auto& P : w.mp) v.insert(v.end(), P.pos, P.pos + 3); break;
    case 7: for (auto& P : w.mp) v.insert(v.end(), P.normal, P.normal + 3); break;
    case 8: for (auto& P : w.mp) v.push_back(P.min_dist); break;
    case 9: for (auto& P : w.mp) v.push_back(P.max_dist); break;
    default: return -1;
    }
    return give(v, out);
}

}  // extern "C"
