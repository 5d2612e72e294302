// The tests' serial restatement of LocalMapping::KeyFrameCulling
// (src/LocalMapping.cc:562-616), KeyFrame::SetBadFlag (src/KeyFrame.cc:497-588),
// EraseConnection (:596-610), UpdateBestCovisibles (:141-160), ChangeParent
// (:436-441), SetNotErase / SetErase (:474-494), MapPoint::EraseObservation
// (src/MapPoint.cc:83-103) and MapPoint::SetBadFlag (:117-131).
//
// Written from the reference's behaviour with std::map / std::set keyed by
// keyframe index (docs/ORACLE_ASSUMPTIONS.md A26, A30); it shares no code with
// gf_orb_slam_amd/loopmap.py, localmapping.py or csrc/kfcull.hip. mspChildrens
// is kept as a set of its own here, where the LoopMap derives it.
#include <algorithm>
#include <cstdint>
#include <map>
#include <set>
#include <utility>
#include <vector>

namespace {

struct KeyFrame {
    int id = 0;
    std::vector<int> octave, slots;
    bool bad = false, not_erase = false, to_be_erased = false;
    std::map<int, int> weights;
    std::vector<int> ordered, ordered_w;
    int parent = -1;
    std::set<int> children, loop_edges;
};

struct MapPoint {
    bool bad = false;
    std::map<int, int> obs;  // keyframe -> slot
    int ref = -1;
};

struct World {
    std::vector<KeyFrame> kf;
    std::vector<MapPoint> mp;
    // what the last calls did, in order
    std::vector<int> cand, nmps, nred, culled_at, deferred_at, flags, culled, points_bad, reparented;
};

// KeyFrame.cc:141-160: (weight, keyframe) pairs sorted, then pushed to the front
void update_best_covisibles(World& w, int k) {
    KeyFrame& K = w.kf[k];
    std::vector<std::pair<int, int>> pairs;
    for (auto& e : K.weights) pairs.push_back({e.second, e.first});
    std::sort(pairs.begin(), pairs.end());
    K.ordered.clear();
    K.ordered_w.clear();
    for (auto it = pairs.rbegin(); it != pairs.rend(); ++it) {
        K.ordered.push_back(it->second);
        K.ordered_w.push_back(it->first);
    }
}

// KeyFrame.cc:596-610
void erase_connection(World& w, int k, int other) {
    if (w.kf[k].weights.erase(other)) update_best_covisibles(w, k);
}

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
void erase_observation(World& w, int p, int k) {
    MapPoint& P = w.mp[p];
    bool bad = false;
    if (P.obs.count(k)) {
        P.obs.erase(k);
        if (P.ref == k && !P.obs.empty()) P.ref = P.obs.begin()->first;
        if (P.obs.size() <= 2) bad = true;
    }
    if (bad) set_bad_point(w, p);
}

void change_parent(World& w, int c, int parent) {  // KeyFrame.cc:436-441
    w.kf[c].parent = parent;
    if (parent >= 0) w.kf[parent].children.insert(c);
    w.reparented.push_back(c);
    w.reparented.push_back(parent);
}

// KeyFrame.cc:497-588 -> 1 erased, 2 deferred, 0 returned
int set_bad_keyframe(World& w, int k) {
    KeyFrame& K = w.kf[k];
    if (K.id == 0) return 0;
    if (K.not_erase) {
        K.to_be_erased = true;
        return 2;
    }
    for (auto& e : K.weights) erase_connection(w, e.first, k);  // :510-511
    for (size_t i = 0; i < K.slots.size(); i++)                  // :513-515
        if (K.slots[i] >= 0) erase_observation(w, K.slots[i], k);
    K.weights.clear();
    K.ordered.clear();
    K.ordered_w.clear();
    std::set<int> candidates;  // :524-525
    if (K.parent >= 0) candidates.insert(K.parent);
    while (!K.children.empty()) {  // :529-572
        bool found = false;
        int max = -1, pc = -1, pp = -1;
        for (int c : K.children) {
            if (w.kf[c].bad) continue;
            const std::vector<int>& connected = w.kf[c].ordered;
            for (size_t i = 0; i < connected.size(); i++)
                for (int s : candidates)
                    if (w.kf[connected[i]].id == w.kf[s].id) {
                        auto it = w.kf[c].weights.find(connected[i]);  // GetWeight
                        const int wt = it == w.kf[c].weights.end() ? 0 : it->second;
                        if (wt > max) {
                            pc = c;
                            pp = connected[i];
                            max = wt;
                            found = true;
                        }
                    }
        }
        if (!found) break;
        change_parent(w, pc, pp);
        candidates.insert(pc);
        K.children.erase(pc);
    }
    for (int c : K.children) change_parent(w, c, K.parent);  // :575-579
    K.children.clear();  // the set dies with the keyframe; nothing reads it again
    if (K.parent >= 0) w.kf[K.parent].children.erase(k);  // :581
    K.bad = true;
    return 1;
}

int set_erase(World& w, int k) {  // KeyFrame.cc:480-494
    KeyFrame& K = w.kf[k];
    if (K.loop_edges.empty()) K.not_erase = false;
    if (K.to_be_erased) return set_bad_keyframe(w, k);
    return 0;
}

// LocalMapping.cc:576-611 of one keyframe on the world as it stands
void count_keyframe(World& w, int k, int& nmps, int& nred, std::vector<int>& flags) {
    const KeyFrame& K = w.kf[k];
    nmps = nred = 0;
    flags.assign(K.slots.size(), 0);
    for (size_t i = 0; i < K.slots.size(); i++) {
        const int p = K.slots[i];
        if (p < 0) continue;
        const MapPoint& P = w.mp[p];
        if (P.bad) continue;
        nmps++;
        flags[i] = 1;
        if (P.obs.size() > 3) {
            const int level = K.octave[i];
            int nobs = 0;
            for (auto& e : P.obs) {
                if (e.first == k) continue;
                if (w.kf[e.first].octave[e.second] <= level + 1) {
                    nobs++;
                    if (nobs >= 3) break;
                }
            }
            if (nobs >= 3) {
                nred++;
                flags[i] = 2;
            }
        }
    }
}

// LocalMapping.cc:562-616
void keyframe_culling(World& w, int cur) {
    w.cand.clear(), w.nmps.clear(), w.nred.clear(), w.culled_at.clear(), w.deferred_at.clear(), w.flags.clear();
    w.culled.clear(), w.points_bad.clear(), w.reparented.clear();
    const std::vector<int> local = w.kf[cur].ordered;  // :567, a copy
    for (int k : local) {
        if (w.kf[k].id == 0) continue;
        int nmps, nred;
        std::vector<int> flags;
        count_keyframe(w, k, nmps, nred, flags);
        w.cand.push_back(k), w.nmps.push_back(nmps), w.nred.push_back(nred);
        w.flags.insert(w.flags.end(), flags.begin(), flags.end());
        int what = 0;
        if (nred > 0.9 * nmps) what = set_bad_keyframe(w, k);  // :613, double
        w.culled_at.push_back(what == 1), w.deferred_at.push_back(what == 2);
        if (what == 1) w.culled.push_back(k);
    }
}

int give(const std::vector<int>& v, int32_t* out) {
    if (out) std::copy(v.begin(), v.end(), out);
    return (int)v.size();
}

}  // namespace

extern "C" {

// weights / ordered as CSR over the keyframes; loop_edges as a count per keyframe (only emptiness is read)
void* kr_create(int nkf, const int32_t* kf_off, const int32_t* octave, const int32_t* slots, const uint8_t* kf_bad,
                const int32_t* kf_id, int nmp, const uint8_t* mp_bad, const int32_t* ref_kf, int nobs,
                const int32_t* obs_p, const int32_t* obs_kf, const int32_t* obs_idx, const int32_t* parent,
                const int32_t* w_off, const int32_t* w_kf, const int32_t* w_w, const int32_t* o_off,
                const int32_t* o_kf, const int32_t* o_w, const int32_t* le_off, const int32_t* le_kf,
                const uint8_t* not_erase, const uint8_t* to_be_erased) {
    World* w = new World;
    w->kf.resize(nkf);
    w->mp.resize(nmp);
    for (int k = 0; k < nkf; k++) {
        KeyFrame& K = w->kf[k];
        K.id = kf_id[k];
        K.octave.assign(octave + kf_off[k], octave + kf_off[k + 1]);
        K.slots.assign(slots + kf_off[k], slots + kf_off[k + 1]);
        K.bad = kf_bad[k], K.not_erase = not_erase[k], K.to_be_erased = to_be_erased[k];
        K.parent = parent[k];
        for (int j = w_off[k]; j < w_off[k + 1]; j++) K.weights[w_kf[j]] = w_w[j];
        for (int j = o_off[k]; j < o_off[k + 1]; j++) K.ordered.push_back(o_kf[j]), K.ordered_w.push_back(o_w[j]);
        for (int j = le_off[k]; j < le_off[k + 1]; j++) K.loop_edges.insert(le_kf[j]);
    }
    for (int k = 0; k < nkf; k++)  // AddChild at the first connection; EraseChild by a keyframe that turned bad
        if (w->kf[k].parent >= 0 && !w->kf[k].bad) w->kf[w->kf[k].parent].children.insert(k);
    for (int p = 0; p < nmp; p++) w->mp[p].bad = mp_bad[p], w->mp[p].ref = ref_kf[p];
    for (int o = 0; o < nobs; o++) w->mp[obs_p[o]].obs[obs_kf[o]] = obs_idx[o];
    return w;
}

void kr_destroy(void* h) { delete (World*)h; }

void kr_clear_log(void* h) {
    World& w = *(World*)h;
    w.points_bad.clear(), w.reparented.clear(), w.culled.clear();
}

int kr_set_bad_keyframe(void* h, int k) { return set_bad_keyframe(*(World*)h, k); }
void kr_erase_observation(void* h, int p, int k) { erase_observation(*(World*)h, p, k); }
void kr_set_not_erase(void* h, int k) { ((World*)h)->kf[k].not_erase = true; }
int kr_set_erase(void* h, int k) { return set_erase(*(World*)h, k); }
void kr_keyframe_culling(void* h, int cur) { keyframe_culling(*(World*)h, cur); }

// the counts of one keyframe on the world as it stands -> flags into out_flags (its slot count)
void kr_count(void* h, int k, int32_t* out2, int32_t* out_flags) {
    std::vector<int> flags;
    count_keyframe(*(World*)h, k, out2[0], out2[1], flags);
    give(flags, out_flags);
}

int kr_get(void* h, int field, int32_t* out) {
    World& w = *(World*)h;
    std::vector<int> v;
    const int nkf = (int)w.kf.size(), nmp = (int)w.mp.size();
    switch (field) {
    case 0: for (int k = 0; k < nkf; k++) v.push_back(w.kf[k].bad); break;
    case 1: for (int p = 0; p < nmp; p++) v.push_back(w.mp[p].bad); break;
    case 2: for (auto& K : w.kf) v.insert(v.end(), K.slots.begin(), K.slots.end()); break;
    case 3:
        for (int p = 0; p < nmp; p++)
            for (auto& e : w.mp[p].obs) v.push_back(p), v.push_back(e.first), v.push_back(e.second);
        break;
    case 4: for (int p = 0; p < nmp; p++) v.push_back(w.mp[p].ref); break;
    case 5: for (int k = 0; k < nkf; k++) v.push_back(w.kf[k].parent); break;
    case 6:
        for (int k = 0; k < nkf; k++)
            for (auto& e : w.kf[k].weights) v.push_back(k), v.push_back(e.first), v.push_back(e.second);
        break;
    case 7:
        for (int k = 0; k < nkf; k++)
            for (size_t j = 0; j < w.kf[k].ordered.size(); j++)
                v.push_back(k), v.push_back(w.kf[k].ordered[j]), v.push_back(w.kf[k].ordered_w[j]);
        break;
    case 8: for (int k = 0; k < nkf; k++) v.push_back(w.kf[k].to_be_erased); break;
    case 9: for (int k = 0; k < nkf; k++) v.push_back(w.kf[k].not_erase); break;
    case 10: v = w.cand; break;
    case 11: v = w.nmps; break;
    case 12: v = w.nred; break;
    case 13: v = w.culled_at; break;
    case 14: v = w.deferred_at; break;
    case 15: v = w.culled; break;
    case 16: v = w.points_bad; break;
    case 17: v = w.reparented; break;
    case 18: v = w.flags; break;
    case 19:
        for (int k = 0; k < nkf; k++)
            for (int c : w.kf[k].children) v.push_back(k), v.push_back(c);
        break;
    default: return -1;
    }
    return give(v, out);
}

// The counting alone over the flat tables gf_keyframe_culling_counts takes
// (include/gfslam/abi.h), one candidate after the other, one slot after the
// other, with the reference's early exit at three.
void kr_counts_arrays(int nkf, const int32_t* kf_off, const uint8_t* octave, const int32_t* slots, int nmp,
                      const uint8_t* mp_bad, const int32_t* obs_off, const int32_t* obs_gkp, int ncand,
                      const int32_t* cand, int32_t* counts, uint8_t* flags) {
    for (int c = 0; c < ncand; c++) {
        const int k = cand[c], first = kf_off[k], last = kf_off[k + 1];
        int nmps = 0, nred = 0;
        for (int i = first; i < last; i++) {
            const int p = slots[i];
            uint8_t flag = 0;
            if (p >= 0 && p < nmp && !mp_bad[p]) {
                nmps++;
                flag = 1;
                int live = 0;
                for (int r = obs_off[p]; r < obs_off[p + 1]; r++) live += obs_gkp[r] >= 0;
                if (live > 3) {
                    int nobs = 0;
                    for (int r = obs_off[p]; r < obs_off[p + 1]; r++) {
                        const int g = obs_gkp[r];
                        if (g < 0 || (g >= first && g < last)) continue;
                        if ((int)octave[g] <= (int)octave[i] + 1 && ++nobs >= 3) break;
                    }
                    if (nobs >= 3) {
                        nred++;
                        flag = 2;
                    }
                }
            }
            if (flags) flags[i] = flag;
        }
        counts[2 * c] = nmps;
        counts[2 * c + 1] = nred;
    }
}

}  // extern "C"
