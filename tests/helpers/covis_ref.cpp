// The tests' serial restatement of KeyFrame::UpdateConnections
// (src/KeyFrame.cc:332-421), AddConnection (:126-139), UpdateBestCovisibles
// (:141-160) and the index state of LocalMapping::ProcessNewKeyFrame
// (src/LocalMapping.cc:163-211): which observations are added, what enters
// mlpRecentAddedMapPoints, the covisibility graph and the parent.
//
// Written from the reference's behaviour with std::map keyed by keyframe index
// (docs/ORACLE_ASSUMPTIONS.md A26); it shares no code with
// gf_orb_slam_amd/loopmap.py, localmapping.py or csrc/covis.hip. Descriptors,
// normals and depths are not restated here (the tests compare them with the
// map's per-point host methods).
#include <algorithm>
#include <cstdint>
#include <map>
#include <utility>
#include <vector>

namespace {

struct KeyFrame {
    int id = 0;  // mnId
    std::vector<int> slots;
    std::map<int, int> weights;
    std::vector<int> ordered, ordered_w;
    int parent = -1;
    bool first_connection = true;
    int bow_computed = 0;  // how many times ComputeBoW did its work
    bool has_bow = false;
};

struct MapPoint {
    bool bad = false;
    std::map<int, int> obs;  // keyframe -> slot
};

struct World {
    std::vector<KeyFrame> kf;
    std::vector<MapPoint> mp;
    std::vector<int> recent, associated;
};

// KeyFrame.cc:141-160: (weight, keyframe) pairs sorted, then pushed to the front
void update_best_covisibles(KeyFrame& K) {
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

// KeyFrame.cc:126-139
void add_connection(World& w, int k, int other, int weight) {
    KeyFrame& K = w.kf[k];
    auto it = K.weights.find(other);
    if (it == K.weights.end()) K.weights[other] = weight;
    else if (it->second != weight) it->second = weight;
    else return;
    update_best_covisibles(K);
}

// KeyFrame.cc:365-403 from a filled KFcounter: the ordered (weight, keyframe) pairs, heaviest first. listed: the
// keyframes AddConnection is called on, in the reference's call order.
void order_counter(const std::map<int, int>& counter, std::vector<std::pair<int, int>>& pairs, std::vector<int>& listed) {
    pairs.clear();
    listed.clear();
    if (counter.empty()) return;
    int nmax = 0, kmax = -1;
    const int th = 15;
    for (auto& e : counter) {
        if (e.second > nmax) nmax = e.second, kmax = e.first;
        if (e.second >= th) pairs.push_back({e.second, e.first}), listed.push_back(e.first);
    }
    if (pairs.empty()) pairs.push_back({nmax, kmax}), listed.push_back(kmax);
    std::sort(pairs.begin(), pairs.end());
    std::reverse(pairs.begin(), pairs.end());  // push_front of every pair in turn
}

// KeyFrame.cc:332-421 on the world
void update_connections(World& w, int k) {
    KeyFrame& K = w.kf[k];
    std::map<int, int> counter;
    const std::vector<int> vpMP = K.slots;
    for (int p : vpMP) {
        if (p < 0) continue;
        if (w.mp[p].bad) continue;
        for (auto& o : w.mp[p].obs) {
            if (w.kf[o.first].id == K.id) continue;
            counter[o.first]++;
        }
    }
    if (counter.empty()) return;
    std::vector<std::pair<int, int>> pairs;
    std::vector<int> listed;
    order_counter(counter, pairs, listed);
    for (int o : listed) add_connection(w, o, k, counter[o]);
    K.weights = counter;
    K.ordered.clear();
    K.ordered_w.clear();
    for (auto& pr : pairs) K.ordered.push_back(pr.second), K.ordered_w.push_back(pr.first);
    if (K.first_connection && K.id != 0) {
        K.parent = K.ordered.front();
        K.first_connection = false;
    }
}

// LocalMapping.cc:163-211, the index state
void process_new_keyframe(World& w, int k) {
    KeyFrame& K = w.kf[k];
    w.associated.clear();
    if (!K.has_bow) K.has_bow = true, K.bow_computed++;  // KeyFrame.cc:56-65
    if (K.id == 0) return;
    const std::vector<int> matches = K.slots;
    if (K.id > 1) {
        for (size_t i = 0; i < matches.size(); i++) {
            const int p = matches[i];
            if (p < 0) continue;
            if (w.mp[p].bad) continue;
            w.mp[p].obs[k] = (int)i;  // AddObservation overwrites
            w.associated.push_back(p);
        }
    }
    if (K.id == 1)
        for (int p : matches)
            if (p >= 0) w.recent.push_back(p);
    update_connections(w, k);
}

int give(const std::vector<int>& v, int32_t* out) {
    if (out) std::copy(v.begin(), v.end(), out);
    return (int)v.size();
}

}  // namespace

extern "C" {

// The counting and ordering over raw flat tables (the signature of gf_update_connections without the context). A
// slot outside [0, nmp) is no point; an entry equal to -1 or outside [0, nkp) is no observation; the keyframe of an
// entry g is the one whose range [kf_off[k], kf_off[k + 1]) holds it.
void cr_counts(int nkf, const int32_t* kf_off, const int32_t* slots, int nmp, const uint8_t* mp_bad,
               const int32_t* obs_off, const int32_t* obs_gkp, int nq, const int32_t* query, int32_t* weights,
               int32_t* n_ordered, int32_t* ordered_kf, int32_t* ordered_w) {
    const int nkp = nkf > 0 ? kf_off[nkf] : 0;
    std::vector<int> owner(nkp > 0 ? nkp : 0);
    for (int k = 0; k < nkf; k++)
        for (int g = kf_off[k]; g < kf_off[k + 1]; g++) owner[g] = k;
    for (int i = 0; i < nq; i++) {
        int32_t* W = weights + (size_t)i * nkf;
        int32_t* OK = ordered_kf + (size_t)i * nkf;
        int32_t* OW = ordered_w + (size_t)i * nkf;
        for (int k = 0; k < nkf; k++) W[k] = 0, OK[k] = -1, OW[k] = 0;
        n_ordered[i] = 0;
        const int K = query[i];
        if (K < 0 || K >= nkf) continue;
        std::map<int, int> counter;
        for (int s = kf_off[K]; s < kf_off[K + 1]; s++) {
            const int p = slots[s];
            if (p < 0 || p >= nmp) continue;
            if (mp_bad[p]) continue;
            for (int r = obs_off[p]; r < obs_off[p + 1]; r++) {
                const int g = obs_gkp[r];
                if (g < 0 || g >= nkp) continue;
                if (owner[g] == K) continue;
                counter[owner[g]]++;
            }
        }
        std::vector<std::pair<int, int>> pairs;
        std::vector<int> listed;
        order_counter(counter, pairs, listed);
        for (auto& e : counter) W[e.first] = e.second;
        n_ordered[i] = (int)pairs.size();
        for (size_t j = 0; j < pairs.size(); j++) OK[j] = pairs[j].second, OW[j] = pairs[j].first;
    }
}

// a world: slot tables, mnIds, bad flags, observation maps and the graph (CSR rows per keyframe)
void* cr_create(int nkf, const int32_t* kf_off, const int32_t* slots, const int32_t* kf_id, const int32_t* parent,
                const uint8_t* first_connection, const uint8_t* has_bow, const int32_t* w_off, const int32_t* w_kf,
                const int32_t* w_w, const int32_t* o_off, const int32_t* o_kf, const int32_t* o_w, int nmp,
                const uint8_t* mp_bad, int nobs, const int32_t* obs_p, const int32_t* obs_k, const int32_t* obs_i) {
    World* w = new World;
    w->kf.resize(nkf);
    for (int k = 0; k < nkf; k++) {
        KeyFrame& K = w->kf[k];
        K.id = kf_id[k];
        K.slots.assign(slots + kf_off[k], slots + kf_off[k + 1]);
        K.parent = parent[k];
        K.first_connection = first_connection[k] != 0;
        K.has_bow = has_bow[k] != 0;
        for (int j = w_off[k]; j < w_off[k + 1]; j++) K.weights[w_kf[j]] = w_w[j];
        for (int j = o_off[k]; j < o_off[k + 1]; j++) K.ordered.push_back(o_kf[j]), K.ordered_w.push_back(o_w[j]);
    }
    w->mp.resize(nmp);
    for (int p = 0; p < nmp; p++) w->mp[p].bad = mp_bad[p] != 0;
    for (int j = 0; j < nobs; j++) w->mp[obs_p[j]].obs[obs_k[j]] = obs_i[j];
    return w;
}

void cr_destroy(void* h) { delete (World*)h; }

// ``new KeyFrame`` + what Map::AddKeyFrame means for the indices: a keyframe without connections or observations
int cr_add_keyframe(void* h, int n, const int32_t* slots, int kf_id) {
    World& w = *(World*)h;
    KeyFrame K;
    K.id = kf_id;
    K.slots.assign(slots, slots + n);
    w.kf.push_back(K);
    return (int)w.kf.size() - 1;
}

void cr_update_connections(void* h, int k) { update_connections(*(World*)h, k); }
void cr_process_new_keyframe(void* h, int k) { process_new_keyframe(*(World*)h, k); }
void cr_set_recent(void* h, int n, const int32_t* ids) { ((World*)h)->recent.assign(ids, ids + n); }

// field: 0 slots, 1 obs (point, keyframe, slot), 2 weights (keyframe, other, weight), 3 ordered (keyframe, other,
// weight), 4 parent, 5 first_connection, 6 recent, 7 associated, 8 bow_computed. out == null: the length only.
int cr_get(void* h, int field, int32_t* out) {
    World& w = *(World*)h;
    std::vector<int> v;
    switch (field) {
        case 0:
            for (auto& K : w.kf) v.insert(v.end(), K.slots.begin(), K.slots.end());
            break;
        case 1:
            for (size_t p = 0; p < w.mp.size(); p++)
                for (auto& o : w.mp[p].obs) v.insert(v.end(), {(int)p, o.first, o.second});
            break;
        case 2:
            for (size_t k = 0; k < w.kf.size(); k++)
                for (auto& e : w.kf[k].weights) v.insert(v.end(), {(int)k, e.first, e.second});
            break;
        case 3:
            for (size_t k = 0; k < w.kf.size(); k++)
                for (size_t j = 0; j < w.kf[k].ordered.size(); j++)
                    v.insert(v.end(), {(int)k, w.kf[k].ordered[j], w.kf[k].ordered_w[j]});
            break;
        case 4:
            for (auto& K : w.kf) v.push_back(K.parent);
            break;
        case 5:
            for (auto& K : w.kf) v.push_back(K.first_connection);
            break;
        case 6:
            v = w.recent;
            break;
        case 7:
            v = w.associated;
            break;
        case 8:
            for (auto& K : w.kf) v.push_back(K.bow_computed);
            break;
        default:
            return -1;
    }
    return give(v, out);
}

}  // extern "C"
