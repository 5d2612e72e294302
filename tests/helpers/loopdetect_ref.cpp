// Serial CPU model of loop detection for the tests, in this project's own
// layout: keyframes are indices, a BowVector is a pair of sorted arrays, the
// inverted file is one std::list<int> of keyframe indices per word, and the
// per-keyframe query state lives in plain arrays. It follows what the
// reference does, not how it is written:
//   file_add / file_erase   KeyFrameDatabase::add / erase (KeyFrameDatabase.cc:39-66)
//   l1_score                L1Scoring::score (ScoringObject.cpp:23-68)
//   query                   KeyFrameDatabase::DetectLoopCandidates (:75-196)
//   detect                  LoopClosing::DetectLoop (LoopClosing.cc:111-238)
// A keyframe's mnId is its index. The query mark starts at -1 (the reference's
// 0 is safe there only because keyframe 0 never queries).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <list>
#include <map>
#include <set>
#include <utility>
#include <vector>

namespace {

struct Bow {
    std::vector<int> word;    // ascending
    std::vector<double> val;
};

// Both vectors are walked once in word order; a word present in both adds
// |a - b| - |a| - |b| to the running sum, in that order. The reference jumps
// with lower_bound where this steps; the words met in common and their order
// are the same.
double l1_score(const Bow& a, const Bow& b) {
    double sum = 0.0;
    size_t i = 0, j = 0;
    while (i < a.word.size() && j < b.word.size()) {
        if (a.word[i] < b.word[j]) {
            i++;
        } else if (b.word[j] < a.word[i]) {
            j++;
        } else {
            sum += std::fabs(a.val[i] - b.val[j]) - std::fabs(a.val[i]) - std::fabs(b.val[j]);
            i++;
            j++;
        }
    }
    return -sum / 2.0;
}

// what a query went through (the tests' scene conditions)
struct Trace {
    int32_t sharing;        // keyframes reached through the file and not connected
    int32_t max_common;
    int32_t min_common;
    int32_t scored;
    int32_t passed;         // score >= floor
    int32_t at_min_score;   // of those, score == floor
    int32_t best_differs;   // entries whose best keyframe is a neighbour
    int32_t retained;       // entries above 0.75 * best accumulated score
    int32_t dropped;        // entries at or below it
    int32_t duplicates;     // retained entries whose best keyframe was already out
    int32_t at_min_common;  // reached keyframes with exactly min_common words
    int32_t just_above;     // ... min_common + 1
    int32_t neigh_summed;   // neighbours added to an accumulated score
    int32_t neigh_skipped;  // neighbours of the first ten not added
    int32_t eleventh;       // entries with more than ten ordered covisibles
    int32_t same_first_word;  // most keyframes first reached at one query word
};

struct Group {
    std::set<int> members;
    int count;
};

struct Ref {
    // keyframes, by index
    std::vector<Bow> bow;
    std::vector<std::vector<int> > ordered;   // mvpOrderedConnectedKeyFrames
    std::vector<std::set<int> > connected;    // keys of mConnectedKeyFrameWeights
    std::vector<char> bad;
    std::vector<long> mark;     // mnLoopQuery
    std::vector<int> common;    // mnLoopWords
    std::vector<float> kscore;  // mLoopScore
    // the inverted file
    std::map<int, std::list<int> > file;
    // DetectLoop's state
    long last_loop_id = 0;      // mLastLoopKFid
    int consistency_th = 3;     // mnCovisibilityConsistencyTh
    std::vector<Group> groups;  // mvConsistentGroups
    std::vector<int> enough;    // mvpEnoughConsistentCandidates

    int insert(const int32_t* w, const double* v, int n) {
        Bow b;
        b.word.assign(w, w + n);
        b.val.assign(v, v + n);
        bow.push_back(b);
        ordered.emplace_back();
        connected.emplace_back();
        bad.push_back(0);
        mark.push_back(-1);
        common.push_back(0);
        kscore.push_back(0.f);
        return (int)bow.size() - 1;
    }

    void file_add(int kf) {
        for (int w : bow[kf].word) file[w].push_back(kf);
    }

    void file_erase(int kf) {  // the first occurrence in each of its words' lists
        for (int w : bow[kf].word) {
            std::list<int>& l = file[w];
            std::list<int>::iterator at = std::find(l.begin(), l.end(), kf);
            if (at != l.end()) l.erase(at);
        }
    }

    std::vector<int> query(int q, float floor_score, Trace* out) {
        Trace t = Trace();
        std::vector<int> result;
        // 1. the file walk: query words ascending, each list front to back.
        // A keyframe met for the first time in this query restarts its count;
        // it joins `reached` unless it is connected to the query (a connected
        // one is never marked, so it restarts at every meeting).
        std::vector<int> reached;
        for (int w : bow[q].word) {
            std::map<int, std::list<int> >::iterator l = file.find(w);
            if (l == file.end()) continue;
            int fresh = 0;
            for (int kf : l->second) {
                if (mark[kf] != q) {
                    common[kf] = 0;
                    if (connected[q].count(kf) == 0) {
                        mark[kf] = q;
                        reached.push_back(kf);
                        fresh++;
                    }
                }
                common[kf]++;
            }
            t.same_first_word = std::max(t.same_first_word, fresh);
        }
        t.sharing = (int)reached.size();
        if (!reached.empty()) {
            // 2. the common-word threshold: 0.8 of the maximum in float, truncated
            int most = 0;
            for (int kf : reached) most = std::max(most, common[kf]);
            const int least = (int)(most * 0.8f);
            t.max_common = most;
            t.min_common = least;
            // 3. scores of the keyframes above it, kept when they reach the floor
            std::vector<int> kept;
            for (int kf : reached) {
                t.at_min_common += common[kf] == least;
                t.just_above += common[kf] == least + 1;
                if (common[kf] <= least) continue;
                t.scored++;
                kscore[kf] = (float)l1_score(bow[q], bow[kf]);
                if (kscore[kf] >= floor_score) {
                    kept.push_back(kf);
                    t.at_min_score += kscore[kf] == floor_score;
                }
            }
            t.passed = (int)kept.size();
            // 4. per kept keyframe: its score plus those of its first ten ordered
            // covisibles that this query scored, in float and in list order; the
            // best-scoring keyframe of the lot (a neighbour only when strictly better)
            std::vector<float> total(kept.size());
            std::vector<int> best(kept.size());
            float top = floor_score;
            for (size_t e = 0; e < kept.size(); e++) {
                const int kf = kept[e];
                const std::vector<int>& nb = ordered[kf];
                t.eleventh += nb.size() > 10;
                float acc = kscore[kf], hi = kscore[kf];
                int who = kf;
                for (size_t c = 0; c < nb.size() && c < 10; c++) {
                    const int k2 = nb[c];
                    if (mark[k2] != q || common[k2] <= least) {
                        t.neigh_skipped++;
                        continue;
                    }
                    t.neigh_summed++;
                    acc += kscore[k2];
                    if (kscore[k2] > hi) {
                        hi = kscore[k2];
                        who = k2;
                    }
                }
                t.best_differs += who != kf;
                total[e] = acc;
                best[e] = who;
                if (acc > top) top = acc;
            }
            // 5. entries above 0.75 of the top, in order, each best keyframe once
            const float bar = 0.75f * top;
            std::set<int> out_already;
            for (size_t e = 0; e < kept.size(); e++) {
                if (!(total[e] > bar)) {
                    t.dropped++;
                    continue;
                }
                t.retained++;
                if (out_already.insert(best[e]).second)
                    result.push_back(best[e]);
                else
                    t.duplicates++;
            }
        }
        if (out) *out = t;
        return result;
    }

    static bool overlap(const std::set<int>& a, const std::set<int>& b) {
        for (int x : a)
            if (b.count(x)) return true;
        return false;
    }

    // -> 0 early return, 1 no candidate, 2 no consistent candidate, 3 loop detected.
    // The keyframe enters the file on every path.
    int detect(int cur, float* floor_out) {
        if (cur < last_loop_id + 10) {
            file_add(cur);
            return 0;
        }
        // the floor: the lowest float score to a non-bad ordered covisible, from 1
        float floor_score = 1.f;
        for (int k : ordered[cur]) {
            if (bad[k]) continue;
            floor_score = std::min(floor_score, (float)l1_score(bow[cur], bow[k]));
        }
        if (floor_out) *floor_out = floor_score;
        const std::vector<int> cands = query(cur, floor_score, nullptr);
        if (cands.empty()) {
            groups.clear();
            file_add(cur);
            return 1;
        }
        // a candidate's group (itself and its connected keyframes) continues every
        // previous group it overlaps: that group's count + 1. A previous group is
        // continued by the first candidate that overlaps it only; a candidate is
        // reported once, at the first overlap whose new count reaches the
        // threshold; a candidate overlapping nothing starts a group at 0.
        enough.clear();
        std::vector<Group> next;
        std::vector<char> continued(groups.size(), 0);
        for (int c : cands) {
            Group g;
            g.members = connected[c];
            g.members.insert(c);
            bool reported = false, any = false;
            for (size_t p = 0; p < groups.size(); p++) {
                if (!overlap(g.members, groups[p].members)) continue;
                any = true;
                g.count = groups[p].count + 1;
                if (!continued[p]) {
                    next.push_back(g);
                    continued[p] = 1;
                }
                if (g.count >= consistency_th && !reported) {
                    enough.push_back(c);
                    reported = true;
                }
            }
            if (!any) {
                g.count = 0;
                next.push_back(g);
            }
        }
        groups.swap(next);
        file_add(cur);
        return enough.empty() ? 2 : 3;
    }
};

}  // namespace

extern "C" {

void* ld_create(int consistency_th) {
    Ref* r = new Ref();
    r->consistency_th = consistency_th;
    return r;
}
void ld_destroy(void* h) { delete (Ref*)h; }

int ld_insert(void* h, const int32_t* words, const double* values, int n) { return ((Ref*)h)->insert(words, values, n); }

void ld_set_graph(void* h, int kf, const int32_t* ordered, int nord, const int32_t* connected, int nconn) {
    Ref* r = (Ref*)h;
    r->ordered[kf].assign(ordered, ordered + nord);
    r->connected[kf] = std::set<int>(connected, connected + nconn);
}
void ld_set_bad(void* h, int kf, int bad) { ((Ref*)h)->bad[kf] = bad != 0; }
void ld_add(void* h, int kf) { ((Ref*)h)->file_add(kf); }
void ld_erase(void* h, int kf) { ((Ref*)h)->file_erase(kf); }
void ld_clear(void* h) { ((Ref*)h)->file.clear(); }

// the keyframes of a word's list, in list order
int ld_word_list(void* h, int word, int32_t* out, int cap) {
    Ref* r = (Ref*)h;
    std::map<int, std::list<int> >::iterator it = r->file.find(word);
    if (it == r->file.end()) return 0;
    int n = 0;
    for (int k : it->second) {
        if (n < cap) out[n] = k;
        n++;
    }
    return n;
}

double ld_score(void* h, int a, int b) { return l1_score(((Ref*)h)->bow[a], ((Ref*)h)->bow[b]); }

double ld_score_vectors(const int32_t* w1, const double* v1, int n1, const int32_t* w2, const double* v2, int n2) {
    Bow a, b;
    a.word.assign(w1, w1 + n1);
    a.val.assign(v1, v1 + n1);
    b.word.assign(w2, w2 + n2);
    b.val.assign(v2, v2 + n2);
    return l1_score(a, b);
}

// words_out / score_out per keyframe: the common-word count where this query
// reached the keyframe (else 0), the score where it was scored (else 0)
int ld_detect_candidates(void* h, int kf, float min_score, int32_t* words_out, float* score_out, int32_t* cands,
                         Trace* trace) {
    Ref* r = (Ref*)h;
    Trace t;
    const std::vector<int> c = r->query(kf, min_score, &t);
    for (size_t i = 0; i < r->bow.size(); i++) {
        const bool reached = r->mark[i] == kf;
        words_out[i] = reached ? r->common[i] : 0;
        score_out[i] = reached && r->common[i] > t.min_common ? r->kscore[i] : 0.f;
    }
    std::copy(c.begin(), c.end(), cands);
    if (trace) *trace = t;
    // the tests query the same keyframe more than once: a later query must not find this one's marks
    std::fill(r->mark.begin(), r->mark.end(), -1L);
    return (int)c.size();
}

void ld_set_last_loop(void* h, long id) { ((Ref*)h)->last_loop_id = id; }

int ld_detect_loop(void* h, int kf, float* min_score, int32_t* enough, int32_t* nenough) {
    Ref* r = (Ref*)h;
    const int path = r->detect(kf, min_score);
    *nenough = 0;
    if (path >= 2) {
        std::copy(r->enough.begin(), r->enough.end(), enough);
        *nenough = (int32_t)r->enough.size();
    }
    return path;
}

// the consistent groups: counters[g], sizes[g], members (ascending) back to back; -> number of groups
int ld_groups(void* h, int32_t* counters, int32_t* sizes, int32_t* members, int cap_groups, int cap_members) {
    Ref* r = (Ref*)h;
    int m = 0, g = 0;
    for (const Group& grp : r->groups) {
        if (g >= cap_groups || m + (int)grp.members.size() > cap_members) return -1;
        counters[g] = grp.count;
        sizes[g] = (int32_t)grp.members.size();
        for (int id : grp.members) members[m++] = id;
        g++;
    }
    return g;
}

}  // extern "C"
