// Serial CPU restatement of gf_frontend_compact_maps for one stream, on flat
// arrays laid out as the front end's slabs: the verdict of a request, the pins,
// the stable remap tables and the restriction of every row, CSR and index
// holder, one item after the other (tests/test_mapcompact_cpu.py,
// tests/test_mapcompact_gpu.py). Rows past the new counts keep their bytes, as
// an in-place ascending move leaves them.
#include <cstdint>
#include <cstring>
#include <vector>

namespace {

enum { OK = 0, ERR_ARG = -1, ERR_UNSUPPORTED = -4 };

struct Request {
    int32_t n_drop_kf;
    const int32_t* drop_kf;
    int32_t n_drop_mp;
    const int32_t* drop_mp;
};

// The arrays of one stream. point_rows / kf_rows: slabs whose row i belongs to
// point / keyframe i, with their row sizes in bytes.
struct Stream {
    int32_t M, KC, slot_cap, cap;
    int32_t* counts;  // nmp, nkf
    int32_t n_point_rows;
    uint8_t* const* point_rows;
    const int32_t* point_row_bytes;
    int32_t n_kf_rows;
    uint8_t* const* kf_rows;
    const int32_t* kf_row_bytes;
    int32_t *kf_mp_off, *kf_mp, *kf_cov_off, *kf_cov, *mp_obs_off, *mp_obs;
    // index holders
    int32_t* kp2mp;
    int32_t nkp;
    int32_t* last_kp2mp;
    int32_t last_nkp;
    int32_t* left;
    int32_t nleft;
    int32_t* out_slots;  // the outbox keyframe's slots, read when pending
    int32_t out_n, pending;
    int32_t* ref_kf;     // the persistent reference-keyframe word
    int32_t* state_ref;  // GF_KF_REF of the keyframe stage, or null
};

int check(int nmp, int nkf, int has_db, const Request& r) {
    if (r.n_drop_kf < 0 || r.n_drop_mp < 0) return ERR_ARG;
    std::vector<char> seen_kf(nkf > 0 ? nkf : 1, 0), seen_mp(nmp > 0 ? nmp : 1, 0);
    for (int i = 0; i < r.n_drop_kf; i++) {
        const int k = r.drop_kf[i];
        if (k < 0 || k >= nkf || seen_kf[k]) return ERR_ARG;
        seen_kf[k] = 1;
    }
    for (int i = 0; i < r.n_drop_mp; i++) {
        const int p = r.drop_mp[i];
        if (p < 0 || p >= nmp || seen_mp[p]) return ERR_ARG;
        seen_mp[p] = 1;
    }
    if (r.n_drop_kf && has_db) return ERR_UNSUPPORTED;
    return OK;
}

int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

void pin(const int32_t* held, int n, std::vector<int32_t>& keep) {
    for (int i = 0; i < n; i++)
        if (held[i] >= 0 && held[i] < (int)keep.size()) keep[held[i]] = 1;
}

void renumber(int32_t* a, int n, const int32_t* remap, int len) {
    for (int i = 0; i < n; i++)
        if (a[i] >= 0 && a[i] < len) a[i] = remap[a[i]];
}

}  // namespace

extern "C" {

int mc_check(int nmp, int nkf, int has_db, const Request* r) { return check(nmp, nkf, has_db, *r); }

// kept[2]: listed keyframes / points that were pinned. kf_remap [nkf], mp_remap [nmp] of the old counts.
int mc_apply(const Stream* S, int has_db, const Request* r, int32_t* kf_remap, int32_t* mp_remap, int32_t* kept) {
    const int n = S->counts[0], nk = S->counts[1];
    const int rc = check(n, nk, has_db, *r);
    if (rc) return rc;
    // mark: everything stays, the listed items go, what frame state holds stays after all
    std::vector<int32_t> keep_mp(n, 1), keep_kf(nk, 1);
    for (int i = 0; i < r->n_drop_mp; i++) keep_mp[r->drop_mp[i]] = 0;
    for (int i = 0; i < r->n_drop_kf; i++) keep_kf[r->drop_kf[i]] = 0;
    pin(S->kp2mp, clampi(S->nkp, 0, S->cap), keep_mp);
    pin(S->last_kp2mp, clampi(S->last_nkp, 0, S->cap), keep_mp);
    if (S->pending) pin(S->out_slots, clampi(S->out_n, 0, S->cap), keep_mp);
    if (*S->ref_kf >= 0 && *S->ref_kf < nk) keep_kf[*S->ref_kf] = 1;
    // scan: stable renumbering
    int n1 = 0, nk1 = 0;
    for (int p = 0; p < n; p++) mp_remap[p] = keep_mp[p] ? n1++ : -1;
    for (int k = 0; k < nk; k++) kf_remap[k] = keep_kf[k] ? nk1++ : -1;
    kept[0] = kept[1] = 0;
    for (int i = 0; i < r->n_drop_kf; i++) kept[0] += kf_remap[r->drop_kf[i]] >= 0;
    for (int i = 0; i < r->n_drop_mp; i++) kept[1] += mp_remap[r->drop_mp[i]] >= 0;
    // rows with their item
    for (int a = 0; a < S->n_point_rows; a++) {
        const size_t w = S->point_row_bytes[a];
        for (int p = 0; p < n; p++)
            if (mp_remap[p] >= 0 && mp_remap[p] != p) memmove(S->point_rows[a] + w * mp_remap[p], S->point_rows[a] + w * p, w);
    }
    for (int a = 0; a < S->n_kf_rows; a++) {
        const size_t w = S->kf_row_bytes[a];
        for (int k = 0; k < nk; k++)
            if (kf_remap[k] >= 0 && kf_remap[k] != k) memmove(S->kf_rows[a] + w * kf_remap[k], S->kf_rows[a] + w * k, w);
    }
    // KeyFrame::mvpMapPoints
    {
        std::vector<int32_t> off(1, 0), flat;
        for (int k = 0; k < nk; k++) {
            if (kf_remap[k] < 0) continue;
            for (int e = S->kf_mp_off[k]; e < S->kf_mp_off[k + 1]; e++) {
                const int v = S->kf_mp[e];
                flat.push_back(v >= 0 && v < n ? mp_remap[v] : -1);
            }
            off.push_back((int32_t)flat.size());
        }
        if (!flat.empty()) memcpy(S->kf_mp, flat.data(), 4 * flat.size());
        memcpy(S->kf_mp_off, off.data(), 4 * off.size());
    }
    // mvpOrderedConnectedKeyFrames
    {
        std::vector<int32_t> off(1, 0), flat;
        for (int k = 0; k < nk; k++) {
            if (kf_remap[k] < 0) continue;
            for (int e = S->kf_cov_off[k]; e < S->kf_cov_off[k + 1]; e++)
                if (kf_remap[S->kf_cov[e]] >= 0) flat.push_back(kf_remap[S->kf_cov[e]]);
            off.push_back((int32_t)flat.size());
        }
        if (!flat.empty()) memcpy(S->kf_cov, flat.data(), 4 * flat.size());
        memcpy(S->kf_cov_off, off.data(), 4 * off.size());
    }
    // MapPoint::mObservations
    {
        std::vector<int32_t> off(1, 0), flat;
        for (int p = 0; p < n; p++) {
            if (mp_remap[p] < 0) continue;
            for (int e = S->mp_obs_off[p]; e < S->mp_obs_off[p + 1]; e++)
                if (kf_remap[S->mp_obs[e]] >= 0) flat.push_back(kf_remap[S->mp_obs[e]]);
            off.push_back((int32_t)flat.size());
        }
        if (!flat.empty()) memcpy(S->mp_obs, flat.data(), 4 * flat.size());
        memcpy(S->mp_obs_off, off.data(), 4 * off.size());
    }
    // the index holders
    renumber(S->kp2mp, clampi(S->nkp, 0, S->cap), mp_remap, n);
    renumber(S->last_kp2mp, clampi(S->last_nkp, 0, S->cap), mp_remap, n);
    renumber(S->left, clampi(S->nleft, 0, S->M), mp_remap, n);
    if (S->pending) renumber(S->out_slots, clampi(S->out_n, 0, S->cap), mp_remap, n);
    renumber(S->ref_kf, 1, kf_remap, nk);
    if (S->state_ref) renumber(S->state_ref, 1, kf_remap, nk);
    S->counts[0] = n1;
    S->counts[1] = nk1;
    return OK;
}

}  // extern "C"
