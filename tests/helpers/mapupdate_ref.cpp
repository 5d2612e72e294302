// Serial CPU restatement of gf_frontend_update_maps for one stream
// (tests/mapupdate_ref.py): the validation verdict of a delta against the
// stream's state, and the delta applied to flat arrays laid out as the front
// end's per-stream slabs (capacities M points, KC keyframes, slot_cap slots
// and observations). One item after the other, no staging, no scan: the
// observation CSR is rebuilt row by row into a vector.
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/gfslam/abi.h"

namespace {
const int OK = 0, ARG = -1, CAP = -3, UNSUPPORTED = -4;
}

extern "C" {

// The verdict gf_frontend_update_maps gives the delta on a stream that holds
// nmp points and nkf keyframes with the given slot and observation offsets.
int mu_check(int M, int KC, int slot_cap, int has_db, int nmp, int nkf, const int32_t* kf_mp_off,
             const int32_t* mp_obs_off, const gf_map_delta* d) {
    if (d->n_new_mp < 0 || d->n_set_mp < 0 || d->n_bad_mp < 0 || d->n_new_kf < 0 || d->n_bad_kf < 0 || d->n_slot < 0 ||
        d->n_obs_rows < 0)
        return ARG;
    if ((long long)nmp + d->n_new_mp > M) return CAP;
    if ((long long)nkf + d->n_new_kf > KC) return CAP;
    const int nmp1 = nmp + d->n_new_mp, nkf1 = nkf + d->n_new_kf;
    if (d->n_new_kf && has_db) return UNSUPPORTED;
    std::vector<char> seen(std::max(nmp1, 1), 0);
    for (int i = 0; i < d->n_set_mp; i++) {
        const int p = d->set_mp_idx[i];
        if (p < 0 || p >= nmp || seen[p]) return ARG;
        seen[p] = 1;
    }
    if (d->n_bad_mp > M || d->n_bad_kf > KC) return ARG;
    for (int i = 0; i < d->n_bad_mp; i++)
        if (d->bad_mp[i] < 0 || d->bad_mp[i] >= nmp1) return ARG;
    for (int i = 0; i < d->n_bad_kf; i++)
        if (d->bad_kf[i] < 0 || d->bad_kf[i] >= nkf1) return ARG;
    const long long ns0 = nkf ? kf_mp_off[nkf] : 0;
    long long nnew = 0;
    if (d->n_new_kf) {
        if (d->new_kf_off[0] != 0) return ARG;
        for (int k = 0; k < d->n_new_kf; k++)
            if (d->new_kf_off[k] > d->new_kf_off[k + 1]) return ARG;
        nnew = d->new_kf_off[d->n_new_kf];
    }
    if (ns0 + nnew > slot_cap) return CAP;
    for (long long i = 0; i < nnew; i++)
        if (d->new_kf_mp[i] < -1 || d->new_kf_mp[i] >= nmp1) return ARG;
    std::vector<long long> where;
    for (int i = 0; i < d->n_slot; i++) {
        const int k = d->slot_kf[i], idx = d->slot_idx[i], v = d->slot_val[i];
        if (k < 0 || k >= nkf || idx < 0 || idx >= kf_mp_off[k + 1] - kf_mp_off[k]) return ARG;
        if (v < -1 || v >= nmp1) return ARG;
        where.push_back((long long)kf_mp_off[k] + idx);
    }
    std::sort(where.begin(), where.end());
    if (std::adjacent_find(where.begin(), where.end()) != where.end()) return ARG;
    long long no = nmp ? mp_obs_off[nmp] : 0;
    std::fill(seen.begin(), seen.end(), 0);
    if (d->n_obs_rows && d->obs_off[0] != 0) return ARG;
    for (int r = 0; r < d->n_obs_rows; r++) {
        const int p = d->obs_mp[r];
        if (p < 0 || p >= nmp1 || seen[p]) return ARG;
        seen[p] = 1;
        const int o0 = d->obs_off[r], o1 = d->obs_off[r + 1];
        if (o0 > o1) return ARG;
        for (int i = o0; i < o1; i++)
            if (d->obs_kf[i] < 0 || d->obs_kf[i] >= nkf1 || (i > o0 && d->obs_kf[i - 1] >= d->obs_kf[i])) return ARG;
        no += (o1 - o0) - (p < nmp ? mp_obs_off[p + 1] - mp_obs_off[p] : 0);
    }
    if (no > slot_cap) return CAP;
    if (d->has_cov) {
        if (d->kf_cov_off[0] != 0) return ARG;
        for (int k = 0; k < nkf1; k++)
            if (d->kf_cov_off[k] > d->kf_cov_off[k + 1]) return ARG;
        const long long nc = d->kf_cov_off[nkf1];
        if (nc > (long long)nkf1 * nkf1) return CAP;
        for (long long i = 0; i < nc; i++)
            if (d->kf_cov[i] < 0 || d->kf_cov[i] >= nkf1) return ARG;
    }
    return OK;
}

// The delta applied in place; a refused delta writes nothing. views: [M][5]
// words; counts[2] = nmp, nkf in and out.
int mu_apply(int M, int KC, int slot_cap, int cap, int has_db, int32_t* counts, gf_map_point* map, uint8_t* desc,
             float* pos, int32_t* upd, int32_t* views, uint8_t* mp_bad, uint8_t* kf_bad, int32_t* kf_mp_off,
             int32_t* kf_mp, int32_t* kf_cov_off, int32_t* kf_cov, int32_t* mp_obs_off, int32_t* mp_obs,
             const int32_t* last_kp2mp, int last_nkp, float* last_pos, const gf_map_delta* d) {
    const int nmp = counts[0], nkf = counts[1];
    const int rc = mu_check(M, KC, slot_cap, has_db, nmp, nkf, kf_mp_off, mp_obs_off, d);
    if (rc) return rc;
    const int nmp1 = nmp + d->n_new_mp, nkf1 = nkf + d->n_new_kf;
    // Map::AddMapPoint
    for (int i = 0; i < d->n_new_mp; i++) {
        const int p = nmp + i;
        map[p] = d->new_mp[i];
        memcpy(desc + 32 * (size_t)p, d->new_mp_desc + 32 * (size_t)i, 32);
        for (int c = 0; c < 3; c++) pos[3 * p + c] = d->new_mp[i].pos[c];
        mp_bad[p] = d->new_mp_bad ? d->new_mp_bad[i] : 0;
        upd[p] = -1000;
        for (int c = 0; c < 5; c++) views[5 * p + c] = 0;
    }
    // SetWorldPos, UpdateNormalAndDepth, ComputeDistinctiveDescriptors
    for (int i = 0; i < d->n_set_mp; i++) {
        const int p = d->set_mp_idx[i];
        map[p] = d->set_mp[i];
        memcpy(desc + 32 * (size_t)p, d->set_mp_desc + 32 * (size_t)i, 32);
        for (int c = 0; c < 3; c++) pos[3 * p + c] = d->set_mp[i].pos[c];
    }
    // Map::AddKeyFrame
    const int ns0 = nkf ? kf_mp_off[nkf] : 0, nc0 = nkf ? kf_cov_off[nkf] : 0;
    if (d->n_new_kf) {
        for (int k = 0; k <= d->n_new_kf; k++) kf_mp_off[nkf + k] = ns0 + d->new_kf_off[k];
        for (int i = 0; i < d->new_kf_off[d->n_new_kf]; i++) kf_mp[ns0 + i] = d->new_kf_mp[i];
        for (int k = 0; k < d->n_new_kf; k++) kf_bad[nkf + k] = d->new_kf_bad ? d->new_kf_bad[k] : 0;
        if (!d->has_cov)
            for (int k = 0; k <= d->n_new_kf; k++) kf_cov_off[nkf + k] = nc0;
    }
    // AddMapPoint / ReplaceMapPointMatch / EraseMapPointMatch
    for (int i = 0; i < d->n_slot; i++) kf_mp[kf_mp_off[d->slot_kf[i]] + d->slot_idx[i]] = d->slot_val[i];
    // mvpOrderedConnectedKeyFrames
    if (d->has_cov) {
        for (int k = 0; k <= nkf1; k++) kf_cov_off[k] = d->kf_cov_off[k];
        for (int i = 0; i < d->kf_cov_off[nkf1]; i++) kf_cov[i] = d->kf_cov[i];
    }
    // mObservations: a replaced row, else the old one
    if (d->n_obs_rows || d->n_new_mp) {
        std::vector<int> row_of(nmp1, -1);
        for (int r = 0; r < d->n_obs_rows; r++) row_of[d->obs_mp[r]] = r;
        std::vector<int32_t> off(nmp1 + 1, 0), rows;
        for (int p = 0; p < nmp1; p++) {
            off[p] = (int32_t)rows.size();
            if (row_of[p] >= 0)
                rows.insert(rows.end(), d->obs_kf + d->obs_off[row_of[p]], d->obs_kf + d->obs_off[row_of[p] + 1]);
            else if (p < nmp)
                rows.insert(rows.end(), mp_obs + mp_obs_off[p], mp_obs + mp_obs_off[p + 1]);
        }
        off[nmp1] = (int32_t)rows.size();
        std::copy(off.begin(), off.end(), mp_obs_off);
        std::copy(rows.begin(), rows.end(), mp_obs);
    }
    // SetBadFlag
    for (int i = 0; i < d->n_bad_mp; i++) mp_bad[d->bad_mp[i]] = 1;
    for (int i = 0; i < d->n_bad_kf; i++) kf_bad[d->bad_kf[i]] = 1;
    // mLastFrame's points through their MapPoint*
    if (d->n_set_mp)
        for (int i = 0; i < std::min(std::max(last_nkp, 0), cap); i++) {
            const int p = last_kp2mp[i];
            if (p < 0 || p >= M) continue;
            for (int c = 0; c < 3; c++) last_pos[3 * i + c] = map[p].pos[c];
        }
    counts[0] = nmp1;
    counts[1] = nkf1;
    return OK;
}

}  // extern "C"
