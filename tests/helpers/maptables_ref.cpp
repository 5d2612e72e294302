// The tests' serial restatement of the resident map tables' two updates
// (gf_map_tables_apply / gf_map_tables_move, include/gfslam/abi.h): a journal
// of slot writes, bad flags and observation ops applied to flat tables whose
// observation rows are slack CSR (live entries ascending, then -1 up to the
// capacity), and the regrow of such a table.
//
// One std::vector per row, one op at a time: MapPoint::AddObservation
// (src/MapPoint.cc:77-81, it overwrites), the erase of EraseObservation
// (:83-103), the clear() of SetBadFlag (:117-131) and Replace (:136-170), and
// the slot writes of KeyFrame::AddMapPoint / EraseMapPointMatch /
// ReplaceMapPointMatch. It shares no code with csrc/maptables.hip or
// gf_orb_slam_amd/maptables.py.
#include <algorithm>
#include <cstdint>
#include <vector>

namespace {

int clampi(int v, int lo, int hi) { return std::min(std::max(v, lo), hi); }

enum { OBS_SET = 0, OBS_ERASE = 1, OBS_CLEAR = 2 };

}  // namespace

extern "C" {

// row_max: the longest row an op may leave on the way (GF_MT_ROW)
void mr_apply(int nkf, const int32_t* kf_off, int32_t* slots, int nmp, uint8_t* mp_bad, const int32_t* obs_off,
              int32_t* obs_gkp, int nslot, const int32_t* slot_g, const int32_t* slot_v, int nbad, const int32_t* bad_p,
              int nrows, const int32_t* row_ids, const int32_t* row_op_off, int nops, const int32_t* ops, int row_max,
              int32_t* status) {
    const int nkp = kf_off[nkf], nobs = nmp ? obs_off[nmp] : 0;
    status[0] = status[1] = 0;
    for (int i = 0; i < nslot; i++) {
        if (slot_g[i] >= 0 && slot_g[i] < nkp) slots[slot_g[i]] = slot_v[i];
        else status[1]++;
    }
    for (int i = 0; i < nbad; i++) {
        if (bad_p[i] >= 0 && bad_p[i] < nmp) mp_bad[bad_p[i]] = 1;
        else status[1]++;
    }
    for (int r = 0; r < nrows; r++) {
        const int p = row_ids[r];
        const int o0 = clampi(row_op_off[r], 0, nops), o1 = clampi(row_op_off[r + 1], o0, nops);
        if (p < 0 || p >= nmp) {
            status[1] += o1 - o0;
            continue;
        }
        const int r0 = clampi(obs_off[p], 0, nobs), r1 = clampi(obs_off[p + 1], r0, nobs);
        std::vector<int32_t> row;
        for (int j = r0; j < r1; j++)
            if (obs_gkp[j] >= 0) row.push_back(obs_gkp[j]);
        bool over = (int)row.size() > row_max;
        for (int j = o0; j < o1 && !over; j++) {
            const int kind = ops[3 * j], kf = ops[3 * j + 1], idx = ops[3 * j + 2];
            if (kind == OBS_CLEAR) {
                row.clear();
                continue;
            }
            if ((kind != OBS_SET && kind != OBS_ERASE) || kf < 0 || kf >= nkf) {
                status[1]++;
                continue;
            }
            const int lo = kf_off[kf], hi = kf_off[kf + 1];
            if (kind == OBS_SET && (idx < 0 || idx >= hi - lo)) {
                status[1]++;
                continue;
            }
            auto mine = std::find_if(row.begin(), row.end(), [&](int32_t v) { return v >= lo && v < hi; });
            if (kind == OBS_ERASE) {
                if (mine != row.end()) row.erase(mine);
            } else if (mine != row.end()) {
                *mine = lo + idx;
            } else if ((int)row.size() + 1 > row_max) {
                over = true;
            } else {
                const auto below = std::count_if(row.begin(), row.end(), [&](int32_t v) { return v < lo; });
                row.insert(row.begin() + below, lo + idx);
            }
        }
        if (over || (int)row.size() > r1 - r0) {
            status[0]++;
            continue;
        }
        for (int j = r0; j < r1; j++) obs_gkp[j] = j - r0 < (int)row.size() ? row[j - r0] : -1;
    }
}

void mr_move(int nmp, const int32_t* old_off, const int32_t* old_gkp, const int32_t* new_off, int32_t* new_gkp,
             int32_t* status) {
    status[0] = 0;
    if (!nmp) return;
    const int no = old_off[nmp], nn = new_off[nmp];
    for (int p = 0; p < nmp; p++) {
        const int o0 = clampi(old_off[p], 0, no), o1 = clampi(old_off[p + 1], o0, no);
        const int n0 = clampi(new_off[p], 0, nn), n1 = clampi(new_off[p + 1], n0, nn);
        std::vector<int32_t> row;
        for (int j = o0; j < o1; j++)
            if (old_gkp[j] >= 0) row.push_back(old_gkp[j]);
        if ((int)row.size() > n1 - n0) {
            status[0]++;
            row.clear();
        }
        for (int j = n0; j < n1; j++) new_gkp[j] = j - n0 < (int)row.size() ? row[j - n0] : -1;
    }
}

}  // extern "C"
