// Map feedback (gf_frontend_update_maps): the staged form of a call's deltas
// and the launch of the kernels that apply them (mapupdate.hip). The front end
// validates and packs on the host (frontend.hip).
#pragma once
#include "common.h"

namespace gf {

// One listed stream of a call, at the head of the staging buffer. Counts
// before (0) and after (1) the delta; section offsets in bytes from the
// staging base, every section 16-byte aligned.
struct MuHdr {
    int32_t stream, nmp0, nmp1, nkf0, nkf1;
    int32_t n_set, n_bad_mp, n_bad_kf, n_slot, has_cov;
    int32_t ns0, ns1;  // slots of all keyframes
    int32_t nc0, nc1;  // covisibility entries
    int32_t no0, no1;  // observations
    int32_t do_obs;    // the observation CSR changes (a replaced row or an appended point)
    int32_t pad;
    int64_t new_mp, new_desc, new_bad;  // [nmp1 - nmp0] rows
    int64_t set_idx, set_mp, set_desc;  // [n_set]
    int64_t bad_mp, bad_kf;             // index lists
    int64_t kf_off, kf_mp, kf_bad;      // [nkf1 - nkf0 + 1] absolute offsets from ns0, the slots, the flags
    int64_t slot_pos, slot_val;         // [n_slot] position in the stream's kf_mp, value
    int64_t row_of;                     // [nmp1] replaced row of a point, -1: its row stays
    int64_t obs_off, obs_kf;            // the replaced rows as a CSR
    int64_t cov_off, cov;               // [nkf1 + 1], [nc1] when has_cov
};

struct MapUpdateArgs {
    const uint8_t* stage;  // MuHdr[L], then the sections
    int L, M, cap, kf_cap;
    long long slot_cap;
    // the stream maps
    gf_map_point* map;
    uint8_t* desc;
    float* pos;
    int32_t* upd;
    gf_mp_view* views;
    int32_t* nmp;
    int32_t* kfc;
    // the keyframe graphs: per-stream slabs of kf_cap (+ 1), slot_cap, kf_cap^2, M (+ 1) entries
    gf_covis_map* covis;
    uint8_t *kf_bad, *mp_bad;
    int32_t *kf_mp_off, *kf_mp, *kf_cov_off, *kf_cov, *mp_obs_off, *mp_obs;
    // the last frame's cache of its points' positions
    const int32_t* last_kp2mp;
    const int32_t* last_nkp;
    float* last_pos;
    // observation rebuild: new offsets [L][M + 1], new rows [L][slot_cap]
    int32_t* obs_off_new;
    int32_t* obs_new;
};

// Largest per-stream counts of the call, for the grids.
struct MapUpdateShape {
    int new_mp = 0, set_mp = 0, new_slots = 0, slot_writes = 0, cov = 0, nmp1 = 0, no1 = 0;
    bool any_new_kf = false, any_cov = false, any_obs = false;
};

int map_update_launch(gf_ctx* ctx, const MapUpdateArgs& a, const MapUpdateShape& sh, hipStream_t s);

}  // namespace gf
