// Map compaction (gf_frontend_compact_maps): the staged form of a call's
// requests and the launch of the kernels that restrict the stream maps in
// place (mapcompact.hip). The front end validates on the host, downloads the
// device's verdict and refreshes its mirrors (frontend.hip).
#pragma once
#include "common.h"

namespace gf {

// One listed stream of a call, at the head of the staging buffer. The drop
// lists follow the headers as int32 arrays; offsets in int32 words from the
// staging base.
struct McHdr {
    int32_t stream, nmp0, nkf0;
    int32_t n_drop_kf, n_drop_mp;
    int32_t drop_kf, drop_mp;  // word offsets of the lists
    int32_t pad;
};

// What the device decided for one listed stream (int32 words of mc_res).
enum { MC_NKF = 0, MC_NMP, MC_KEPT_KF, MC_KEPT_MP, MC_NS, MC_NC, MC_NO, MC_RES_N = 8 };

struct MapCompactArgs {
    const int32_t* stage;  // McHdr[L], then the lists
    int L, M, cap, kf_cap;
    long long slot_cap;
    // per-point rows of the stream maps, [B][M] each
    gf_map_point* map;
    uint8_t* desc;
    float* pos;
    gf_mp_view* views;
    double* H;
    double* info;
    double* info_lt;
    float* uv;
    int32_t* upd;
    uint8_t* updated;
    uint8_t* mp_bad;
    // per-keyframe rows
    uint8_t* kf_bad;
    gf_reloc_kf* reloc;  // [B][kf_cap]
    // the keyframe graphs
    int32_t *kf_mp_off, *kf_mp, *kf_cov_off, *kf_cov, *mp_obs_off, *mp_obs;
    // the counts the step reads
    int32_t* nmp;
    int32_t* kfc;
    gf_covis_map* covis;
    // index holders
    int32_t* kp2mp;
    const int32_t* nkp;
    int32_t* last_kp2mp;
    const int32_t* last_nkp;
    int32_t* left;
    const int32_t* nleft;
    int32_t* ref_kf;
    int32_t* track;             // [B][GF_TR_N]: GF_TR_FORCE_KF of a pending forced relocalisation
    int32_t* kf_state;          // [B][GF_KF_N] or null: no keyframe stage
    const gf_keyframe_hdr* out_hdr;
    int32_t* out_slots;         // [B][cap]
    // outputs and scratch, per listed stream
    int32_t* mp_remap;     // [L][M]: keep flags after the mark pass, new indices after the scan
    int32_t* kf_remap;     // [L][kf_cap]
    int32_t* res;          // [L][MC_RES_N]
    int32_t* obs_off_new;  // [L][M + 1]
    int32_t* obs_new;      // [L][slot_cap]
};

int map_compact_launch(gf_ctx* ctx, const MapCompactArgs& a, hipStream_t s);

}  // namespace gf
