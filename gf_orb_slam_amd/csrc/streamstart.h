// Stream start (gf_frontend_start_streams): the staged form of a call's
// requests and the launch of the kernel that clears a named stream and
// installs its last frame and state words (streamstart.hip). The map rows go
// through the map update's launches (mapupdate.h) with every "before" count
// of their header 0 (the host packs it from emptied mirrors), the database
// rows through the growable database's (reloc.h) against the emptied record. The
// front end validates and packs on the host (frontend.hip).
#pragma once
#include "common.h"
#include "reloc.h"

namespace gf {

// One named stream of a call, at the head of the staging buffer; request l is
// also delta l of the map update's staging (MuHdr l). Section offsets in bytes
// from the staging base, every section 16-byte aligned.
struct SsHdr {
    int32_t stream, n_last;
    int32_t frame_id, since_reloc, ref_kf;
    int32_t clear_db;          // 1: the stream's growable database is emptied
    int64_t kps, desc, kp2mp;  // [n_last] rows of the frame that becomes mLastFrame
    double timestamp;
    float Tcw[16];
    KfdbDev* db_rec;           // the growable database's own record, or null
};

struct StreamStartArgs {
    const uint8_t* stage;     // SsHdr[L], then the sections
    const uint8_t* mu_stage;  // the map update's staging: MuHdr[L], then the new points
    int L, B, M, cap;
    // current frame
    int32_t* kp2mp;
    uint8_t* outl;
    // last frame
    gf_keypoint* last_kps;
    uint8_t* last_desc;
    int32_t* last_nkp;
    int32_t* last_kp2mp;
    uint8_t* last_outl;
    float* last_pos;
    float* Tcw_last;
    double* t_prev;
    double* t_cur;
    // words and holders
    int32_t* track;     // [B][GF_TR_N]
    int32_t* kf_state;  // [B][GF_KF_N] or null (no keyframe stage)
    int32_t* ref_kf;    // [B] the persistent reference-keyframe word
    int32_t* nleft;     // [B]
    int32_t* nlist;     // [B]
    int32_t* st_nleft;  // [B] GF_ST_NLEFT column
    double* Xv;         // [B][13]
    double* Xv_next;    // [B][13]
    double* base;       // [B][49]
    // counts the map update's last kernel sets again
    int32_t* nmp;
    int32_t* kfc;
    gf_covis_map* covis;
    // relocalisation state, null without the relocalisation buffers
    gf_reloc_kf* rkf;   // [B][RL_NC]
    int32_t* ncand;     // [B]
    KfdbDev* fe_rec;    // [B] the front end's stream records
};

int stream_start_launch(gf_ctx* ctx, const StreamStartArgs& a, hipStream_t s);

// gf_frontend_force_relocalisation: the staged requests are (stream, last_kf)
// pairs, last_kf -1 for the newest keyframe that is not bad.
struct ForceRelocArgs {
    const int32_t* stage;  // [n][2]
    int n, B;
    int32_t* track;              // [B][GF_TR_N]
    const gf_covis_map* covis;   // [B]
};
int force_reloc_launch(gf_ctx* ctx, const ForceRelocArgs& a, hipStream_t s);

}  // namespace gf
