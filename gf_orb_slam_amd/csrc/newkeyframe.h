// NeedNewKeyFrame / CreateNewKeyFrame (newkeyframe.hip): what the front end's
// step and its hand-over entries call.
#pragma once
#include "common.h"

namespace gf {

// Tracking::NeedNewKeyFrame (Tracking.cc:3035-3077) on scalars, in the
// reference's order: the GF_KF_DECISION bits (1 always set). n_ref < 0: no
// reference keyframe. Shared by the kernel and gf_need_new_keyframe.
__host__ __device__ inline int need_keyframe_rule(int since_kf, int since_reloc, int stop, int nkf, int n_ref,
                                                  int inliers, int accept, int min_frames, int max_frames) {
    int d = 1;
    if (stop) return d | 2;                                       // :3042
    if (since_reloc < max_frames && nkf > max_frames) return d | 4;  // :3046
    if (n_ref < 0) return d | 256;                                // mpReferenceKF == NULL
    const bool c1a = since_kf >= max_frames;                      // :3056
    const bool c1b = since_kf >= min_frames && accept;            // :3058
    const bool c2 = inliers < n_ref * 0.9 && inliers > 15;        // :3060, the product a double
    d |= (c1a ? 8 : 0) | (c1b ? 16 : 0) | (c2 ? 32 : 0);
    if ((c1a || c1b) && c2) d |= accept ? 64 : 128;               // :3065-3073
    return d;
}

// k_need_keyframe over args (device pointers) on s.
int need_keyframe_launch(gf_ctx* ctx, const gf_newkf_args& a, hipStream_t s);

// The pack buffer of gf_frontend_take_keyframes (device memory, rows = B x cap).
struct KeyframePack {
    int32_t* totals;        // [2] keyframes, rows
    int32_t* list;          // [B] taken streams, ascending
    int32_t* rowoff;        // [B] their first rows (exclusive sums of N)
    gf_keyframe_hdr* hdr;   // [B]
    gf_keypoint* kps;       // [rows]
    uint8_t* desc;          // [rows][32]
    int32_t* slots;         // [rows]
};
// k_keyframe_pack: the first max_kf pending outbox slots of a, ascending, into p.
int keyframe_pack_launch(gf_ctx* ctx, const gf_newkf_args& a, const KeyframePack& p, int max_kf, hipStream_t s);
// PENDING = 0 on the streams p.list names (p.totals[0] of them).
int keyframe_clear_launch(gf_ctx* ctx, const gf_newkf_args& a, const KeyframePack& p, hipStream_t s);

}  // namespace gf
