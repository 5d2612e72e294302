// The counting of LocalMapping::KeyFrameCulling (src/LocalMapping.cc:562-616):
//
//   k_kfcull_count: for every candidate keyframe, nMPs and
//     nRedundantObservations of :576-611 over flat tables: the slot tables and
//     keypoint octaves of all keyframes back to back (kf_off), the bad flags
//     of the points and the observation maps as CSR rows of global keypoint
//     indices (kf_off[kf'] + idx'), -1 = an erased observation. One workgroup
//     per candidate, one lane per slot; a row's entries are loaded eight at a
//     time and their octaves gathered together, so the chain slot -> row ->
//     octave waits once per stage and not once per observation.
//
// The decision nRedundantObservations > 0.9 * nMPs (:613) is a double
// comparison and KeyFrame::SetBadFlag is map surgery: both stay with the
// caller (gf_orb_slam_amd/localmapping.py: keyframe_culling).
#include <vector>

#include "common.h"

#define KC_THREADS 256
#define KC_BATCH 8
#define KC_MAX_KP 4096

namespace {

__global__ __launch_bounds__(KC_THREADS) void k_kfcull_count(
    int nkf, int nkp, const int32_t* __restrict__ kf_off, const uint8_t* __restrict__ octave,
    const int32_t* __restrict__ slots, int nmp, const uint8_t* __restrict__ mp_bad,
    const int32_t* __restrict__ obs_off, const int32_t* __restrict__ obs_gkp, int nobs,
    const int32_t* __restrict__ cand, int32_t* __restrict__ counts, uint8_t* __restrict__ flags) {
    __shared__ int red[2 * (KC_THREADS / 64)];
    const int tid = threadIdx.x;
    const int K = gfd::ldg(cand + blockIdx.x);
    int s0 = 0, s1 = 0;
    if (K >= 0 && K < nkf) {
        s0 = min(max(gfd::ldg(kf_off + K), 0), nkp);
        s1 = min(max(gfd::ldg(kf_off + K + 1), s0), nkp);
    }
    int nmps = 0, nred = 0;
    for (int i = s0 + tid; i < s1; i += KC_THREADS) {
        const int p = gfd::ldg(slots + i);
        uint8_t flag = 0;
        if (p >= 0 && p < nmp) {  // pMP (:581)
            const int bad = gfd::ldg(mp_bad + p), level = gfd::ldg(octave + i);
            const int r0 = max(gfd::ldg(obs_off + p), 0), r1 = min(gfd::ldg(obs_off + p + 1), nobs);
            if (!bad) {  // :583
                flag = 1;
                nmps++;
                int live = 0, nobs_ok = 0;  // Observations(), nObs without its early exit
                for (int r = r0; r < r1; r += KC_BATCH) {
                    int g[KC_BATCH], o[KC_BATCH];
#pragma unroll
                    for (int j = 0; j < KC_BATCH; j++) g[j] = r + j < r1 ? gfd::ldg(obs_gkp + r + j) : -1;
#pragma unroll
                    for (int j = 0; j < KC_BATCH; j++) {
                        if (g[j] >= nkp) g[j] = -1;
                        o[j] = g[j] >= 0 ? (int)gfd::ldg(octave + g[j]) : 0;
                    }
#pragma unroll
                    for (int j = 0; j < KC_BATCH; j++) {
                        const bool is_live = g[j] >= 0;
                        live += is_live;
                        // pKFi != pKF (:594) and scaleLeveli <= scaleLevel + 1 (:597)
                        nobs_ok += is_live && !(g[j] >= s0 && g[j] < s1) && o[j] <= level + 1;
                    }
                }
                if (live > 3 && nobs_ok >= 3) {  // :586, :604
                    flag = 2;
                    nred++;
                }
            }
        }
        if (flags) flags[i] = flag;
    }
    nmps = gfd::warp_sum(nmps);
    nred = gfd::warp_sum(nred);
    if ((tid & 63) == 0) {
        red[2 * (tid >> 6)] = nmps;
        red[2 * (tid >> 6) + 1] = nred;
    }
    __syncthreads();
    if (tid < 2) {
        int v = 0;
        for (int w = 0; w < KC_THREADS / 64; w++) v += red[2 * w + tid];
        counts[2 * blockIdx.x + tid] = v;
    }
}

}  // namespace

extern "C" {

// LocalMapping.cc:562-616, the counting of every candidate in one launch on device tables
int gf_keyframe_culling_counts_dev(gf_ctx* ctx, int nkf, int nkp, const int32_t* d_kf_off, const uint8_t* d_octave,
                                   const int32_t* d_slots, int nmp, const uint8_t* d_mp_bad, const int32_t* d_obs_off,
                                   const int32_t* d_obs_gkp, int nobs, int ncand, const int32_t* d_cand,
                                   int32_t* d_counts, uint8_t* d_flags, void* stream) {
    GF_CHECK(ctx, GF_ERR_ARG, "gf_keyframe_culling_counts_dev: null arg");
    if (ncand <= 0) return GF_OK;
    GF_CHECK(nkf >= 0 && nkp >= 0 && nmp >= 0 && nobs >= 0, GF_ERR_ARG, "gf_keyframe_culling_counts_dev: negative size");
    GF_CHECK(d_kf_off && d_cand && d_counts, GF_ERR_ARG, "gf_keyframe_culling_counts_dev: null buffer");
    GF_CHECK(nkp == 0 || (d_octave && d_slots), GF_ERR_ARG, "gf_keyframe_culling_counts_dev: null keyframe table");
    GF_CHECK(nmp == 0 || (d_mp_bad && d_obs_off), GF_ERR_ARG, "gf_keyframe_culling_counts_dev: null point table");
    GF_CHECK(nobs == 0 || d_obs_gkp, GF_ERR_ARG, "gf_keyframe_culling_counts_dev: null observation table");
    hipStream_t s = (hipStream_t)stream;
    GF_PROF(ctx, s, "k_kfcull_count");
    GF_LAUNCH(k_kfcull_count, ncand, KC_THREADS, 0, s, nkf, nkp, d_kf_off, d_octave, d_slots, nmp, d_mp_bad, d_obs_off,
              d_obs_gkp, nobs, d_cand, d_counts, d_flags);
    GF_HIP(hipGetLastError());
    return GF_OK;
}

// LocalMapping.cc:562-616, the counting on host arrays, synchronous
int gf_keyframe_culling_counts(gf_ctx* ctx, int nkf, const int32_t* kf_off, const uint8_t* octave, const int32_t* slots,
                               int nmp, const uint8_t* mp_bad, const int32_t* obs_off, const int32_t* obs_gkp,
                               int ncand, const int32_t* cand, int32_t* counts, uint8_t* flags) {
    GF_CHECK(ctx, GF_ERR_ARG, "gf_keyframe_culling_counts: null arg");
    if (ncand <= 0) return GF_OK;
    GF_CHECK(nkf >= 0 && nmp >= 0, GF_ERR_ARG, "gf_keyframe_culling_counts: negative size");
    GF_CHECK(kf_off && cand && counts, GF_ERR_ARG, "gf_keyframe_culling_counts: null buffer");
    GF_CHECK(kf_off[0] == 0, GF_ERR_ARG, "kf_off[0] must be 0");
    for (int k = 0; k < nkf; k++) {
        GF_CHECK(kf_off[k + 1] >= kf_off[k], GF_ERR_ARG, "kf_off must be non-decreasing");
        GF_CHECK(kf_off[k + 1] - kf_off[k] <= KC_MAX_KP, GF_ERR_CAP, "at most 4096 keypoints per keyframe");
    }
    const int nkp = kf_off[nkf];
    GF_CHECK(nkp == 0 || (octave && slots), GF_ERR_ARG, "gf_keyframe_culling_counts: null keyframe table");
    GF_CHECK(nmp == 0 || (mp_bad && obs_off), GF_ERR_ARG, "gf_keyframe_culling_counts: null point table");
    int nobs = 0;
    if (nmp) {
        GF_CHECK(obs_off[0] == 0, GF_ERR_ARG, "obs_off[0] must be 0");
        for (int p = 0; p < nmp; p++)
            GF_CHECK(obs_off[p + 1] >= obs_off[p], GF_ERR_ARG, "obs_off must be non-decreasing");
        nobs = obs_off[nmp];
    }
    GF_CHECK(nobs == 0 || obs_gkp, GF_ERR_ARG, "gf_keyframe_culling_counts: null observation table");
    for (int o = 0; o < nobs; o++)
        GF_CHECK(obs_gkp[o] >= -1 && obs_gkp[o] < nkp, GF_ERR_ARG, "observation entry out of range");
    for (int c = 0; c < ncand; c++) GF_CHECK(cand[c] >= 0 && cand[c] < nkf, GF_ERR_ARG, "candidate out of range");
    GF_HIP(hipSetDevice(ctx->device));
    // one scratch block: [kf_off | octave | slots | mp_bad | obs_off | obs_gkp | cand | counts | flags]
    size_t off = 0;
    std::vector<std::pair<const void*, size_t>> parts;
    auto add = [&](const void* h, size_t bytes) {
        const size_t o = off;
        parts.push_back({h, bytes});
        off += (bytes + 15) & ~(size_t)15;
        return o;
    };
    const size_t NK = (size_t)nkp, NM = (size_t)nmp, NC = (size_t)ncand;
    const size_t o_ko = add(kf_off, 4 * ((size_t)nkf + 1)), o_oc = add(octave, NK), o_sl = add(slots, 4 * NK),
                 o_mb = add(mp_bad, NM), o_oo = add(nmp ? obs_off : nullptr, nmp ? 4 * (NM + 1) : 0),
                 o_og = add(obs_gkp, 4 * (size_t)nobs), o_ca = add(cand, 4 * NC), o_cn = add(nullptr, 8 * NC),
                 o_fl = add(flags, flags ? NK : 0);
    void* dbuf;
    int rc = gf::ws_get(ctx, 69, off, &dbuf);
    if (rc) return rc;
    uint8_t* base = (uint8_t*)dbuf;
    hipStream_t s = ctx->stream;
    size_t cur = 0;
    for (auto& pr : parts) {
        if (pr.second && pr.first) GF_HIP(hipMemcpyAsync(base + cur, pr.first, pr.second, hipMemcpyHostToDevice, s));
        cur += (pr.second + 15) & ~(size_t)15;
    }
    rc = gf_keyframe_culling_counts_dev(ctx, nkf, nkp, (const int32_t*)(base + o_ko), base + o_oc,
                                        (const int32_t*)(base + o_sl), nmp, base + o_mb, (const int32_t*)(base + o_oo),
                                        (const int32_t*)(base + o_og), nobs, ncand, (const int32_t*)(base + o_ca),
                                        (int32_t*)(base + o_cn), flags && nkp ? base + o_fl : nullptr, s);
    if (rc) return rc;
    GF_HIP(hipMemcpyAsync(counts, base + o_cn, 8 * NC, hipMemcpyDeviceToHost, s));
    if (flags && nkp) GF_HIP(hipMemcpyAsync(flags, base + o_fl, NK, hipMemcpyDeviceToHost, s));
    GF_HIP(hipStreamSynchronize(s));
    return GF_OK;
}

}  // extern "C"
