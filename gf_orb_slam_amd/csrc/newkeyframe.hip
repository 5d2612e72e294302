// Tracking::NeedNewKeyFrame / CreateNewKeyFrame (Tracking.cc:3035-3092) for B
// streams, and the hand-over of the created keyframes (LocalMapping::
// InsertKeyFrame, LocalMapping.cc:149-155):
//   k_need_keyframe   one workgroup per stream: nRefMatches =
//                     mpReferenceKF->TrackedMapPoints() (KeyFrame.cc:253-265),
//                     the rule, and for a stream that creates the snapshot of
//                     `new KeyFrame(mCurrentFrame, ...)` (KeyFrame.cc:30-54)
//                     into its outbox slot, outliers still in place
//   k_keyframe_scan   the pending outbox slots as an ascending list with
//                     exclusive row offsets (one workgroup)
//   k_keyframe_pack   their headers and rows into one contiguous buffer
//   k_keyframe_clear  PENDING = 0 on the listed streams
// The state words are GF_KF_* (include/gfslam/abi.h). No atomics: every word
// has one writer, so the results do not depend on scheduling.
#include "newkeyframe.h"

namespace {

constexpr int KF_U = 4;          // loads in flight per thread, as k_fe_end's END_U
constexpr int PACK_ROWS = 128;   // rows a k_keyframe_pack workgroup copies

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// n words from src to dst: each round KF_U loads (clamped, unconditional),
// then their stores, so the loads of a round do not wait on one another.
template <typename T>
__device__ __forceinline__ void copy_rows(const T* __restrict__ src, T* __restrict__ dst, int n) {
    for (int i0 = threadIdx.x; i0 < n; i0 += 256 * KF_U) {
        T v[KF_U];
#pragma unroll
        for (int u = 0; u < KF_U; u++) v[u] = src[min(i0 + 256 * u, n - 1)];
#pragma unroll
        for (int u = 0; u < KF_U; u++)
            if (i0 + 256 * u < n) dst[i0 + 256 * u] = v[u];
    }
}

__global__ __launch_bounds__(256) void k_need_keyframe(gf_newkf_args A) {
    __shared__ int s_wave[4];
    __shared__ int s_create;
    const int b = blockIdx.x, t = threadIdx.x;
    int32_t* S = A.state + (size_t)b * GF_KF_N;
    // a parked stream (GF_TR_PATH 4) has no frame of its map: its words stay, SINCE included (uniform)
    if (A.track[(size_t)b * GF_TR_N + GF_TR_PATH] == 4) return;
    const bool working = A.working[b] != 0;  // mState == WORKING (Tracking.cc:854)
    // phase 1: TrackedMapPoints of the reference keyframe: slots that are not
    // NULL (bad points count, as a non-NULL pointer does)
    int ref = -1;
    if (working) {
        ref = A.ref_kf[b];
        if (ref < 0 || ref >= A.kf_count[b]) ref = -1;
    }
    int c = 0;
    if (ref >= 0) {  // uniform over the workgroup
        const int32_t* off = A.kf_mp_off + (long long)b * A.off_stride;
        const int o0 = off[ref], n = max(off[ref + 1] - o0, 0);
        const int32_t* row = A.kf_mp + (long long)b * A.slot_stride + o0;
        // CSR offsets are arbitrary: scalar loads up to the first 16-byte
        // boundary, int4 loads over the body, scalar loads over the tail
        const int head = min(n, (int)((4 - (((uintptr_t)row >> 2) & 3)) & 3));
        const int nv = (n - head) >> 2, tail = head + 4 * nv;
        if (t < head) c += row[t] != -1;
        const int4* v = (const int4*)(row + head);
        for (int i = t; i < nv; i += 256) {
            const int4 q = v[i];
            c += (q.x != -1) + (q.y != -1) + (q.z != -1) + (q.w != -1);
        }
        if (tail + t < n) c += row[tail + t] != -1;
    }
    c = gfd::warp_sum(c);
    if ((t & 63) == 0) s_wave[t >> 6] = c;
    __syncthreads();
    // phase 2: the rule (one lane), the state words, the verdict through LDS
    if (t == 0) {
        const int nref = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
        const int32_t* T = A.track + (size_t)b * GF_TR_N;
        const int since = min(S[GF_KF_SINCE] + 1, 1 << 30);  // mnId - mnLastKeyFrameId of this frame
        int d = 0, inl = 0;
        if (working) {
            inl = A.inliers[b];
            const int nkf = S[GF_KF_NKF] != -1 ? S[GF_KF_NKF] : A.kf_count[b];
            // a pending outbox slot reads as "not accepting": an untaken keyframe is never overwritten
            const int accept = S[GF_KF_ACCEPT] != 0 && S[GF_KF_PENDING] == 0;
            d = gf::need_keyframe_rule(since, T[GF_TR_SINCE], S[GF_KF_STOP] != 0, nkf, ref >= 0 ? nref : -1, inl, accept,
                                       A.min_frames, A.max_frames);
        }
        const int create = d & 64;
        S[GF_KF_DECISION] = d;
        S[GF_KF_REF] = ref;
        S[GF_KF_REF_MATCHES] = nref;
        S[GF_KF_INLIERS] = inl;
        if (d & 128) S[GF_KF_ABORT] = 1;  // InterruptBA (:3071)
        if (create) {
            // CreateNewKeyFrame (:3086-3090) and InsertKeyFrame (LocalMapping.cc:149-155, :70)
            const int n = clampi(A.nkp[b], 0, A.cap);
            const int seq = S[GF_KF_SEQ] + 1;
            S[GF_KF_SINCE] = 0;   // mnLastKeyFrameId = mnId
            S[GF_KF_ACCEPT] = 0;  // SetAcceptKeyFrames(false)
            S[GF_KF_ABORT] = 1;   // mbAbortBA = true
            S[GF_KF_SEQ] = seq;
            S[GF_KF_PENDING] = 1;
            S[GF_KF_FRAME] = T[GF_TR_QUERY];
            gf_keyframe_hdr h;
            h.stream = b;
            h.seq = seq;
            h.frame_id = T[GF_TR_QUERY];
            h.n = n;
            h.timestamp = A.t_cur[b];
            for (int i = 0; i < 16; i++) h.Tcw[i] = A.Tcw[16 * b + i];
            A.out_hdr[b] = h;
        } else {
            S[GF_KF_SINCE] = since;
        }
        s_create = create;
    }
    __syncthreads();
    if (!s_create) return;  // uniform: a stream that does not create writes nothing into the outbox
    // phase 3: the snapshot, rows < N only
    const int n = clampi(A.nkp[b], 0, A.cap);
    const long long o = (long long)b * A.cap;
    constexpr int KW = sizeof(gf_keypoint) / 4;
    copy_rows((const uint32_t*)(A.kps + o), (uint32_t*)(A.out_kps + o), KW * n);
    copy_rows((const uint4*)(A.desc + o * 32), (uint4*)(A.out_desc + o * 32), 2 * n);
    copy_rows(A.kp2mp + o, A.out_slots + o, n);  // mvpMapPoints, outliers included (:899-902)
}

__global__ __launch_bounds__(256) void k_keyframe_scan(gf_newkf_args A, gf::KeyframePack P, int max_kf) {
    __shared__ int s_c[256], s_r[256];
    __shared__ int base_c, base_r;
    const int t = threadIdx.x;
    if (t == 0) base_c = base_r = 0;
    __syncthreads();
    for (int b0 = 0; b0 < A.B; b0 += 256) {
        const int b = b0 + t;
        const int f = b < A.B && A.state[(size_t)b * GF_KF_N + GF_KF_PENDING] != 0;
        const int n = f ? clampi(A.out_hdr[b].n, 0, A.cap) : 0;
        s_c[t] = f;
        s_r[t] = n;
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {  // inclusive scan of the flags and of the row counts
            const int vc = t >= o ? s_c[t - o] : 0, vr = t >= o ? s_r[t - o] : 0;
            __syncthreads();
            s_c[t] += vc;
            s_r[t] += vr;
            __syncthreads();
        }
        const int j = base_c + s_c[t] - f, r = base_r + s_r[t] - n;  // exclusive
        if (f && j < max_kf) {
            P.list[j] = b;
            P.rowoff[j] = r;
        }
        if (f && j == max_kf) P.totals[1] = r;  // rows of the max_kf taken ones
        __syncthreads();
        if (t == 255) {
            base_c += s_c[255];
            base_r += s_r[255];
        }
        __syncthreads();
    }
    if (t == 0) {
        P.totals[0] = min(base_c, max_kf);
        if (base_c <= max_kf) P.totals[1] = base_r;
    }
}

// grid (row chunks, B): workgroup (x, j) copies rows [x * PACK_ROWS, ...) of the j-th listed stream
__global__ __launch_bounds__(256) void k_keyframe_pack(gf_newkf_args A, gf::KeyframePack P) {
    const int j = blockIdx.y;
    if (j >= P.totals[0]) return;
    const int b = P.list[j];
    const int n = clampi(A.out_hdr[b].n, 0, A.cap);
    const int k0 = blockIdx.x * PACK_ROWS;
    if (blockIdx.x == 0 && threadIdx.x == 0) P.hdr[j] = A.out_hdr[b];
    if (k0 >= n) return;
    const int np = min(PACK_ROWS, n - k0);
    const long long so = (long long)b * A.cap + k0, dst = (long long)P.rowoff[j] + k0;
    constexpr int KW = sizeof(gf_keypoint) / 4;
    copy_rows((const uint32_t*)(A.out_kps + so), (uint32_t*)(P.kps + dst), KW * np);
    copy_rows((const uint4*)(A.out_desc + so * 32), (uint4*)(P.desc + dst * 32), 2 * np);
    copy_rows(A.out_slots + so, P.slots + dst, np);
}

__global__ __launch_bounds__(256) void k_keyframe_clear(gf_newkf_args A, gf::KeyframePack P) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j < P.totals[0]) A.state[(size_t)P.list[j] * GF_KF_N + GF_KF_PENDING] = 0;
}

}  // namespace

namespace gf {

int need_keyframe_launch(gf_ctx* ctx, const gf_newkf_args& a, hipStream_t s) {
    GF_PROF(ctx, s, "k_need_keyframe");
    GF_LAUNCH(k_need_keyframe, a.B, 256, 0, s, a);
    GF_HIP(hipGetLastError());
    return GF_OK;
}

int keyframe_pack_launch(gf_ctx* ctx, const gf_newkf_args& a, const KeyframePack& p, int max_kf, hipStream_t s) {
    {
        GF_PROF(ctx, s, "k_keyframe_scan");
        GF_LAUNCH(k_keyframe_scan, 1, 256, 0, s, a, p, max_kf);
        GF_HIP(hipGetLastError());
    }
    GF_PROF(ctx, s, "k_keyframe_pack");
    GF_LAUNCH(k_keyframe_pack, dim3((a.cap + PACK_ROWS - 1) / PACK_ROWS, a.B), 256, 0, s, a, p);
    GF_HIP(hipGetLastError());
    return GF_OK;
}

int keyframe_clear_launch(gf_ctx* ctx, const gf_newkf_args& a, const KeyframePack& p, hipStream_t s) {
    GF_LAUNCH(k_keyframe_clear, (a.B + 255) / 256, 256, 0, s, a, p);
    GF_HIP(hipGetLastError());
    return GF_OK;
}

}  // namespace gf

extern "C" {

int gf_need_new_keyframe(int since_kf, int since_reloc, int stop, int nkf, int n_ref_matches, int inliers, int accept,
                         int min_frames, int max_frames, int* need, int* decision) {
    GF_CHECK(need, GF_ERR_ARG, "null arg");
    const int d = gf::need_keyframe_rule(since_kf, since_reloc, stop != 0, nkf, n_ref_matches, inliers, accept != 0,
                                         min_frames, max_frames);
    *need = (d & 64) ? 1 : 0;
    if (decision) *decision = d;
    return GF_OK;
}

int gf_need_new_keyframe_dev(gf_ctx* ctx, const gf_newkf_args* a, void* stream) {
    GF_CHECK(ctx && a, GF_ERR_ARG, "null arg");
    GF_CHECK(a->B > 0 && a->cap > 0, GF_ERR_ARG, "bad batch / capacity");
    GF_CHECK(a->nkp && a->kps && a->desc && a->kp2mp && a->Tcw && a->t_cur && a->track && a->inliers && a->working &&
                 a->ref_kf && a->kf_count && a->kf_mp_off && a->kf_mp && a->state && a->out_hdr && a->out_kps &&
                 a->out_desc && a->out_slots,
             GF_ERR_ARG, "null array");
    GF_CHECK(a->off_stride >= 2 && a->slot_stride >= 0 && a->min_frames >= 0 && a->max_frames > 0, GF_ERR_ARG,
             "bad strides / frame limits");
    // the descriptor rows move as uint4
    GF_CHECK(((uintptr_t)a->desc & 15) == 0 && ((uintptr_t)a->out_desc & 15) == 0, GF_ERR_ARG,
             "descriptor arrays must be 16-byte aligned");
    GF_HIP(hipSetDevice(ctx->device));
    return gf::need_keyframe_launch(ctx, *a, (hipStream_t)stream);
}

}  // extern "C"
