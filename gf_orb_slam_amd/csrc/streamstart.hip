// Stream start (gf_frontend_start_streams): one stream's beginning on the
// device, Tracking::CreateInitialMap's hand-over to the tracker
// (Tracking.cc:1302-1321) for the streams a call names, while the other
// streams of the batch keep running.
//   k_ss_install  grid (row chunk x named stream): the frame that becomes
//                 mLastFrame with GF_FE_LAST_POS gathered from the staged new
//                 points, the current frame's match arrays cleared, the
//                 tracking and keyframe words, the observability state, the
//                 relocalisation query rows, and the growable database's
//                 records emptied (KeyFrameDatabase::clear) before the rows'
//                 append. The stream's counts are zeroed too, so that it holds
//                 an empty map until the map update's last kernel sets the new
//                 ones; the map update's kernels do not read them: they take
//                 every "before" count from their header, which the host packed
//                 from mirrors it had emptied, and that is what makes the delta
//                 the whole map
//   k_force_reloc the request of gf_frontend_force_relocalisation: the three
//                 tracking words of each named stream, one thread a request
// Every destination has one writer: a row chunk belongs to one workgroup and
// the words of a stream to chunk 0. Nothing waits on another workgroup; a
// stream not named is not touched and costs nothing. The kernel runs on the
// context's stream behind the uploads of its own staging and of the map
// update's, and before the map update's kernels.
#include "streamstart.h"

#include "mapupdate.h"

namespace {

using gf::SsHdr;
using gf::StreamStartArgs;

constexpr int SS_ROWS = 256;  // last-frame rows per workgroup, one per thread
constexpr int KP_WORDS = (int)(sizeof(gf_keypoint) / 4);
constexpr int RKF_WORDS = gf::RL_NC * (int)(sizeof(gf_reloc_kf) / 4);
static_assert(sizeof(gf_keypoint) % 4 == 0, "keypoints move as words");
static_assert(RKF_WORDS <= SS_ROWS, "one relocalisation-state word per thread");
static_assert(sizeof(gf_map_point) == 32, "a staged point is two uint4");

__global__ __launch_bounds__(SS_ROWS) void k_ss_install(StreamStartArgs A) {
    const int l = blockIdx.y, t = threadIdx.x;
    const SsHdr* H = reinterpret_cast<const SsHdr*>(A.stage) + l;
    const gf::MuHdr* MH = reinterpret_cast<const gf::MuHdr*>(A.mu_stage) + l;
    const int b = H->stream;
    const long long o = (long long)b * A.cap;
    const int k0 = blockIdx.x * SS_ROWS;
    if (k0 < A.cap) {
        // the current frame holds no match of the old map (mvpMapPoints NULL, mvbOutlier false)
        const int i = k0 + t;
        if (i < A.cap) {
            A.kp2mp[o + i] = -1;
            A.outl[o + i] = 0;
        }
    }
    const int n = H->n_last;
    if (k0 < n) {
        // mLastFrame = Frame(mCurrentFrame) (:1308): keypoints as words, descriptors as uint4 (two a row; the
        // staged sections are 16-byte aligned and a stream's descriptor rows start on 32 bytes), the points'
        // positions through the new map as it is staged for the map update
        const int np = min(SS_ROWS, n - k0);
        const uint32_t* sk = reinterpret_cast<const uint32_t*>(A.stage + H->kps) + (long long)KP_WORDS * k0;
        uint32_t* dk = reinterpret_cast<uint32_t*>(A.last_kps + o + k0);
        const uint4* sd = reinterpret_cast<const uint4*>(A.stage + H->desc) + 2LL * k0;
        uint4* dd = reinterpret_cast<uint4*>(A.last_desc + (o + k0) * 32);
        const uint4 d0 = sd[min(t, 2 * np - 1)], d1 = sd[min(t + SS_ROWS, 2 * np - 1)];
        const int r = min(t, np - 1);
        const int mp = reinterpret_cast<const int32_t*>(A.stage + H->kp2mp)[k0 + r];
        const int nnew = MH->nmp1 - MH->nmp0;
        const gf_map_point* P = reinterpret_cast<const gf_map_point*>(A.mu_stage + MH->new_mp);
        const bool on = mp >= 0 && mp < nnew;  // the host has checked the range
        float3 pos = make_float3(0.f, 0.f, 0.f);
        if (on) pos = make_float3(P[mp].pos[0], P[mp].pos[1], P[mp].pos[2]);
        for (int w = t; w < KP_WORDS * np; w += SS_ROWS) dk[w] = sk[w];
        if (t < 2 * np) dd[t] = d0;
        if (t + SS_ROWS < 2 * np) dd[t + SS_ROWS] = d1;
        if (t < np) {
            const long long i = o + k0 + t;
            A.last_kp2mp[i] = on ? mp : -1;
            A.last_outl[i] = 0;
            float* p = A.last_pos + 3 * i;
            p[0] = pos.x;
            p[1] = pos.y;
            p[2] = pos.z;
        }
    }
    if (blockIdx.x != 0) return;
    // the stream's words: chunk 0 alone writes them
    if (t < 16) A.Tcw_last[16 * (long long)b + t] = H->Tcw[t];
    if (t < 13) {  // kinematic[0..1].Xv and mCurrentInfoMat as gf_frontend_create leaves them
        A.Xv[13 * (long long)b + t] = 0.0;
        A.Xv_next[13 * (long long)b + t] = 0.0;
    }
    if (t < 49) A.base[49 * (long long)b + t] = 0.0;
    if (A.rkf && t < RKF_WORDS)  // mnRelocQuery / mnRelocWords of keyframes no query has touched
        reinterpret_cast<uint32_t*>(A.rkf + (long long)b * gf::RL_NC)[t] = 0u;
    if (t != 0) return;
    A.last_nkp[b] = n;
    A.t_prev[b] = H->timestamp;
    A.t_cur[b] = H->timestamp;
    int32_t* T = A.track + (long long)b * GF_TR_N;
    T[GF_TR_STATE] = 0;
    T[GF_TR_VEL] = 0;  // mVelocity is empty after the initialiser: the next step takes TrackPreviousFrame
    T[GF_TR_SINCE] = H->since_reloc;
    T[GF_TR_PATH] = 2;
    T[GF_TR_QUERY] = H->frame_id;
    T[GF_TR_OK] = 1;
    T[GF_TR_FORCE] = 0;  // a pending ForceRelocalisation belonged to the old map
    T[GF_TR_FORCE_KF] = 0;
    if (A.kf_state) {
        int32_t* S = A.kf_state + (long long)b * GF_KF_N;
        S[GF_KF_SINCE] = 0;    // mnLastKeyFrameId = mCurrentFrame.mnId (:1309)
        S[GF_KF_PENDING] = 0;  // RequestReset empties mlNewKeyFrames: an untaken keyframe of the old map is dropped
        S[GF_KF_ABORT] = 0;
        S[GF_KF_DECISION] = 0;
        S[GF_KF_REF] = H->ref_kf;
    }
    A.ref_kf[b] = H->ref_kf;  // mpReferenceKF = pKFcur (:1315)
    A.nleft[b] = 0;           // mLeftMapPoints named points of the old map
    A.nlist[b] = 0;
    A.st_nleft[b] = 0;
    // the map is empty until the map update's kernels have appended the new one
    A.nmp[b] = 0;
    A.kfc[b] = 0;
    A.covis[b].nkf = 0;
    A.covis[b].nmp = 0;
    if (A.ncand) A.ncand[b] = 0;  // candidates named keyframes of the old database
    if (H->clear_db) {            // KeyFrameDatabase::clear: no keyframes, no words; the arrays stay where they are
        H->db_rec->nkf = 0;
        H->db_rec->nw = 0;
        A.fe_rec[b].nkf = 0;
        A.fe_rec[b].nw = 0;
    }
}

// Tracking::ForceRelocalisation (Tracking.cc:4035-4045) for the streams a call
// names: one thread per request. last_kf -1 is the newest keyframe of the graph
// that is not bad (the newest one when all are). The host has checked the
// streams (distinct, in range, a graph with keyframes) and last_kf's range.
__global__ __launch_bounds__(64) void k_force_reloc(gf::ForceRelocArgs A) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= A.n) return;
    const int b = A.stage[2 * i];
    int kf = A.stage[2 * i + 1];
    if (b < 0 || b >= A.B) return;
    const int nkf = A.covis[b].nkf;
    if (kf < 0) {
        const uint8_t* bad = A.covis[b].kf_bad;
        kf = nkf - 1;
        for (int k = nkf - 1; k >= 0; k--)
            if (!bad[k]) {
                kf = k;
                break;
            }
    }
    if (kf < 0 || kf >= nkf) return;  // not reached: the mirrors the host checked against follow the device
    int32_t* T = A.track + (long long)b * GF_TR_N;
    T[GF_TR_FORCE] = 1;
    T[GF_TR_FORCE_KF] = kf;
    T[GF_TR_SINCE] = 0;  // mnLastRelocFrameId = mCurrentFrame.mnId (:4044)
}

}  // namespace

namespace gf {

int force_reloc_launch(gf_ctx* ctx, const ForceRelocArgs& a, hipStream_t s) {
    if (a.n <= 0) return GF_OK;
    GF_PROF(ctx, s, "k_force_reloc");
    GF_LAUNCH(k_force_reloc, (a.n + 63) / 64, 64, 0, s, a);
    GF_HIP(hipGetLastError());
    return GF_OK;
}

int stream_start_launch(gf_ctx* ctx, const StreamStartArgs& a, hipStream_t s) {
    GF_PROF(ctx, s, "k_ss_install");
    GF_LAUNCH(k_ss_install, dim3((a.cap + SS_ROWS - 1) / SS_ROWS, a.L), SS_ROWS, 0, s, a);
    GF_HIP(hipGetLastError());
    return GF_OK;
}

}  // namespace gf
