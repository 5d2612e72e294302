// Tracking::CreateInitialMap on gfx950 (src/Tracking.cc:1199-1322, with the
// filter of Tracking::Initialize :1126-1133 in front): the initialiser's
// output becomes a two-keyframe map, for a batch of independent problems, in
// two stages around the bundle adjustment (ba.hip, Optimizer.cc:36-142).
//
//   k_initmap_points  one workgroup per problem. The matches with
//                     matches12[i] >= 0 && triangulated[i] become the map
//                     points 0..n-1 in increasing i: 256 consecutive indices
//                     a round, numbered by wave64 ballots and a prefix over
//                     the four wave totals, so the ids do not depend on the
//                     wave split. Per point: its keypoint pair, position,
//                     descriptor (KFini's row), UpdateNormalAndDepth over
//                     the two observations, both slot tables (atomicMax: the
//                     later i owns a contested KFcur slot, as AddMapPoint
//                     overwrites) and the point's two edges of the
//                     gf_ba_problem.
//   k_initmap_finish  one workgroup per problem, reading the solver's output
//                     in place: UpdateNormalAndDepth of every point
//                     (Optimizer.cc:139), ComputeSceneMedianDepth(2) of KFini
//                     by the exact radix select of depthselect.h,
//                     TrackedMapPoints of KFcur, the reset tests and the
//                     scaling of the baseline and the points (:1268-1299).
//
// Every lane loads its inputs at clamped indices before the first test, so a
// round is two memory round trips (index, then the rows it names) and no load
// sits behind a branch. Arithmetic: float, -ffp-contract=off; the OpenCV
// readings are docs/ORACLE_ASSUMPTIONS.md A22 / A33. Parity: bit-exact against
// tests/helpers/initmap_ref.cpp.
#include "depthselect.h"
#include "match_common.h"
#include "normaldepth.h"

namespace {

constexpr int IM_T = 256;  // threads of both kernels: four waves
constexpr int IM_W = IM_T / 64;

struct ImConst {
    float fx, fy, cx, cy;
    float sf;  // mfScaleFactor
    int nlevels;
    float scales[16];      // mvScaleFactors
    float inv_sigma2[16];  // mvInvLevelSigma2
};

struct ImKp {  // what the stages read of a cv::KeyPoint
    float x, y;
    int octave;
};

__device__ __forceinline__ ImKp load_kp(const gf_keypoint* k) {
    ImKp r;
    r.x = gfd::ldg(&k->x);
    r.y = gfd::ldg(&k->y);
    r.octave = gfd::ldg(&k->octave);
    return r;
}

__device__ __forceinline__ void pose_of(const gf_init_result* r, float* T) {  // [R21 | t21; 0 0 0 1]
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) T[4 * i + j] = r->R21[3 * i + j];
        T[4 * i + 3] = r->t21[i];
    }
    T[12] = T[13] = T[14] = 0.f;
    T[15] = 1.f;
}

__global__ __launch_bounds__(IM_T) void k_initmap_points(ImConst C, gf_initmap_in in, gf_initmap_points out) {
    __shared__ int s_wave[IM_W];
    __shared__ int s_base;
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int cap1 = in.cap1, cap2 = in.cap2;
    const int n1 = max(0, min(in.n1[p], cap1)), n2 = max(0, min(in.n2[p], cap2));
    const gf_init_result* R = in.init + p;
    const bool ok = R->ok != 0;
    const gf_keypoint* kps1 = in.kps1 + (size_t)p * cap1;
    const gf_keypoint* kps2 = in.kps2 + (size_t)p * cap2;
    const uint32_t* desc1 = (const uint32_t*)(in.desc1 + (size_t)p * cap1 * 32);
    const int32_t* m12 = in.matches12 + (size_t)p * cap1;
    const float* p3d = in.p3d + (size_t)p * cap1 * 3;
    const uint8_t* tri = in.triangulated + (size_t)p * cap1;
    int32_t* slots1 = out.slots1 + (size_t)p * cap1;
    int32_t* slots2 = out.slots2 + (size_t)p * cap2;
    for (int i = tid; i < cap1; i += IM_T) slots1[i] = -1;
    for (int i = tid; i < cap2; i += IM_T) slots2[i] = -1;
    if (tid == 0) s_base = 0;
    // the two keyframes of the gf_ba_problem: KFini identity and fixed (mnId 0), KFcur at [R21 | t21]
    float T1[16];
    pose_of(R, T1);
    if (tid < 32) {
        const int k = tid >> 4, q = tid & 15;
        out.kf_Tcw[(size_t)p * 32 + tid] = (k == 0 || !ok) ? ((q & 3) == (q >> 2) ? 1.f : 0.f) : T1[q];
    } else if (tid < 34) {
        out.kf_kind[(size_t)p * 2 + (tid - 32)] = tid == 32 ? 1 : 0;
    } else if (tid >= 64 && tid < 72) {
        const int q = (tid - 64) & 3;
        out.kf_cam[(size_t)p * 8 + (tid - 64)] = q == 0 ? C.fx : q == 1 ? C.fy : q == 2 ? C.cx : C.cy;
    }
    const float I16[12] = {1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f};
    float Ow0[3], Ow1[3];
    gfnd::camera_center(I16, Ow0);
    gfnd::camera_center(T1, Ow1);
    __syncthreads();  // the cleared slot tables before the first atomicMax
    if (!ok) {
        if (tid == 0) {
            out.npts[p] = 0;
            out.status[p] = GF_IM_NOT_INITIALIZED;
        }
        return;
    }
    for (int i0 = 0; i0 < n1; i0 += IM_T) {
        const int i = i0 + tid, ic = min(i, n1 - 1);
        // round trip 1: the match and everything indexed by i
        const int i2 = gfd::ldg(m12 + ic);
        const uint8_t t = gfd::ldg(tri + ic);
        const ImKp k1 = load_kp(kps1 + ic);
        const float X[3] = {gfd::ldg(p3d + 3 * ic), gfd::ldg(p3d + 3 * ic + 1), gfd::ldg(p3d + 3 * ic + 2)};
        uint32_t d[8];
#pragma unroll
        for (int q = 0; q < 8; q++) d[q] = gfd::ldg(desc1 + (size_t)ic * 8 + q);
        // round trip 2: the KFcur keypoint (a match outside the frame is no match)
        const bool take = i < n1 && i2 >= 0 && i2 < n2 && t;
        const ImKp k2 = load_kp(kps2 + (take ? i2 : 0));  // cap2 >= 1: row 0 exists
        // ordered compaction: ballot inside the wave, prefix over the wave totals
        const unsigned long long bal = __ballot(take);
        const int below = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) s_wave[w] = __popcll(bal);
        __syncthreads();
        int off = s_base, total = 0;
#pragma unroll
        for (int q = 0; q < IM_W; q++) {
            if (q < w) off += s_wave[q];
            total += s_wave[q];
        }
        if (take) {
            const int j = off + below;  // the point's id
            out.pt_kp[((size_t)p * cap1 + j) * 2] = i;
            out.pt_kp[((size_t)p * cap1 + j) * 2 + 1] = i2;
            uint32_t* dd = (uint32_t*)(out.mp_desc + ((size_t)p * cap1 + j) * 32);
#pragma unroll
            for (int q = 0; q < 8; q++) dd[q] = d[q];
            // UpdateNormalAndDepth: observations KFini, KFcur (A26); mpRefKF = pKFcur
            const int lv = min(max(k2.octave, 0), C.nlevels - 1);
            float nr[3] = {0.f, 0.f, 0.f};
            gfnd::add_view(X, Ow0, nr);
            gfnd::add_view(X, Ow1, nr);
            gf_map_point mp;
            gfnd::finish(X, Ow1, nr, 2, C.sf, C.scales[lv], C.scales[C.nlevels - 1 - lv], mp.normal, mp.min_dist,
                         mp.max_dist);
#pragma unroll
            for (int c = 0; c < 3; c++) {
                mp.pos[c] = X[c];
                out.pt_pos[((size_t)p * cap1 + j) * 3 + c] = X[c];
            }
            out.mps[(size_t)p * cap1 + j] = mp;
            slots1[i] = j;
            atomicMax(slots2 + i2, j);  // ids grow with i: the later AddMapPoint owns the slot
            const size_t e = (size_t)p * 2 * cap1 + 2 * (size_t)j;
            out.edge_pt[e] = j;
            out.edge_pt[e + 1] = j;
            out.edge_kf[e] = 0;
            out.edge_kf[e + 1] = 1;
            out.edge_z[2 * e] = k1.x;
            out.edge_z[2 * e + 1] = k1.y;
            out.edge_z[2 * e + 2] = k2.x;
            out.edge_z[2 * e + 3] = k2.y;
            out.edge_inv_sigma2[e] = C.inv_sigma2[min(max(k1.octave, 0), C.nlevels - 1)];
            out.edge_inv_sigma2[e + 1] = C.inv_sigma2[lv];
        }
        __syncthreads();  // s_wave and s_base are read by everyone before the next round writes them
        if (tid == 0) s_base = off + total;  // w == 0: off is the base of this round
        __syncthreads();
    }
    if (tid == 0) {
        out.npts[p] = s_base;
        out.status[p] = GF_IM_OK;
    }
}

__global__ __launch_bounds__(IM_T) void k_initmap_finish(ImConst C, gf_initmap_in in, gf_initmap_points pts,
                                                         const float* const* __restrict__ ba_Tcw,
                                                         const float* const* __restrict__ ba_pos,
                                                         const int32_t* const* __restrict__ ba_iters, int thres,
                                                         gf_initmap_report* __restrict__ rep,
                                                         gf_map_point* __restrict__ mps_out) {
    __shared__ uint32_t keys[KP_MAX];
    __shared__ int hist[256];
    __shared__ uint32_t s_prefix;
    __shared__ int s_rank, s_tracked;
    const int p = blockIdx.x, tid = threadIdx.x;
    const int cap1 = in.cap1, cap2 = in.cap2;
    const int n2 = max(0, min(in.n2[p], cap2));
    const int npts = max(0, min(pts.npts[p], min(cap1, KP_MAX)));
    const int st0 = pts.status[p];
    const gf_keypoint* kps2 = in.kps2 + (size_t)p * cap2;
    const int32_t* slots2 = pts.slots2 + (size_t)p * cap2;
    const int32_t* pt_kp = pts.pt_kp + (size_t)p * cap1 * 2;
    gf_map_point* mo = mps_out + (size_t)p * cap1;
    if (tid == 0) s_tracked = 0;
    __syncthreads();
    gf_initmap_report Rp;
    Rp.status = st0;
    Rp.npts = npts;
    Rp.tracked = 0;
    Rp.ba_iterations = -1;
    Rp.median_depth = 0.f;
    for (int q = 0; q < 32; q++) Rp.Tcw[q] = pts.kf_Tcw[(size_t)p * 32 + q];
    if (st0 == GF_IM_NOT_INITIALIZED) {
        if (tid == 0) rep[p] = Rp;
        return;
    }
    // the optimised poses (Optimizer.cc:125-131); a problem the solver had nothing to do on returns its inputs
    const float* T = ba_Tcw[p];
    const float* Xs = ba_pos[p];
    if (ba_iters) Rp.ba_iterations = *ba_iters[p];
    for (int q = 0; q < 32; q++) Rp.Tcw[q] = T[q];
    const float* T0 = Rp.Tcw;
    const float* T1 = Rp.Tcw + 16;
    float Ow0[3], Ow1[3];
    gfnd::camera_center(T0, Ow0);
    gfnd::camera_center(T1, Ow1);
    // TrackedMapPoints of KFcur: its non-NULL slots
    int cnt = 0;
    for (int i = tid; i < n2; i += IM_T) cnt += slots2[i] >= 0;
    cnt = gfd::warp_sum(cnt);
    if ((tid & 63) == 0 && cnt) atomicAdd(&s_tracked, cnt);
    // UpdateNormalAndDepth of every point (Optimizer.cc:139) and its depth in KFini: every KFini slot holds
    // its own point, so the non-NULL slots of KFini are the points
    for (int j = tid; j < npts; j += IM_T) {
        const int i2 = pt_kp[2 * j + 1];
        const float X[3] = {Xs[3 * j], Xs[3 * j + 1], Xs[3 * j + 2]};
        const int oct = gfd::ldg(&kps2[min(max(i2, 0), max(n2 - 1, 0))].octave);
        const int lv = min(max(oct, 0), C.nlevels - 1);
        float nr[3] = {0.f, 0.f, 0.f};
        gfnd::add_view(X, Ow0, nr);
        gfnd::add_view(X, Ow1, nr);
        gf_map_point mp;
        gfnd::finish(X, Ow1, nr, 2, C.sf, C.scales[lv], C.scales[C.nlevels - 1 - lv], mp.normal, mp.min_dist,
                     mp.max_dist);
        for (int c = 0; c < 3; c++) mp.pos[c] = X[c];
        mo[j] = mp;
        keys[j] = gfcv::ord_key(gfsel::scene_depth(T0, X));
    }
    __syncthreads();
    float median = 0.f;
    if (npts > 0) median = gfcv::key_val(gfsel::radix_select<IM_T>(keys, npts, (npts - 1) / 2, hist, &s_prefix, &s_rank));
    const int tracked = s_tracked;
    // :1269; with no point the reference indexes an empty vector: defined as too few (A33)
    int st = GF_IM_OK;
    if (npts == 0) st = GF_IM_RESET_FEW;
    else if (median < 0.f) st = GF_IM_RESET_DEPTH;
    else if (tracked < thres) st = GF_IM_RESET_FEW;
    Rp.status = st;
    Rp.tracked = tracked;
    Rp.median_depth = median;
    if (st == GF_IM_OK) {
        // :1282-1299: Mat * scalar is one float product per element (A33); the normals and distances stay
        // those of the unscaled result
        const float inv = 1.0f / median;
        for (int c = 0; c < 3; c++) Rp.Tcw[16 + 4 * c + 3] = Rp.Tcw[16 + 4 * c + 3] * inv;
        for (int j = tid; j < npts; j += IM_T)
            for (int c = 0; c < 3; c++) mo[j].pos[c] = Xs[3 * j + c] * inv;
    }
    if (tid == 0) rep[p] = Rp;
}

int im_const(const gf_frame_info* fi, ImConst* C) {
    GF_CHECK(fi->nlevels >= 1 && fi->nlevels <= 16, GF_ERR_ARG, "nlevels out of range");
    const FrameConst fc = gf::make_frame_const(fi);
    C->fx = fi->fx;
    C->fy = fi->fy;
    C->cx = fi->cx;
    C->cy = fi->cy;
    C->sf = fi->scale_factor;
    C->nlevels = fi->nlevels;
    for (int l = 0; l < 16; l++) {
        C->scales[l] = l < fi->nlevels ? fc.scales[l] : 1.f;
        C->inv_sigma2[l] = 1.0f / (C->scales[l] * C->scales[l]);  // 1 / mvLevelSigma2 (ORBextractor.cc:443-452)
    }
    return GF_OK;
}

int im_check_in(const gf_initmap_in* in) {
    GF_CHECK(in->cap1 >= 1 && in->cap1 <= KP_MAX && in->cap2 >= 1 && in->cap2 <= KP_MAX, GF_ERR_UNSUPPORTED,
             "a frame holds 1 to 4096 keypoints");
    GF_CHECK(in->kps1 && in->desc1 && in->n1 && in->kps2 && in->desc2 && in->n2 && in->matches12 && in->init &&
                 in->p3d && in->triangulated,
             GF_ERR_ARG, "null input buffer");
    GF_CHECK(((uintptr_t)in->desc1 & 3) == 0, GF_ERR_ARG, "descriptors must be 4-byte aligned");
    return GF_OK;
}

int im_check_pts(const gf_initmap_points* o) {
    GF_CHECK(o->status && o->npts && o->pt_kp && o->mps && o->mp_desc && o->slots1 && o->slots2 && o->kf_Tcw &&
                 o->kf_kind && o->kf_cam && o->pt_pos && o->edge_pt && o->edge_kf && o->edge_z && o->edge_inv_sigma2,
             GF_ERR_ARG, "null output buffer");
    GF_CHECK(((uintptr_t)o->mp_desc & 3) == 0, GF_ERR_ARG, "descriptors must be 4-byte aligned");
    return GF_OK;
}

}  // namespace

extern "C" {

int gf_initial_map_points_dev(gf_ctx* ctx, const gf_frame_info* fi, int nprob, const gf_initmap_in* in,
                              const gf_initmap_points* out, void* stream) {
    GF_CHECK(ctx && fi && in && out, GF_ERR_ARG, "gf_initial_map_points_dev: null arg");
    if (nprob <= 0) return GF_OK;
    ImConst C;
    int rc = im_const(fi, &C);
    if (rc || (rc = im_check_in(in)) || (rc = im_check_pts(out))) return rc;
    GF_HIP(hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    GF_PROF(ctx, s, "k_initmap_points");
    GF_LAUNCH(k_initmap_points, nprob, IM_T, 0, s, C, *in, *out);
    GF_HIP(hipGetLastError());
    return GF_OK;
}

int gf_initial_map_finish_dev(gf_ctx* ctx, const gf_frame_info* fi, int nprob, const gf_initmap_in* in,
                              const gf_initmap_points* pts, const float* const* d_ba_kf_Tcw,
                              const float* const* d_ba_pt_pos, const int32_t* const* d_ba_iterations,
                              int thres_init_mpt_num,
                              gf_initmap_report* d_report, gf_map_point* d_mps, void* stream) {
    GF_CHECK(ctx && fi && in && pts, GF_ERR_ARG, "gf_initial_map_finish_dev: null arg");
    if (nprob <= 0) return GF_OK;
    GF_CHECK(d_ba_kf_Tcw && d_ba_pt_pos && d_report && d_mps, GF_ERR_ARG, "gf_initial_map_finish_dev: null buffer");
    ImConst C;
    int rc = im_const(fi, &C);
    if (rc || (rc = im_check_in(in)) || (rc = im_check_pts(pts))) return rc;
    GF_HIP(hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    GF_PROF(ctx, s, "k_initmap_finish");
    GF_LAUNCH(k_initmap_finish, nprob, IM_T, 0, s, C, *in, *pts, d_ba_kf_Tcw, d_ba_pt_pos, d_ba_iterations,
              thres_init_mpt_num, d_report, d_mps);
    GF_HIP(hipGetLastError());
    return GF_OK;
}

}  // extern "C"
