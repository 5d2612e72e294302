// The device side of LocalMapping::SearchInNeighbors (src/LocalMapping.cc:411-488):
//
//   k_fuse_search: ORBmatcher::Fuse(pKF, vpMapPoints, th) (src/ORBmatcher.cc:
//     1607-1687) up to the choice of bestIdx, for many (keyframe, candidate-id
//     list) problems in one launch against the whole-map arrays. The candidate
//     body is k_fuse's pass 1 (lmap.hip); the grid is k_fuse_sim3's (problem,
//     chunk of candidates) workgroups. The add / replace / keep decision of
//     :1690-1703 reads the live map and stays with the caller
//     (gf_orb_slam_amd/localmapping.py: search_in_neighbors).
//
//   k_update_normal_and_depth: MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:
//     285-324) for many points, one lane per point, its observations walked in
//     observation-map order so the float sum keeps the reference's order.
#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

#include "match_common.h"
#include "normaldepth.h"

#define NS_THREADS 256
#define NS_TH_LOW 50

namespace {

struct FuseSearchProb {
    float T[12];  // Rcw | tcw, row-major 3x4
    float Ow[3];
    float th;
    const gf_keypoint* kps;
    const uint8_t* desc;
    const int32_t* points;
    const uint8_t* skip;
    gf_fuse_search_result* res;
    int32_t n, m;
};

// one workgroup: candidates [first, min(first + chunk, m)) of problem prob
struct FuseSearchBlock {
    int32_t prob, first;
};

__global__ __launch_bounds__(NS_THREADS) void k_fuse_search(FrameConst fc, const FuseSearchProb* __restrict__ probs,
                                                            const FuseSearchBlock* __restrict__ blocks, int chunk,
                                                            const gf_map_point* __restrict__ mps,
                                                            const uint8_t* __restrict__ mp_desc,
                                                            const uint8_t* __restrict__ mp_bad, int nmp) {
    extern __shared__ int lds[];
    const FuseSearchBlock B = blocks[blockIdx.x];
    const FuseSearchProb& P = probs[B.prob];
    const int n = P.n, tid = threadIdx.x;
    const int last = min(B.first + chunk, P.m);
    if (n == 0) {  // GetFeaturesInArea is empty for every candidate (:1661)
        for (int i = B.first + tid; i < last; i += NS_THREADS) P.res[i] = gf_fuse_search_result{-1, -1};
        return;
    }
    int* cell_start = lds;                 // NCELLS + 1
    int* items = cell_start + NCELLS + 1;  // n
    // no slot table takes part in the search (occupancy is read after bestIdx is chosen)
    build_grid_only(fc, P.kps, n, cell_start, items, items + n, NS_THREADS);
    const int nmax = fc.nlevels - 1;
    for (int i = B.first + tid; i < last; i += NS_THREADS) {
        int bestIdx = -1, bestDist = INT_MAX;
        do {
            const int id = P.points[i];
            if (id < 0 || id >= nmp) break;  // NULL (:1611)
            // the point's row, its descriptor and its flags are in flight before the first exit
            const gf_map_point mp = mps[id];
            const uint4* dq = (const uint4*)(mp_desc + (size_t)id * 32);
            const uint4 a0 = dq[0], a1 = dq[1];
            const bool bad = mp_bad && mp_bad[id];
            const bool skip = P.skip && P.skip[i];
            if (bad || skip) break;  // isBad() || IsInKeyFrame(pKF) (:1614)
            float Pc[3];
            transform3(P.T, mp.pos, Pc);
            if (Pc[2] < 0.0f) break;
            const float invz = 1.f / Pc[2];
            const float x = Pc[0] * invz, y = Pc[1] * invz;
            const float u = fc.fx * x + fc.cx, v = fc.fy * y + fc.cy;
            // KeyFrame::IsInImage (KeyFrame.cc:654-657)
            if (!(u >= (float)fc.min_x && u < (float)fc.max_x && v >= (float)fc.min_y && v < (float)fc.max_y)) break;
            const float PO[3] = {mp.pos[0] - P.Ow[0], mp.pos[1] - P.Ow[1], mp.pos[2] - P.Ow[2]};
            // cv::norm / Mat::dot accumulate in double
            const float dist3D = (float)sqrt((double)PO[0] * PO[0] + (double)PO[1] * PO[1] + (double)PO[2] * PO[2]);
            if (dist3D < mp.min_dist || dist3D > mp.max_dist) break;
            const double dot = (double)PO[0] * mp.normal[0] + (double)PO[1] * mp.normal[1] + (double)PO[2] * mp.normal[2];
            if (dot < 0.5 * (double)dist3D) break;
            const float ratio = dist3D / mp.min_dist;
            int lvl = 0;
            while (lvl < fc.nlevels && fc.scales[lvl] < ratio) lvl++;  // lower_bound
            lvl = min(lvl, nmax);
            const float r = P.th * fc.scales[lvl];
            int cx0, cx1, cy0, cy1;
            if (!grid_window(fc, u, v, r, cx0, cx1, cy0, cy1)) break;
            for (int cx = cx0; cx <= cx1; cx++)
                for (int cy = cy0; cy <= cy1; cy++) {
                    const int c = cx * GRID_ROWS + cy;
                    for (int a = cell_start[c], e = cell_start[c + 1]; a < e; a++) {
                        const int idx = items[a];
                        const gf_keypoint kp = P.kps[idx];
                        const uint4* dk = (const uint4*)(P.desc + (size_t)idx * 32);
                        const uint4 b0 = dk[0], b1 = dk[1];
                        if (fabsf(kp.x - u) > r || fabsf(kp.y - v) > r) continue;
                        if (kp.octave < lvl - 1 || kp.octave > lvl) continue;
                        const int d = hamming_regs(a0, a1, b0, b1);
                        if (d < bestDist) {
                            bestDist = d;
                            bestIdx = idx;
                        }
                    }
                }
        } while (false);
        const bool fused = bestDist <= NS_TH_LOW;
        P.res[i] = gf_fuse_search_result{fused ? bestIdx : -1, fused ? bestDist : -1};
    }
}

__global__ __launch_bounds__(256) void k_update_normal_and_depth(
    int npts, const float* __restrict__ pos, const int32_t* __restrict__ offs, const int32_t* __restrict__ obs_kf,
    const float* __restrict__ kf_Ow, int nkf, const int32_t* __restrict__ ref_kf,
    const int32_t* __restrict__ ref_level, float sf, FrameConst fc, float* __restrict__ normal,
    float* __restrict__ min_dist, float* __restrict__ max_dist) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= npts) return;
    const int a = offs[p], e = offs[p + 1], ref = ref_kf[p], level = ref_level[p];
    // no observations or no reference keyframe: the reference divides by zero, the point is left as it is
    if (e <= a || ref < 0 || ref >= nkf || level < 0 || level >= fc.nlevels) return;
    const float X[3] = {pos[3 * p], pos[3 * p + 1], pos[3 * p + 2]};
    float nr[3] = {0.f, 0.f, 0.f};
    for (int o = a; o < e; o++) {  // observation-map order (:302-309)
        const int kf = obs_kf[o];
        if (kf < 0 || kf >= nkf) return;
        gfnd::add_view(X, kf_Ow + 3 * kf, nr);
    }
    float nm[3], mn, mx;
    gfnd::finish(X, kf_Ow + 3 * ref, nr, e - a, sf, fc.scales[level], fc.scales[fc.nlevels - 1 - level], nm, mn, mx);
    min_dist[p] = mn;
    max_dist[p] = mx;
#pragma unroll
    for (int c = 0; c < 3; c++) normal[3 * p + c] = nm[c];
}

}  // namespace

extern "C" {

int gf_fuse_search_set_chunk(gf_ctx* ctx, int chunk) {
    GF_CHECK(ctx, GF_ERR_ARG, "gf_fuse_search_set_chunk: null ctx");
    GF_CHECK(chunk >= 64 && chunk <= (1 << 16), GF_ERR_ARG, "chunk outside [64, 65536]");
    ctx->fuse_search_chunk = chunk;
    return GF_OK;
}

int gf_fuse_search_dev(gf_ctx* ctx, const gf_frame_info* fi, int nprob, const gf_fuse_search_problem* probs,
                       const gf_map_point* d_mps, const uint8_t* d_mp_desc, const uint8_t* d_mp_bad, int nmp,
                       void* stream) {
    GF_CHECK(ctx && fi, GF_ERR_ARG, "gf_fuse_search_dev: null arg");
    if (nprob <= 0) return GF_OK;
    GF_CHECK(probs, GF_ERR_ARG, "gf_fuse_search_dev: null problems");
    GF_CHECK(fi->nlevels >= 1 && fi->nlevels <= 16, GF_ERR_ARG, "nlevels out of range");
    GF_CHECK(fi->max_x > fi->min_x && fi->max_y > fi->min_y, GF_ERR_ARG, "empty image bounds");
    GF_CHECK(nmp >= 0, GF_ERR_ARG, "nmp < 0");
    const int chunk = ctx->fuse_search_chunk;
    std::vector<FuseSearchProb> P(nprob);
    std::vector<FuseSearchBlock> B;
    int nmax = 0;
    for (int p = 0; p < nprob; p++) {
        const gf_fuse_search_problem& q = probs[p];
        GF_CHECK(q.n >= 0 && q.n <= KP_MAX, GF_ERR_UNSUPPORTED, "at most 4096 keyframe keypoints");
        GF_CHECK(q.npoints >= 0, GF_ERR_ARG, "negative candidate count");
        GF_CHECK(q.npoints == 0 || (q.points && q.res), GF_ERR_ARG, "gf_fuse_search_dev: null candidate list or result");
        GF_CHECK(q.npoints == 0 || q.n == 0 || (q.kps && q.desc && d_mps && d_mp_desc && nmp > 0), GF_ERR_ARG,
                 "gf_fuse_search_dev: null keyframe or map buffer");
        for (int k = 0; k < 12; k++) P[p].T[k] = q.Tcw[k];
        for (int k = 0; k < 3; k++) P[p].Ow[k] = q.Ow[k];
        P[p].th = q.th;
        P[p].kps = q.kps;
        P[p].desc = q.desc;
        P[p].points = q.points;
        P[p].skip = q.skip;
        P[p].res = q.res;
        P[p].n = q.n;
        P[p].m = q.npoints;
        for (int first = 0; first < q.npoints; first += chunk) B.push_back(FuseSearchBlock{p, first});
        if (q.npoints) nmax = std::max(nmax, q.n);
    }
    if (B.empty()) return GF_OK;
    hipStream_t s = (hipStream_t)stream;
    // one scratch block: [problems | workgroup table]
    const size_t pb = (sizeof(FuseSearchProb) * (size_t)nprob + 15) & ~(size_t)15, bb = sizeof(FuseSearchBlock) * B.size();
    void* dp;
    int rc = gf::ws_get(ctx, 66, pb + bb, &dp);
    if (rc) return rc;
    GF_HIP(hipMemcpyAsync(dp, P.data(), sizeof(FuseSearchProb) * (size_t)nprob, hipMemcpyHostToDevice, s));
    GF_HIP(hipMemcpyAsync((char*)dp + pb, B.data(), bb, hipMemcpyHostToDevice, s));
    GF_PROF(ctx, s, "k_fuse_search");
    GF_LAUNCH(k_fuse_search, (int)B.size(), NS_THREADS, sizeof(int) * ((size_t)NCELLS + 1 + 2 * (size_t)nmax), s,
              gf::make_frame_const(fi), (const FuseSearchProb*)dp, (const FuseSearchBlock*)((char*)dp + pb), chunk, d_mps,
              d_mp_desc, d_mp_bad, nmp);
    GF_HIP(hipGetLastError());
    return GF_OK;
}

int gf_fuse_search(gf_ctx* ctx, const gf_frame_info* fi, const float* Tcw, const float* Ow, const gf_keypoint* kps,
                   const uint8_t* desc, int n, const gf_map_point* mps, const uint8_t* mp_desc, const uint8_t* mp_bad,
                   int nmp, const int32_t* points, const uint8_t* skip, int npoints, float th,
                   gf_fuse_search_result* res) {
    GF_CHECK(ctx && fi && Tcw && Ow, GF_ERR_ARG, "gf_fuse_search: null arg");
    GF_CHECK(n >= 0 && n <= KP_MAX, GF_ERR_UNSUPPORTED, "at most 4096 keyframe keypoints");
    GF_CHECK(nmp >= 0 && npoints >= 0, GF_ERR_ARG, "negative count");
    if (npoints == 0) return GF_OK;
    GF_CHECK(points && res && (nmp == 0 || (mps && mp_desc)) && (n == 0 || (kps && desc)), GF_ERR_ARG,
             "gf_fuse_search: null buffer");
    if (nmp == 0) {  // every id is outside the map
        for (int i = 0; i < npoints; i++) res[i] = gf_fuse_search_result{-1, -1};
        return GF_OK;
    }
    GF_HIP(hipSetDevice(ctx->device));
    // one scratch block: [kps | desc | mps | mp_desc | bad | points | skip | res]
    size_t off = 0;
    std::vector<std::pair<const void*, size_t>> parts;
    auto add = [&](const void* h, size_t bytes) {
        const size_t o = off;
        parts.push_back({h, bytes});
        off += (bytes + 15) & ~(size_t)15;
        return o;
    };
    const size_t o_k = add(kps, sizeof(gf_keypoint) * (size_t)n), o_d = add(desc, 32 * (size_t)n),
                 o_mp = add(mps, sizeof(gf_map_point) * (size_t)nmp),
                 o_md = add(mp_desc, 32 * (size_t)nmp), o_bad = add(mp_bad, mp_bad ? (size_t)nmp : 0),
                 o_pts = add(points, 4 * (size_t)npoints), o_sk = add(skip, skip ? (size_t)npoints : 0),
                 o_r = add(nullptr, sizeof(gf_fuse_search_result) * (size_t)npoints);
    void* dbuf;
    int rc = gf::ws_get(ctx, 67, off, &dbuf);
    if (rc) return rc;
    uint8_t* base = (uint8_t*)dbuf;
    hipStream_t s = ctx->stream;
    size_t cur = 0;
    for (auto& pr : parts) {
        if (pr.first && pr.second) GF_HIP(hipMemcpyAsync(base + cur, pr.first, pr.second, hipMemcpyHostToDevice, s));
        cur += (pr.second + 15) & ~(size_t)15;
    }
    gf_fuse_search_problem q{};
    for (int k = 0; k < 16; k++) q.Tcw[k] = Tcw[k];
    for (int k = 0; k < 3; k++) q.Ow[k] = Ow[k];
    q.th = th;
    q.kps = (const gf_keypoint*)(base + o_k);
    q.desc = base + o_d;
    q.n = n;
    q.points = (const int32_t*)(base + o_pts);
    q.skip = skip ? base + o_sk : nullptr;
    q.npoints = npoints;
    q.res = (gf_fuse_search_result*)(base + o_r);
    rc = gf_fuse_search_dev(ctx, fi, 1, &q, (const gf_map_point*)(base + o_mp), base + o_md,
                            mp_bad ? base + o_bad : nullptr, nmp, s);
    if (rc) return rc;
    GF_HIP(hipMemcpyAsync(res, base + o_r, sizeof(gf_fuse_search_result) * (size_t)npoints, hipMemcpyDeviceToHost, s));
    GF_HIP(hipStreamSynchronize(s));
    return GF_OK;
}

int gf_update_normal_and_depth_dev(gf_ctx* ctx, const gf_frame_info* fi, int npts, const float* d_pos,
                                   const int32_t* d_offsets, const int32_t* d_obs_kf, const float* d_kf_Ow, int nkf,
                                   const int32_t* d_ref_kf, const int32_t* d_ref_level, float* d_normal,
                                   float* d_min_dist, float* d_max_dist, void* stream) {
    GF_CHECK(ctx && fi, GF_ERR_ARG, "gf_update_normal_and_depth_dev: null arg");
    if (npts <= 0) return GF_OK;
    GF_CHECK(fi->nlevels >= 1 && fi->nlevels <= 16, GF_ERR_ARG, "nlevels out of range");
    GF_CHECK(nkf >= 0, GF_ERR_ARG, "nkf < 0");
    GF_CHECK(d_pos && d_offsets && d_ref_kf && d_ref_level && d_normal && d_min_dist && d_max_dist, GF_ERR_ARG,
             "gf_update_normal_and_depth_dev: null buffer");
    if (nkf == 0) return GF_OK;  // no keyframe: no point has a reference keyframe
    GF_CHECK(d_obs_kf && d_kf_Ow, GF_ERR_ARG, "gf_update_normal_and_depth_dev: null observation or centre buffer");
    hipStream_t s = (hipStream_t)stream;
    GF_PROF(ctx, s, "k_update_normal_and_depth");
    GF_LAUNCH(k_update_normal_and_depth, (npts + 255) / 256, 256, 0, s, npts, d_pos, d_offsets, d_obs_kf, d_kf_Ow, nkf,
              d_ref_kf, d_ref_level, fi->scale_factor, gf::make_frame_const(fi), d_normal, d_min_dist, d_max_dist);
    GF_HIP(hipGetLastError());
    return GF_OK;
}

int gf_update_normal_and_depth(gf_ctx* ctx, const gf_frame_info* fi, int npts, const float* pos, const int32_t* offsets,
                               const int32_t* obs_kf, const float* kf_Ow, int nkf, const int32_t* ref_kf,
                               const int32_t* ref_level, float* normal, float* min_dist, float* max_dist) {
    GF_CHECK(ctx && fi, GF_ERR_ARG, "gf_update_normal_and_depth: null arg");
    if (npts <= 0) return GF_OK;
    GF_CHECK(pos && offsets && ref_kf && ref_level && normal && min_dist && max_dist, GF_ERR_ARG,
             "gf_update_normal_and_depth: null buffer");
    GF_CHECK(nkf >= 0 && offsets[0] == 0, GF_ERR_ARG, "offsets[0] must be 0");
    for (int p = 0; p < npts; p++) {
        GF_CHECK(offsets[p + 1] >= offsets[p], GF_ERR_ARG, "offsets must be non-decreasing");
        GF_CHECK(ref_kf[p] < nkf, GF_ERR_ARG, "reference keyframe out of range");
        GF_CHECK(ref_kf[p] < 0 || (ref_level[p] >= 0 && ref_level[p] < fi->nlevels), GF_ERR_ARG,
                 "reference level out of range");
    }
    const int total = offsets[npts];
    GF_CHECK(total == 0 || (obs_kf && kf_Ow), GF_ERR_ARG, "null observations");
    for (int o = 0; o < total; o++)
        GF_CHECK(obs_kf[o] >= 0 && obs_kf[o] < nkf, GF_ERR_ARG, "observing keyframe out of range");
    if (total == 0 || nkf == 0) return GF_OK;
    GF_HIP(hipSetDevice(ctx->device));
    // one scratch block: [pos | offsets | obs_kf | kf_Ow | ref_kf | ref_level | normal | min | max]
    size_t off = 0;
    std::vector<std::pair<const void*, size_t>> parts;
    auto add = [&](const void* h, size_t bytes) {
        const size_t o = off;
        parts.push_back({h, bytes});
        off += (bytes + 15) & ~(size_t)15;
        return o;
    };
    const size_t N = (size_t)npts;
    const size_t o_p = add(pos, 12 * N), o_o = add(offsets, 4 * (N + 1)), o_k = add(obs_kf, 4 * (size_t)total),
                 o_c = add(kf_Ow, 12 * (size_t)nkf), o_r = add(ref_kf, 4 * N), o_l = add(ref_level, 4 * N),
                 o_n = add(normal, 12 * N), o_mn = add(min_dist, 4 * N), o_mx = add(max_dist, 4 * N);
    void* dbuf;
    int rc = gf::ws_get(ctx, 68, off, &dbuf);
    if (rc) return rc;
    uint8_t* base = (uint8_t*)dbuf;
    hipStream_t s = ctx->stream;
    size_t cur = 0;
    for (auto& pr : parts) {
        if (pr.second) GF_HIP(hipMemcpyAsync(base + cur, pr.first, pr.second, hipMemcpyHostToDevice, s));
        cur += (pr.second + 15) & ~(size_t)15;
    }
    rc = gf_update_normal_and_depth_dev(ctx, fi, npts, (const float*)(base + o_p), (const int32_t*)(base + o_o),
                                        (const int32_t*)(base + o_k), (const float*)(base + o_c), nkf,
                                        (const int32_t*)(base + o_r), (const int32_t*)(base + o_l),
                                        (float*)(base + o_n), (float*)(base + o_mn), (float*)(base + o_mx), s);
    if (rc) return rc;
    GF_HIP(hipMemcpyAsync(normal, base + o_n, 12 * N, hipMemcpyDeviceToHost, s));
    GF_HIP(hipMemcpyAsync(min_dist, base + o_mn, 4 * N, hipMemcpyDeviceToHost, s));
    GF_HIP(hipMemcpyAsync(max_dist, base + o_mx, 4 * N, hipMemcpyDeviceToHost, s));
    GF_HIP(hipStreamSynchronize(s));
    return GF_OK;
}

}  // extern "C"
