// The searches of LoopClosing::SearchAndFuse (src/LoopClosing.cc:572-585):
// ORBmatcher::Fuse(pKF, Scw, vpPoints, th) (src/ORBmatcher.cc:1710-1839) up to
// the choice of bestIdx, for every keyframe of CorrectedSim3 in one launch.
// The add / replace decision (:1819-1833) reads the live map and stays with the
// caller (gf_orb_slam_amd/sim3.py: search_and_fuse).
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>

#include "match_common.h"

#define FS_THREADS 256
#define FS_TH_LOW 50
#define FS_CHUNK_DEFAULT 256

namespace {

struct FuseSim3Prob {
    float T[12];  // Rcw | tcw, row-major 3x4 (Scw / scw)
    float Ow[3];
    float th;
    const gf_keypoint* kps;
    const uint8_t* desc;
    const int32_t* kf_mp;
    const int32_t* points;
    gf_fuse_sim3_result* res;
    int32_t n, m;
};

// one workgroup: candidates [first, min(first + chunk, m)) of problem prob
struct FuseSim3Block {
    int32_t prob, first;
};

__device__ __forceinline__ unsigned fs_hash(int id) { return (unsigned)id * 2654435761u; }

__global__ __launch_bounds__(FS_THREADS) void k_fuse_sim3(FrameConst fc, const FuseSim3Prob* __restrict__ probs,
                                                          const FuseSim3Block* __restrict__ blocks, int chunk,
                                                          const gf_map_point* __restrict__ mps,
                                                          const uint8_t* __restrict__ mp_desc,
                                                          const uint8_t* __restrict__ mp_bad, int nmp) {
    extern __shared__ int lds[];
    const FuseSim3Block B = blocks[blockIdx.x];
    const FuseSim3Prob& P = probs[B.prob];
    const int n = P.n, tid = threadIdx.x;
    const int last = min(B.first + chunk, P.m);
    if (n == 0) {  // GetFeaturesInArea is empty for every candidate (:1790)
        for (int i = B.first + tid; i < last; i += FS_THREADS) P.res[i] = gf_fuse_sim3_result{-1, -1};
        return;
    }
    int* cell_start = lds;                 // NCELLS + 1
    int* items = cell_start + NCELLS + 1;  // n
    int* tab = items + n;                  // 2n: build_grid's scratch, then the set spAlreadyFound
    build_grid(fc, P.kps, n, P.kf_mp, cell_start, items, tab, tab + n, FS_THREADS);
    // spAlreadyFound = pKF->GetMapPoints() (:1726): the non-bad points of the
    // slot table, as an open-addressing set of ids (load <= 1/2, -1 = free)
    const int ts = 2 * n;
    for (int k = tid; k < ts; k += FS_THREADS) tab[k] = -1;
    __syncthreads();
    for (int k = tid; k < n; k += FS_THREADS) {
        const int id = P.kf_mp[k];
        if (id < 0 || id >= nmp || (mp_bad && mp_bad[id])) continue;
        int h = (int)(fs_hash(id) % (unsigned)ts);
        while (true) {
            const int old = atomicCAS(&tab[h], -1, id);
            if (old == -1 || old == id) break;
            h = h + 1 == ts ? 0 : h + 1;
        }
    }
    __syncthreads();
    const int nmax = fc.nlevels - 1;
    for (int i = B.first + tid; i < last; i += FS_THREADS) {
        int bestIdx = -1, bestDist = INT_MAX;
        do {
            const int id = P.points[i];
            if (id < 0 || id >= nmp) break;
            // the point's row, its descriptor and its flag are in flight before the first exit
            const gf_map_point mp = mps[id];
            const uint4* dq = (const uint4*)(mp_desc + (size_t)id * 32);
            const uint4 a0 = dq[0], a1 = dq[1];
            const bool bad = mp_bad && mp_bad[id];
            bool found = false;
            for (int h = (int)(fs_hash(id) % (unsigned)ts), v; (v = tab[h]) != -1; h = h + 1 == ts ? 0 : h + 1)
                if (v == id) {
                    found = true;
                    break;
                }
            if (bad || found) break;  // isBad() || spAlreadyFound.count(pMP) (:1739)
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
        const bool fused = bestDist <= FS_TH_LOW;
        P.res[i] = gf_fuse_sim3_result{fused ? bestIdx : -1, fused ? bestDist : -1};
    }
}

// Decompose Scw (:1719-1723) with the arithmetic gf_search_kf_sim3_projection
// fixes for the same lines of SearchByProjection: scw = sqrt(row0 . row0)
// (Mat::dot, a double sum), Rcw = sRcw / scw and tcw = t / scw as one float
// factor 1 / scw, Ow = -Rcw^T tcw.
void decompose_scw(const float* Scw, float* T, float* Ow) {
    const double d0 = ((double)Scw[0] * Scw[0] + (double)Scw[1] * Scw[1]) + (double)Scw[2] * Scw[2];
    const float scw = (float)std::sqrt(d0);
    const float inv = (float)(1.0 / (double)scw);
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 4; c++) T[4 * r + c] = Scw[4 * r + c] * inv;
    for (int r = 0; r < 3; r++) Ow[r] = -((T[r] * T[3] + T[4 + r] * T[7]) + T[8 + r] * T[11]);
}

// Candidates per workgroup. GF_FUSE_SIM3_CHUNK overrides the default for
// scripts/fuse_sim3_timing.py; read once.
int fuse_sim3_chunk() {
    static const int chunk = [] {
        const char* e = std::getenv("GF_FUSE_SIM3_CHUNK");
        const int v = e ? std::atoi(e) : FS_CHUNK_DEFAULT;
        return std::min(std::max(v, 64), 1 << 16);
    }();
    return chunk;
}

}  // namespace

extern "C" {

int gf_fuse_sim3_dev(gf_ctx* ctx, const gf_frame_info* fi, int nprob, const gf_fuse_sim3_problem* probs,
                     const gf_map_point* d_mps, const uint8_t* d_mp_desc, const uint8_t* d_mp_bad, int nmp,
                     void* stream) {
    GF_CHECK(ctx && fi, GF_ERR_ARG, "gf_fuse_sim3_dev: null arg");
    if (nprob <= 0) return GF_OK;
    GF_CHECK(probs, GF_ERR_ARG, "gf_fuse_sim3_dev: null problems");
    GF_CHECK(fi->nlevels >= 1 && fi->nlevels <= 16, GF_ERR_ARG, "nlevels out of range");
    GF_CHECK(fi->max_x > fi->min_x && fi->max_y > fi->min_y, GF_ERR_ARG, "empty image bounds");
    GF_CHECK(nmp >= 0, GF_ERR_ARG, "nmp < 0");
    const int chunk = fuse_sim3_chunk();
    std::vector<FuseSim3Prob> P(nprob);
    std::vector<FuseSim3Block> B;
    int nmax = 0;
    for (int p = 0; p < nprob; p++) {
        const gf_fuse_sim3_problem& q = probs[p];
        GF_CHECK(q.n >= 0 && q.n <= KP_MAX, GF_ERR_UNSUPPORTED, "at most 4096 keyframe keypoints");
        GF_CHECK(q.npoints >= 0, GF_ERR_ARG, "negative candidate count");
        GF_CHECK(q.npoints == 0 || (q.points && q.res), GF_ERR_ARG, "gf_fuse_sim3_dev: null candidate list or result");
        GF_CHECK(q.npoints == 0 || q.n == 0 || (q.kps && q.desc && q.kf_mp && d_mps && d_mp_desc && nmp > 0),
                 GF_ERR_ARG, "gf_fuse_sim3_dev: null keyframe or map buffer");
        decompose_scw(q.Scw, P[p].T, P[p].Ow);
        P[p].th = q.th;
        P[p].kps = q.kps;
        P[p].desc = q.desc;
        P[p].kf_mp = q.kf_mp;
        P[p].points = q.points;
        P[p].res = q.res;
        P[p].n = q.n;
        P[p].m = q.npoints;
        for (int first = 0; first < q.npoints; first += chunk) B.push_back(FuseSim3Block{p, first});
        if (q.npoints) nmax = std::max(nmax, q.n);
    }
    if (B.empty()) return GF_OK;
    hipStream_t s = (hipStream_t)stream;
    // one scratch block: [problems | workgroup table]
    const size_t pb = (sizeof(FuseSim3Prob) * (size_t)nprob + 15) & ~(size_t)15, bb = sizeof(FuseSim3Block) * B.size();
    void* dp;
    int rc = gf::ws_get(ctx, 18, pb + bb, &dp);
    if (rc) return rc;
    GF_HIP(hipMemcpyAsync(dp, P.data(), sizeof(FuseSim3Prob) * (size_t)nprob, hipMemcpyHostToDevice, s));
    GF_HIP(hipMemcpyAsync((char*)dp + pb, B.data(), bb, hipMemcpyHostToDevice, s));
    GF_PROF(ctx, s, "k_fuse_sim3");
    GF_LAUNCH(k_fuse_sim3, (int)B.size(), FS_THREADS, sizeof(int) * ((size_t)NCELLS + 1 + 3 * (size_t)nmax), s,
              gf::make_frame_const(fi), (const FuseSim3Prob*)dp, (const FuseSim3Block*)((char*)dp + pb), chunk, d_mps,
              d_mp_desc, d_mp_bad, nmp);
    GF_HIP(hipGetLastError());
    return GF_OK;
}

int gf_fuse_sim3(gf_ctx* ctx, const gf_frame_info* fi, const float Scw[16], const gf_keypoint* kps, const uint8_t* desc,
                 int n, const int32_t* kf_mp, const gf_map_point* mps, const uint8_t* mp_desc, const uint8_t* mp_bad,
                 int nmp, const int32_t* points, int npoints, float th, gf_fuse_sim3_result* res) {
    GF_CHECK(ctx && fi && Scw, GF_ERR_ARG, "gf_fuse_sim3: null arg");
    GF_CHECK(n >= 0 && n <= KP_MAX, GF_ERR_UNSUPPORTED, "at most 4096 keyframe keypoints");
    GF_CHECK(nmp >= 0 && npoints >= 0, GF_ERR_ARG, "negative count");
    if (npoints == 0) return GF_OK;
    GF_CHECK(points && res && mps && mp_desc && nmp > 0 && (n == 0 || (kps && desc && kf_mp)), GF_ERR_ARG,
             "gf_fuse_sim3: null buffer");
    for (int i = 0; i < npoints; i++)
        GF_CHECK(points[i] >= 0 && points[i] < nmp, GF_ERR_ARG, "candidate map point id out of range");
    for (int k = 0; k < n; k++) GF_CHECK(kf_mp[k] < nmp, GF_ERR_ARG, "slot map point id out of range");
    GF_HIP(hipSetDevice(ctx->device));
    // one scratch block: [kps | desc | kf_mp | mps | mp_desc | bad | points | res]
    size_t off = 0;
    std::vector<std::pair<const void*, size_t>> parts;
    auto add = [&](const void* h, size_t bytes) {
        const size_t o = off;
        parts.push_back({h, bytes});
        off += (bytes + 15) & ~(size_t)15;
        return o;
    };
    const size_t o_k = add(kps, sizeof(gf_keypoint) * (size_t)n), o_d = add(desc, 32 * (size_t)n),
                 o_s = add(kf_mp, 4 * (size_t)n), o_mp = add(mps, sizeof(gf_map_point) * (size_t)nmp),
                 o_md = add(mp_desc, 32 * (size_t)nmp), o_bad = add(mp_bad, mp_bad ? (size_t)nmp : 0),
                 o_pts = add(points, 4 * (size_t)npoints),
                 o_r = add(nullptr, sizeof(gf_fuse_sim3_result) * (size_t)npoints);
    void* dbuf;
    int rc = gf::ws_get(ctx, 17, off, &dbuf);
    if (rc) return rc;
    uint8_t* base = (uint8_t*)dbuf;
    hipStream_t s = ctx->stream;
    size_t cur = 0;
    for (auto& pr : parts) {
        if (pr.first && pr.second) GF_HIP(hipMemcpyAsync(base + cur, pr.first, pr.second, hipMemcpyHostToDevice, s));
        cur += (pr.second + 15) & ~(size_t)15;
    }
    gf_fuse_sim3_problem q{};
    for (int k = 0; k < 16; k++) q.Scw[k] = Scw[k];
    q.kps = (const gf_keypoint*)(base + o_k);
    q.desc = base + o_d;
    q.n = n;
    q.kf_mp = (const int32_t*)(base + o_s);
    q.points = (const int32_t*)(base + o_pts);
    q.npoints = npoints;
    q.th = th;
    q.res = (gf_fuse_sim3_result*)(base + o_r);
    rc = gf_fuse_sim3_dev(ctx, fi, 1, &q, (const gf_map_point*)(base + o_mp), base + o_md,
                          mp_bad ? base + o_bad : nullptr, nmp, s);
    if (rc) return rc;
    GF_HIP(hipMemcpyAsync(res, base + o_r, sizeof(gf_fuse_sim3_result) * (size_t)npoints, hipMemcpyDeviceToHost, s));
    GF_HIP(hipStreamSynchronize(s));
    return GF_OK;
}

}  // extern "C"
