// Loop-closure Sim3 on gfx950: ORB_SLAM::Sim3Solver (src/Sim3Solver.cc), the
// 3-point Horn RANSAC that LoopClosing::ComputeSim3 runs per loop candidate
// (LoopClosing.cc:240-352), as three kernels per iterate() call of a batch of
// independent solvers (the split of pnp.hip):
//   k_sim3_draw  one lane per solver replays the solver's std::rand() stream
//                and stores every minimal set the call can use; the draws do
//                not depend on the hypotheses;
//   k_sim3_hyp   one wave per hypothesis: lane 0 runs computeT (:226-332) with
//                the pivot-indexed Jacobi matrices in LDS, then the 64 lanes
//                stride over the solver's correspondences (CheckInliers,
//                :335-359); the inlier bits of 64 correspondences come from one
//                __ballot, the count from its popcount. The bit plane of every
//                hypothesis is kept;
//   k_sim3_scan  one wave per solver walks the counts in iteration order as
//                iterate() does (:158-201): best-so-far on >=, return on
//                > min_inliers, bNoMore; expands the chosen bit planes into
//                the best mask and the inlier bytes, advances the caller's
//                std::rand() state by three draws per iteration run.
// The correspondences are read as the ABI hands them over (n x 3 rows): a wave
// reads 64 consecutive rows, 768 contiguous bytes, once per hypothesis, so a
// transposed staging copy would cost a launch and save nothing.
#include "sim3_core.h"
#include "match_common.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <utility>
#include <vector>

namespace {
using namespace gfsim3;

__global__ void k_sim3_draw(int nprob, const gf_sim3_state* __restrict__ states, const gf_rng* __restrict__ rngs,
                            int n_iterations, int lcap, int32_t* __restrict__ draws, int cap) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nprob) return;
    draw_one(states, rngs, b, n_iterations, lcap, draws, cap);
}

__global__ void __launch_bounds__(64) k_sim3_hyp(const float* __restrict__ X1, const float* __restrict__ X2,
                                                 const float* __restrict__ sig1, const float* __restrict__ sig2,
                                                 int cap, Cam k1, Cam k2, const gf_sim3_state* __restrict__ states,
                                                 int n_iterations, int lcap, const int32_t* __restrict__ draws,
                                                 float* __restrict__ hyp, int32_t* __restrict__ hyp_cnt,
                                                 unsigned long long* __restrict__ planes, int nwords) {
    __shared__ float sH[kHyp];
    __shared__ float sT21[12];
    __shared__ float sJ[44];
    const int b = blockIdx.y, h = blockIdx.x, lane = threadIdx.x;
    const gf_sim3_state st = load_state(states, b, cap);
    if (h >= min(loop_count(st, n_iterations), lcap)) return;  // uniform over the wave
    const float* P1 = X1 + (size_t)b * cap * 3;
    const float* P2 = X2 + (size_t)b * cap * 3;
    const float* S1 = sig1 + (size_t)b * cap;
    const float* S2 = sig2 + (size_t)b * cap;
    const size_t slot = (size_t)b * lcap + h;
    if (lane == 0) {
        const int32_t* dr = draws + slot * 3;
        float A[3][3], B[3][3];
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const int idx = dr[i];
#pragma unroll
            for (int k = 0; k < 3; k++) {
                A[k][i] = P1[3 * idx + k];
                B[k][i] = P2[3 * idx + k];
            }
        }
        compute_T(A, B, sH, sT21, sJ);
    }
    __syncthreads();
    float T12[12], T21[12];
#pragma unroll
    for (int i = 0; i < 12; i++) {
        T12[i] = sH[i];
        T21[i] = sT21[i];
    }
    unsigned long long* pl = planes + slot * nwords;
    int cnt = 0;
    for (int base = 0; base < st.n; base += 64) {
        const int i = base + lane;
        bool in = false;
        if (i < st.n) in = is_inlier(P1 + 3 * i, P2 + 3 * i, S1[i], S2[i], T12, T21, k1, k2);
        const unsigned long long m = __ballot(in);
        cnt += __popcll(m);
        if (lane == 0) pl[base >> 6] = m;
    }
    if (lane < kHyp) hyp[slot * kHyp + lane] = sH[lane];
    if (lane == 0) hyp_cnt[slot] = cnt;
}

__global__ void __launch_bounds__(64) k_sim3_scan(int cap, gf_sim3_state* __restrict__ states,
                                                  uint8_t* __restrict__ best_mask, int n_iterations, int lcap,
                                                  const float* __restrict__ hyp, const int32_t* __restrict__ hyp_cnt,
                                                  const unsigned long long* __restrict__ planes, int nwords,
                                                  gf_rng* __restrict__ rngs, float* __restrict__ T12_out,
                                                  uint8_t* __restrict__ inliers, int32_t* __restrict__ ninliers,
                                                  int32_t* __restrict__ flags) {
    __shared__ gf_rng sg;  // indexed by the ring position
    const int b = blockIdx.x, lane = threadIdx.x;
    const gf_sim3_state st = load_state(states, b, cap);
    const int n = st.n;
    const int full = loop_count(st, n_iterations);
    const int L = min(full, lcap);
    const int32_t* cnts = hyp_cnt + (size_t)b * lcap;
    // the walk of :158-201 over the counts (every lane, the same values)
    int best = st.best_inliers, last = -1, ran = 0;
    bool found = false;
    for (int h = 0; h < L && !found; h++) {
        ran = h + 1;
        const int c = cnts[h];
        if (c >= best) {
            best = c;
            last = h;
            found = c > st.min_inliers;
        }
    }
    uint8_t* bm = best_mask + (size_t)b * cap;
    uint8_t* out = inliers + (size_t)b * cap;
    float* T = T12_out + (size_t)b * 16;
    const unsigned long long* pl = planes + ((size_t)b * lcap + (last < 0 ? 0 : last)) * nwords;
    for (int i = lane; i < n; i += 64) {
        const uint8_t bit = last >= 0 ? (uint8_t)((pl[i >> 6] >> (i & 63)) & 1) : 0;
        if (last >= 0) bm[i] = bit;
        out[i] = found ? bit : 0;
    }
    const float* H = hyp + ((size_t)b * lcap + (last < 0 ? 0 : last)) * kHyp;
    if (lane < 16) T[lane] = found ? H[lane] : 0.f;
    if (lane < 31) sg.state[lane] = rngs[b].state[lane];
    __syncthreads();
    if (lane == 0) {
        gf_sim3_state* o = states + b;
        const int iterations = st.iterations + ran;
        o->n = n;
        o->iterations = iterations;
        if (last >= 0) {
            o->best_inliers = best;
            o->best_scale = H[28];
            for (int i = 0; i < 16; i++) o->best_T12[i] = H[i];
            for (int i = 0; i < 9; i++) o->best_R[i] = H[16 + i];
            for (int i = 0; i < 3; i++) o->best_t[i] = H[25 + i];
        }
        int fl = 0;
        if (found) fl = GF_SIM3_FOUND;
        else if (n < st.min_inliers || n < 3 || iterations >= st.max_iterations) fl = GF_SIM3_NOMORE;
        if (full > lcap && !found) fl |= GF_SIM3_TRUNCATED;
        ninliers[b] = found ? best : 0;
        flags[b] = fl;
        int32_t f = rngs[b].f, r = rngs[b].r;
        for (int i = 0; i < ran * 3; i++) (void)gfrng::next(sg.state, &f, &r);
        rngs[b].f = f;
        rngs[b].r = r;
    }
    __syncthreads();
    if (lane < 31) rngs[b].state[lane] = sg.state[lane];
}

// ---------------------------------------------------------------- SearchBySim3
// ORBmatcher::SearchBySim3 (ORBmatcher.cc:1841-2079) for one keyframe pair by
// one 1024-thread workgroup: KF1's unmatched map points into KF2 (sR21, t21),
// KF2's into KF1 (sR12, t12), then the agreement pass. Each thread walks its
// point's window serially in KeyFrame::GetFeaturesInArea order (cell column
// outer, row inner, keypoint index ascending in a cell), so `dist < bestDist`
// keeps the first of equal distances in that order, as the reference does. The
// keypoint grid of the searched keyframe lives in LDS (build_grid), rebuilt
// between the passes.
struct Sim3Side {
    float T[12];   // Rcw | tcw of the keyframe whose points are projected
    float sR[12];  // sR | t into the other camera
    const int32_t* kf_mp;   // projected keyframe: slot -> map point id
    int32_t n;
    const gf_keypoint* kps;  // searched keyframe
    const uint8_t* desc;
    const int32_t* kf_mp_o;
    int32_t n_o;
    int32_t* match;  // vnMatch of the projected keyframe's slots
};

__device__ void sim3_project_search(const FrameConst& fc, const Sim3Side& S, const gf_map_point* __restrict__ mps,
                                    const uint8_t* __restrict__ mp_desc, const uint8_t* __restrict__ mp_bad,
                                    const int32_t* matches12, const uint8_t* mark, float th,
                                    const int* cell_start, const int* items) {
    const int nmax = fc.nlevels - 1;
    for (int i = threadIdx.x; i < S.n; i += MATCH_THREADS) {
        int bestIdx = -1, bestDist = INT_MAX;
        do {
            const int mp = S.kf_mp[i];
            if (mp < 0) break;
            // vbAlreadyMatched1 is the slot's incoming match, vbAlreadyMatched2 the marked map point
            if (matches12 ? matches12[i] >= 0 : mark[mp] != 0) break;
            if (mp_bad && mp_bad[mp]) break;
            const gf_map_point P = mps[mp];
            float Pa[3], Pb[3];
            transform3(S.T, P.pos, Pa);
            transform3(S.sR, Pa, Pb);
            if (Pb[2] < 0.0f) break;
            const float invz = 1.f / Pb[2];
            const float x = Pb[0] * invz, y = Pb[1] * invz;
            const float u = fc.fx * x + fc.cx, v = fc.fy * y + fc.cy;
            // KeyFrame::IsInImage (KeyFrame.cc:654-657)
            if (!(u >= (float)fc.min_x && u < (float)fc.max_x && v >= (float)fc.min_y && v < (float)fc.max_y)) break;
            const float dist3D = (float)sqrt((double)Pb[0] * Pb[0] + (double)Pb[1] * Pb[1] + (double)Pb[2] * Pb[2]);
            if (dist3D < P.min_dist || dist3D > P.max_dist) break;
            const float ratio = dist3D / P.min_dist;
            int lvl = 0;
            while (lvl < fc.nlevels && fc.scales[lvl] < ratio) lvl++;  // lower_bound
            lvl = min(lvl, nmax);
            const float r = th * fc.scales[lvl];
            int cx0, cx1, cy0, cy1;
            if (!grid_window(fc, u, v, r, cx0, cx1, cy0, cy1)) break;
            const uint4* dq = (const uint4*)(mp_desc + (size_t)mp * 32);
            const uint4 a0 = dq[0], a1 = dq[1];
            for (int cx = cx0; cx <= cx1; cx++)
                for (int cy = cy0; cy <= cy1; cy++) {
                    const int c = cx * GRID_ROWS + cy;
                    for (int a = cell_start[c], e = cell_start[c + 1]; a < e; a++) {
                        const int idx = items[a];
                        const gf_keypoint kp = S.kps[idx];
                        if (!(fabsf(kp.x - u) <= r && fabsf(kp.y - v) <= r)) continue;
                        if (kp.octave < lvl - 1 || kp.octave > lvl) continue;
                        const uint4* dk = (const uint4*)(S.desc + (size_t)idx * 32);
                        const int d = hamming_regs(a0, a1, dk[0], dk[1]);
                        if (d < bestDist) {
                            bestDist = d;
                            bestIdx = idx;
                        }
                    }
                }
        } while (false);
        S.match[i] = bestDist <= TH_HIGH ? bestIdx : -1;
    }
}

__global__ __launch_bounds__(MATCH_THREADS) void k_search_sim3(FrameConst fc, Sim3Side s1, Sim3Side s2,
                                                               const gf_map_point* __restrict__ mps,
                                                               const uint8_t* __restrict__ mp_desc,
                                                               const uint8_t* __restrict__ mp_bad, int nmp,
                                                               int32_t* matches12,
                                                               uint8_t* mark, float th,
                                                               int32_t* __restrict__ nfound) {
    extern __shared__ int lds[];
    const int tid = threadIdx.x;
    const int nmaxkp = max(s1.n, s2.n);
    int* cell_start = lds;                 // NCELLS + 1
    int* items = cell_start + NCELLS + 1;  // n
    int* claim = items + nmaxkp;           // n (build_grid's copy of the slot table, unused here)
    int* scratch = claim + nmaxkp;         // n
    __shared__ int s_nf;
    if (tid == 0) s_nf = 0;
    // vbAlreadyMatched2 (:1877-1887): the map points named by the incoming matches
    for (int i = tid; i < s1.n; i += MATCH_THREADS) {
        const int m = matches12[i];
        if (m >= 0 && m < nmp) mark[m] = 1;
    }
    // KF1 -> KF2 (:1893-1973) over KF2's grid
    build_grid(fc, s1.kps, s1.n_o, s1.kf_mp_o, cell_start, items, claim, scratch, MATCH_THREADS);
    sim3_project_search(fc, s1, mps, mp_desc, mp_bad, matches12, nullptr, th, cell_start, items);
    __syncthreads();
    // KF2 -> KF1 (:1976-2058) over KF1's grid
    build_grid(fc, s2.kps, s2.n_o, s2.kf_mp_o, cell_start, items, claim, scratch, MATCH_THREADS);
    sim3_project_search(fc, s2, mps, mp_desc, mp_bad, nullptr, mark, th, cell_start, items);
    __syncthreads();
    // agreement (:2060-2076)
    int nf = 0;
    for (int i1 = tid; i1 < s1.n; i1 += MATCH_THREADS) {
        const int idx2 = s1.match[i1];
        if (idx2 >= 0 && s2.match[idx2] == i1) {
            matches12[i1] = s2.kf_mp[idx2];
            nf++;
        }
    }
    if (nf) atomicAdd(&s_nf, nf);
    __syncthreads();
    if (tid == 0) *nfound = s_nf;
}

// ------------------------------------------- SearchByProjection(pKF, Scw, ...)
// ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th)
// (ORBmatcher.cc:855-977) by one 1024-thread workgroup. The reference walks
// the candidates in list order and writes vpMatched[bestIdx] inside the loop,
// so a keypoint taken by an earlier candidate is gone for the later ones. That
// is a serial dictatorship, which equals the one stable assignment when every
// keypoint prefers the lower candidate index and every candidate orders the
// keypoints of its window by (distance, GetFeaturesInArea position), cut at
// TH_LOW. The rounds below reach it by deferred acceptance: owner[k] is the
// lowest candidate that has asked for keypoint k so far and only ever
// decreases; a candidate that does not hold its keypoint searches again among
// the keypoints whose owner is above it. A candidate's choice set only
// shrinks, so a keypoint it holds stays its best, and one that finds nothing
// is done. Each round with a request lowers an owner: at most m + 1 rounds.
#define SP_TH_LOW 50

struct ProjCand {
    float u, v, r;
    int32_t lvl;  // predicted level, -1: the candidate left at one of the exits
};

struct ProjArgs {
    float T[12];  // Rcw | tcw of the decomposed Scw
    float Ow[3];
    const gf_keypoint* kps;
    const uint8_t* desc;
    int32_t n;
    const gf_map_point* mps;
    const uint8_t* mp_desc;
    const uint8_t* mp_bad;
    int32_t nmp;
    const int32_t* points;  // vpPoints: map point ids, list order
    int32_t m;
    int32_t* matched;  // vpMatched, in and out
    uint8_t* mark;     // nmp bytes, zeroed: spAlreadyFound
    ProjCand* cand;    // m
    int32_t* cur;      // m: the keypoint candidate i asked for, -1 none yet, -2 nothing left
    float th;
    int32_t* nmatches;
};

__global__ __launch_bounds__(MATCH_THREADS) void k_search_proj_sim3(FrameConst fc, ProjArgs P) {
    extern __shared__ int lds[];
    const int tid = threadIdx.x, n = P.n, m = P.m;
    int* cell_start = lds;                 // NCELLS + 1
    int* items = cell_start + NCELLS + 1;  // n
    int* owner = items + n;                // n
    int* scratch = owner + n;              // n
    __shared__ int s_req, s_nm;
    if (tid == 0) s_nm = 0;
    build_grid(fc, P.kps, n, P.matched, cell_start, items, owner, scratch, MATCH_THREADS);
    // spAlreadyFound (:874-875) is built once, before the loop
    for (int k = tid; k < n; k += MATCH_THREADS) {
        const int id = owner[k];
        if (id >= 0 && id < P.nmp) P.mark[id] = 1;
        owner[k] = id >= 0 ? -1 : INT_MAX;  // vpMatched[idx] set at entry: taken for everyone
    }
    __syncthreads();
    const int nmax = fc.nlevels - 1;
    // the exits that do not depend on the claims (:882-937, window part)
    for (int i = tid; i < m; i += MATCH_THREADS) {
        ProjCand c{0.f, 0.f, 0.f, -1};
        do {
            const int id = P.points[i];
            if (id < 0 || id >= P.nmp) break;
            if ((P.mp_bad && P.mp_bad[id]) || P.mark[id]) break;
            const gf_map_point mp = P.mps[id];
            float Pc[3];
            transform3(P.T, mp.pos, Pc);
            if (Pc[2] < 0.0f) break;
            const float invz = 1.f / Pc[2];
            const float x = Pc[0] * invz, y = Pc[1] * invz;
            const float u = fc.fx * x + fc.cx, v = fc.fy * y + fc.cy;
            if (!(u >= (float)fc.min_x && u < (float)fc.max_x && v >= (float)fc.min_y && v < (float)fc.max_y)) break;
            const float PO[3] = {mp.pos[0] - P.Ow[0], mp.pos[1] - P.Ow[1], mp.pos[2] - P.Ow[2]};
            // cv::norm / Mat::dot accumulate in double
            const float dist = (float)sqrt((double)PO[0] * PO[0] + (double)PO[1] * PO[1] + (double)PO[2] * PO[2]);
            if (dist < mp.min_dist || dist > mp.max_dist) break;
            const double dot = (double)PO[0] * mp.normal[0] + (double)PO[1] * mp.normal[1] + (double)PO[2] * mp.normal[2];
            if (dot < 0.5 * (double)dist) break;
            const float ratio = dist / mp.min_dist;
            int lvl = 0;
            while (lvl < fc.nlevels && fc.scales[lvl] < ratio) lvl++;  // lower_bound
            lvl = min(lvl, nmax);
            c = ProjCand{u, v, P.th * fc.scales[lvl], lvl};
        } while (false);
        P.cand[i] = c;
        P.cur[i] = -1;
    }
    __syncthreads();
    for (int round = 0; round <= m; round++) {
        if (tid == 0) s_req = 0;
        __syncthreads();
        for (int i = tid; i < m; i += MATCH_THREADS) {
            const ProjCand c = P.cand[i];
            const int held = P.cur[i];
            if (c.lvl < 0 || held == -2 || (held >= 0 && owner[held] == i)) continue;
            int bestIdx = -1, bestDist = INT_MAX;
            int cx0, cx1, cy0, cy1;
            if (grid_window(fc, c.u, c.v, c.r, cx0, cx1, cy0, cy1)) {
                const uint4* dq = (const uint4*)(P.mp_desc + (size_t)P.points[i] * 32);
                const uint4 a0 = dq[0], a1 = dq[1];
                for (int cx = cx0; cx <= cx1; cx++)
                    for (int cy = cy0; cy <= cy1; cy++) {
                        const int cell = cx * GRID_ROWS + cy;
                        for (int a = cell_start[cell], e = cell_start[cell + 1]; a < e; a++) {
                            const int idx = items[a];
                            if (owner[idx] <= i) continue;  // vpMatched[idx] set by the entry or an earlier candidate
                            const gf_keypoint kp = P.kps[idx];
                            if (!(fabsf(kp.x - c.u) <= c.r && fabsf(kp.y - c.v) <= c.r)) continue;
                            if (kp.octave < c.lvl - 1 || kp.octave > c.lvl) continue;
                            const uint4* dk = (const uint4*)(P.desc + (size_t)idx * 32);
                            const int d = hamming_regs(a0, a1, dk[0], dk[1]);
                            if (d < bestDist) {
                                bestDist = d;
                                bestIdx = idx;
                            }
                        }
                    }
            }
            if (bestDist <= SP_TH_LOW) {
                P.cur[i] = bestIdx;
                atomicMin(&owner[bestIdx], i);
                s_req = 1;
            } else {
                P.cur[i] = -2;
            }
        }
        __syncthreads();
        const int req = s_req;
        __syncthreads();
        if (!req) break;
    }
    int nm = 0;
    for (int k = tid; k < n; k += MATCH_THREADS) {
        const int o = owner[k];
        if (o >= 0 && o < m) {
            P.matched[k] = P.points[o];
            nm++;
        }
    }
    if (nm) atomicAdd(&s_nm, nm);
    __syncthreads();
    if (tid == 0) *P.nmatches = s_nm;
}

}  // namespace

extern "C" {

int gf_search_kf_sim3_projection(gf_ctx* ctx, const gf_frame_info* fi, const float Scw[16], const gf_keypoint* kps,
                                 const uint8_t* desc, int n, const gf_map_point* mps, const uint8_t* mp_desc,
                                 const uint8_t* mp_bad, int nmp, const int32_t* points, int npoints, int32_t* matched,
                                 int th, int* nmatches) {
    GF_CHECK(ctx && fi && Scw && nmatches, GF_ERR_ARG, "gf_search_kf_sim3_projection: null arg");
    GF_CHECK(fi->nlevels >= 1 && fi->nlevels <= 16, GF_ERR_ARG, "nlevels out of range");
    GF_CHECK(fi->max_x > fi->min_x && fi->max_y > fi->min_y, GF_ERR_ARG, "empty image bounds");
    GF_CHECK(n >= 0 && n <= KP_MAX, GF_ERR_UNSUPPORTED, "at most 4096 keyframe keypoints");
    GF_CHECK(nmp >= 0 && npoints >= 0, GF_ERR_ARG, "negative count");
    *nmatches = 0;
    if (n == 0 || npoints == 0) return GF_OK;
    GF_CHECK(kps && desc && matched && points && mps && mp_desc && nmp > 0, GF_ERR_ARG,
             "gf_search_kf_sim3_projection: null buffer");
    for (int i = 0; i < npoints; i++)
        GF_CHECK(points[i] >= 0 && points[i] < nmp, GF_ERR_ARG, "candidate map point id out of range");
    for (int i = 0; i < n; i++) GF_CHECK(matched[i] < nmp, GF_ERR_ARG, "matched map point id out of range");
    GF_HIP(hipSetDevice(ctx->device));
    size_t off = 0;
    std::vector<std::pair<const void*, size_t>> parts;
    auto add = [&](const void* h, size_t bytes) {
        const size_t o = off;
        parts.push_back({h, bytes});
        off += (bytes + 15) & ~(size_t)15;
        return o;
    };
    const size_t o_k = add(kps, sizeof(gf_keypoint) * (size_t)n), o_d = add(desc, 32 * (size_t)n),
                 o_mp = add(mps, sizeof(gf_map_point) * (size_t)nmp), o_md = add(mp_desc, 32 * (size_t)nmp),
                 o_bad = add(mp_bad, mp_bad ? (size_t)nmp : 0), o_pts = add(points, 4 * (size_t)npoints),
                 o_m = add(matched, 4 * (size_t)n), o_mark = add(nullptr, (size_t)nmp),
                 o_cand = add(nullptr, sizeof(ProjCand) * (size_t)npoints), o_cur = add(nullptr, 4 * (size_t)npoints),
                 o_nm = add(nullptr, 4);
    void* dbuf;
    int rc = gf::ws_get(ctx, 0, off, &dbuf);
    if (rc) return rc;
    uint8_t* base = (uint8_t*)dbuf;
    hipStream_t s = ctx->stream;
    size_t cur = 0;
    for (auto& pr : parts) {
        if (pr.first && pr.second) GF_HIP(hipMemcpyAsync(base + cur, pr.first, pr.second, hipMemcpyHostToDevice, s));
        cur += (pr.second + 15) & ~(size_t)15;
    }
    GF_HIP(hipMemsetAsync(base + o_mark, 0, (size_t)nmp, s));
    ProjArgs P{};
    // Decompose Scw (:866-871): scw = sqrt(row0 . row0) (Mat::dot, a double sum),
    // Rcw = sRcw / scw and tcw = t / scw as one float factor 1 / scw, Ow = -Rcw^T tcw
    const double d0 = ((double)Scw[0] * Scw[0] + (double)Scw[1] * Scw[1]) + (double)Scw[2] * Scw[2];
    const float scw = (float)std::sqrt(d0);
    const float inv = (float)(1.0 / (double)scw);
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 4; c++) P.T[4 * r + c] = Scw[4 * r + c] * inv;
    for (int r = 0; r < 3; r++) P.Ow[r] = -((P.T[r] * P.T[3] + P.T[4 + r] * P.T[7]) + P.T[8 + r] * P.T[11]);
    P.kps = (const gf_keypoint*)(base + o_k);
    P.desc = base + o_d;
    P.n = n;
    P.mps = (const gf_map_point*)(base + o_mp);
    P.mp_desc = base + o_md;
    P.mp_bad = mp_bad ? base + o_bad : nullptr;
    P.nmp = nmp;
    P.points = (const int32_t*)(base + o_pts);
    P.m = npoints;
    P.matched = (int32_t*)(base + o_m);
    P.mark = base + o_mark;
    P.cand = (ProjCand*)(base + o_cand);
    P.cur = (int32_t*)(base + o_cur);
    P.th = (float)th;
    P.nmatches = (int32_t*)(base + o_nm);
    {
        GF_PROF(ctx, s, "k_search_proj_sim3");
        GF_LAUNCH(k_search_proj_sim3, 1, MATCH_THREADS, sizeof(int) * ((size_t)NCELLS + 1 + 3 * (size_t)n), s,
                  gf::make_frame_const(fi), P);
        GF_HIP(hipGetLastError());
    }
    int32_t nm = 0;
    GF_HIP(hipMemcpyAsync(matched, base + o_m, 4 * (size_t)n, hipMemcpyDeviceToHost, s));
    GF_HIP(hipMemcpyAsync(&nm, base + o_nm, 4, hipMemcpyDeviceToHost, s));
    GF_HIP(hipStreamSynchronize(s));
    *nmatches = nm;
    return GF_OK;
}

int gf_search_by_sim3(gf_ctx* ctx, const gf_frame_info* fi, const float* Tcw1, const gf_keypoint* kps1,
                      const uint8_t* desc1, int n1, const int32_t* kf_mp1, const float* Tcw2, const gf_keypoint* kps2,
                      const uint8_t* desc2, int n2, const int32_t* kf_mp2, const gf_map_point* mps,
                      const uint8_t* mp_desc, const uint8_t* mp_bad, int nmp, int32_t* matches12, float s12,
                      const float R12[9], const float t12[3], float th, int* nfound) {
    GF_CHECK(ctx && fi && Tcw1 && Tcw2 && R12 && t12 && nfound, GF_ERR_ARG, "gf_search_by_sim3: null arg");
    GF_CHECK(fi->nlevels >= 1 && fi->nlevels <= 16, GF_ERR_ARG, "nlevels out of range");
    GF_CHECK(fi->max_x > fi->min_x && fi->max_y > fi->min_y, GF_ERR_ARG, "empty image bounds");
    GF_CHECK(n1 >= 0 && n1 <= KP_MAX && n2 >= 0 && n2 <= KP_MAX, GF_ERR_UNSUPPORTED, "at most 4096 keyframe keypoints");
    GF_CHECK(nmp >= 0, GF_ERR_ARG, "nmp < 0");
    *nfound = 0;
    if (n1 == 0 || n2 == 0) return GF_OK;
    GF_CHECK(kps1 && desc1 && kf_mp1 && kps2 && desc2 && kf_mp2 && matches12 && (nmp == 0 || (mps && mp_desc)),
             GF_ERR_ARG, "gf_search_by_sim3: null buffer");
    for (int i = 0; i < n1; i++)
        GF_CHECK(kf_mp1[i] < nmp && matches12[i] < nmp, GF_ERR_ARG, "gf_search_by_sim3: map point id out of range");
    for (int i = 0; i < n2; i++) GF_CHECK(kf_mp2[i] < nmp, GF_ERR_ARG, "gf_search_by_sim3: map point id out of range");
    GF_HIP(hipSetDevice(ctx->device));
    // one scratch block
    size_t off = 0;
    std::vector<std::pair<const void*, size_t>> parts;
    auto add = [&](const void* h, size_t bytes) {
        const size_t o = off;
        parts.push_back({h, bytes});
        off += (bytes + 15) & ~(size_t)15;
        return o;
    };
    const size_t o_k1 = add(kps1, sizeof(gf_keypoint) * (size_t)n1), o_d1 = add(desc1, 32 * (size_t)n1),
                 o_m1 = add(kf_mp1, 4 * (size_t)n1), o_k2 = add(kps2, sizeof(gf_keypoint) * (size_t)n2),
                 o_d2 = add(desc2, 32 * (size_t)n2), o_m2 = add(kf_mp2, 4 * (size_t)n2),
                 o_mp = add(mps, sizeof(gf_map_point) * (size_t)nmp), o_md = add(mp_desc, 32 * (size_t)nmp),
                 o_bad = add(mp_bad, mp_bad ? (size_t)nmp : 0), o_12 = add(matches12, 4 * (size_t)n1),
                 o_v1 = add(nullptr, 4 * (size_t)n1), o_v2 = add(nullptr, 4 * (size_t)n2),
                 o_mark = add(nullptr, (size_t)nmp + 1), o_nf = add(nullptr, 4);
    void* dbuf;
    int rc = gf::ws_get(ctx, 0, off, &dbuf);
    if (rc) return rc;
    uint8_t* base = (uint8_t*)dbuf;
    hipStream_t s = ctx->stream;
    size_t cur = 0;
    for (auto& pr : parts) {
        if (pr.first && pr.second) GF_HIP(hipMemcpyAsync(base + cur, pr.first, pr.second, hipMemcpyHostToDevice, s));
        cur += (pr.second + 15) & ~(size_t)15;
    }
    GF_HIP(hipMemsetAsync(base + o_mark, 0, (size_t)nmp + 1, s));
    // sR12 = s12*R12, sR21 = (1.0/s12)*R12.t(), t21 = -sR21*t12 (:1858-1860)
    Sim3Side a{}, b{};
    const float inv = (float)(1.0 / (double)s12);
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) {
            b.sR[4 * r + c] = R12[3 * r + c] * s12;
            a.sR[4 * r + c] = R12[3 * c + r] * inv;
        }
        b.sR[4 * r + 3] = t12[r];
    }
    for (int r = 0; r < 3; r++)
        a.sR[4 * r + 3] = -((a.sR[4 * r] * t12[0] + a.sR[4 * r + 1] * t12[1]) + a.sR[4 * r + 2] * t12[2]);
    for (int k = 0; k < 12; k++) {
        a.T[k] = Tcw1[k];
        b.T[k] = Tcw2[k];
    }
    a.kf_mp = (const int32_t*)(base + o_m1), a.n = n1;
    a.kps = (const gf_keypoint*)(base + o_k2), a.desc = base + o_d2, a.kf_mp_o = (const int32_t*)(base + o_m2), a.n_o = n2;
    a.match = (int32_t*)(base + o_v1);
    b.kf_mp = (const int32_t*)(base + o_m2), b.n = n2;
    b.kps = (const gf_keypoint*)(base + o_k1), b.desc = base + o_d1, b.kf_mp_o = (const int32_t*)(base + o_m1), b.n_o = n1;
    b.match = (int32_t*)(base + o_v2);
    {
        GF_PROF(ctx, s, "k_search_sim3");
        GF_LAUNCH(k_search_sim3, 1, MATCH_THREADS, sizeof(int) * ((size_t)NCELLS + 1 + 3 * (size_t)std::max(n1, n2)), s,
                  gf::make_frame_const(fi), a, b, (const gf_map_point*)(base + o_mp), (const uint8_t*)(base + o_md),
                  mp_bad ? (const uint8_t*)(base + o_bad) : (const uint8_t*)nullptr, nmp, (int32_t*)(base + o_12),
                  (uint8_t*)(base + o_mark), th, (int32_t*)(base + o_nf));
        GF_HIP(hipGetLastError());
    }
    int32_t nf = 0;
    GF_HIP(hipMemcpyAsync(matches12, base + o_12, 4 * (size_t)n1, hipMemcpyDeviceToHost, s));
    GF_HIP(hipMemcpyAsync(&nf, base + o_nf, 4, hipMemcpyDeviceToHost, s));
    GF_HIP(hipStreamSynchronize(s));
    *nfound = nf;
    return GF_OK;
}

int gf_sim3_init(int n, const gf_sim3_params* p, gf_sim3_state* st) {
    if (!p || !st || n < 0) return gf::fail(GF_ERR_ARG, "gf_sim3_init: null arg or n < 0");
    // SetRansacParameters :114-138 (host scalar set-up)
    *st = gf_sim3_state{};
    st->n = n;
    st->min_inliers = p->min_inliers;
    const float epsilon = (float)p->min_inliers / n;
    int nIterations;
    if (p->min_inliers == n) {
        nIterations = 1;
    } else {
        // the reference converts a NaN / out-of-range double to int here
        const double it = std::ceil(std::log(1 - p->probability) / std::log(1 - std::pow((double)epsilon, 3.0)));
        nIterations = (it == it && it < 2147483647.0 && it > -2147483648.0) ? (int)it : p->max_iterations;
    }
    st->max_iterations = std::max(1, std::min(nIterations, p->max_iterations));
    return GF_OK;
}

int gf_sim3_iterate_dev(gf_ctx* ctx, int nprob, const float* d_X1, const float* d_X2, const float* d_sigma2_1,
                        const float* d_sigma2_2, int cap, const float K1[4], const float K2[4],
                        gf_sim3_state* d_state, uint8_t* d_best_mask, int n_iterations, int max_iterations,
                        gf_rng* d_rng, float* d_T12, uint8_t* d_inliers, int32_t* d_ninliers, int32_t* d_flags,
                        void* stream) {
    GF_CHECK(ctx && K1 && K2, GF_ERR_ARG, "gf_sim3_iterate_dev: null arg");
    if (nprob <= 0) return GF_OK;
    GF_CHECK(d_X1 && d_X2 && d_sigma2_1 && d_sigma2_2 && d_state && d_best_mask && d_rng && d_T12 && d_inliers &&
                 d_ninliers && d_flags && cap > 0,
             GF_ERR_ARG, "gf_sim3_iterate_dev: null buffer or cap <= 0");
    const int lcap = std::max(std::min(n_iterations, max_iterations), 1);
    const int nwords = (cap + 63) / 64;
    hipStream_t s = (hipStream_t)stream;
    // one device-family scratch slot (63), carved: records, planes, draws, counts
    const size_t nh = (size_t)lcap * nprob;
    const size_t o_planes = sizeof(float) * kHyp * nh;
    const size_t o_draws = o_planes + sizeof(unsigned long long) * nwords * nh;
    const size_t o_cnt = o_draws + sizeof(int32_t) * 3 * nh;
    void* ws;
    int rc;
    if ((rc = gf::ws_get(ctx, 63, o_cnt + sizeof(int32_t) * nh, &ws))) return rc;
    float* hyp = (float*)ws;
    unsigned long long* planes = (unsigned long long*)((char*)ws + o_planes);
    int32_t* draws = (int32_t*)((char*)ws + o_draws);
    int32_t* cnt = (int32_t*)((char*)ws + o_cnt);
    const Cam k1{K1[0], K1[1], K1[2], K1[3]}, k2{K2[0], K2[1], K2[2], K2[3]};
    {
        GF_PROF(ctx, s, "k_sim3_draw");
        GF_LAUNCH(k_sim3_draw, (nprob + 63) / 64, 64, 0, s, nprob, d_state, d_rng, n_iterations, lcap, draws, cap);
        GF_HIP(hipGetLastError());
    }
    {
        GF_PROF(ctx, s, "k_sim3_hyp");
        GF_LAUNCH(k_sim3_hyp, dim3(lcap, nprob), 64, 0, s, d_X1, d_X2, d_sigma2_1, d_sigma2_2, cap, k1, k2, d_state,
                  n_iterations, lcap, (const int32_t*)draws, hyp, cnt, planes, nwords);
        GF_HIP(hipGetLastError());
    }
    {
        GF_PROF(ctx, s, "k_sim3_scan");
        GF_LAUNCH(k_sim3_scan, nprob, 64, 0, s, cap, d_state, d_best_mask, n_iterations, lcap, (const float*)hyp,
                  (const int32_t*)cnt, (const unsigned long long*)planes, nwords, d_rng, d_T12, d_inliers, d_ninliers,
                  d_flags);
        GF_HIP(hipGetLastError());
    }
    return GF_OK;
}

int gf_sim3_iterate(gf_ctx* ctx, const float* X1, const float* X2, const float* sigma2_1, const float* sigma2_2,
                    const float K1[4], const float K2[4], gf_sim3_state* state, uint8_t* best_mask, int n_iterations,
                    gf_rng* rng, float T12[16], uint8_t* inliers, int32_t* ninliers, int32_t* flags) {
    GF_CHECK(ctx && K1 && K2 && state && rng && T12 && ninliers && flags, GF_ERR_ARG, "gf_sim3_iterate: null arg");
    const int n = state->n;
    GF_CHECK(n >= 0, GF_ERR_ARG, "gf_sim3_iterate: state not initialised");
    GF_CHECK(n == 0 || (X1 && X2 && sigma2_1 && sigma2_2 && best_mask && inliers), GF_ERR_ARG,
             "gf_sim3_iterate: null buffer");
    GF_HIP(hipSetDevice(ctx->device));
    const int cap = std::max(n, 1);
    void *d1, *d2, *ds1, *ds2, *dst, *dbm, *drng, *dT, *dinl, *dn, *dfl;
    int rc;
    if ((rc = gf::ws_upload(ctx, 0, X1, sizeof(float) * 3 * (size_t)n, &d1)) ||
        (rc = gf::ws_upload(ctx, 1, X2, sizeof(float) * 3 * (size_t)n, &d2)) ||
        (rc = gf::ws_upload(ctx, 2, sigma2_1, sizeof(float) * (size_t)n, &ds1)) ||
        (rc = gf::ws_upload(ctx, 3, sigma2_2, sizeof(float) * (size_t)n, &ds2)) ||
        (rc = gf::ws_upload(ctx, 4, state, sizeof(gf_sim3_state), &dst)) ||
        (rc = gf::ws_upload(ctx, 5, best_mask, (size_t)n, &dbm)) ||
        (rc = gf::ws_upload(ctx, 6, rng, sizeof(gf_rng), &drng)) || (rc = gf::ws_get(ctx, 7, sizeof(float) * 16, &dT)) ||
        (rc = gf::ws_get(ctx, 8, (size_t)cap, &dinl)) || (rc = gf::ws_get(ctx, 9, sizeof(int32_t), &dn)) ||
        (rc = gf::ws_get(ctx, 10, sizeof(int32_t), &dfl)))
        return rc;
    // the draw/hypothesis bound: this call's loop count
    const int L = std::min(n_iterations, state->max_iterations - state->iterations);
    rc = gf_sim3_iterate_dev(ctx, 1, (const float*)d1, (const float*)d2, (const float*)ds1, (const float*)ds2, cap, K1,
                             K2, (gf_sim3_state*)dst, (uint8_t*)dbm, n_iterations, std::max(L, 1), (gf_rng*)drng,
                             (float*)dT, (uint8_t*)dinl, (int32_t*)dn, (int32_t*)dfl, ctx->stream);
    if (rc) return rc;
    hipStream_t s = ctx->stream;
    GF_HIP(hipMemcpyAsync(state, dst, sizeof(gf_sim3_state), hipMemcpyDeviceToHost, s));
    GF_HIP(hipMemcpyAsync(rng, drng, sizeof(gf_rng), hipMemcpyDeviceToHost, s));
    GF_HIP(hipMemcpyAsync(T12, dT, sizeof(float) * 16, hipMemcpyDeviceToHost, s));
    GF_HIP(hipMemcpyAsync(ninliers, dn, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    GF_HIP(hipMemcpyAsync(flags, dfl, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (n) {
        GF_HIP(hipMemcpyAsync(best_mask, dbm, (size_t)n, hipMemcpyDeviceToHost, s));
        GF_HIP(hipMemcpyAsync(inliers, dinl, (size_t)n, hipMemcpyDeviceToHost, s));
    }
    GF_HIP(hipStreamSynchronize(s));
    return GF_OK;
}

}  // extern "C"
