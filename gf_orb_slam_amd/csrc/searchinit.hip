// ORBmatcher::SearchForInitialization (ORBmatcher.cc:1172-1287) and the gate
// of Tracking::Initialize (Tracking.cc:999-1017) on gfx950, for a batch of
// independent two-frame problems (every sequence of a multi-sequence tracker
// at start-up).
//
// The reference walks F1's keypoints in index order and its accepts feed back
// into the candidate filter (vMatchedDistance), so the claim state is
// sequential. Everything that does not read it is taken out of that walk:
//
//   k_si_grid     one workgroup per problem: F2's level-0 keypoints in the
//                 64 x 48 grid of Frame.cc:100-131 (cells ix-major, keypoint
//                 index ascending inside a cell), to HBM scratch;
//   k_si_cand     one wave per (problem, level-0 query of F1): the window of
//                 Frame::GetFeaturesInArea (Frame.cc:300-365) around
//                 vbPrevMatched[i1] in the reference's order, the 256-bit
//                 Hamming distances, and the list (F2 index, distance) in
//                 walk order, at most SI_CAP entries; a longer list is
//                 flagged. Reads no match state;
//   k_si_resolve  one wave per problem walks F1 in index order with
//                 vMatchedDistance and vnMatches21 in LDS: a query's stored
//                 list is one entry per lane, filtered by vMatchedDistance and
//                 reduced to best / second best / first best position; then
//                 the accept and the steal. A flagged query (and every query
//                 under GF_SI_DIRECT) walks its window itself with the
//                 distances computed in place. Then the rotation histogram
//                 over every accept (robbed queries included), the three
//                 maxima, the removal, vbPrevMatched and nmatches;
//   k_si_gate     Tracking::Initialize's two tests per problem.
#include <algorithm>

#include "common.h"
#include "match_common.h"
#include "top2.h"

namespace {

constexpr int SI_T = 64;        // one wave per query / per problem
constexpr int SI_QW = 4;        // queries (waves) per workgroup of k_si_cand
constexpr int SI_GRID_T = 256;  // k_si_grid, k_si_gate
// Stored candidates per query: one per lane of the resolving wave, so a query
// is one load and one reduction (256 B a query in HBM). The EuRoC shape has a
// few tens of level-0 candidates in a 200 x 200 window.
constexpr int SI_CAP = 64;
constexpr int SI_FLAG = 0x7fffffff;  // count of a query that walks its window in the resolve pass
constexpr int SI_TH_LOW = 50;

struct SIArgs {
    FrameConst fc;
    const gf_keypoint* K1;  // [P][cap1]
    const uint8_t* D1;
    const int32_t* n1;
    int cap1;
    const gf_keypoint* K2;  // [P][cap2]
    const uint8_t* D2;
    const int32_t* n2;
    int cap2;
    float* prev;   // [P][cap1][2] vbPrevMatched, in / out
    int32_t* m12;  // [P][cap1]
    int32_t* nm;   // [P]
    float window, nnratio;
    int check_ori, direct;
    int32_t* grid;  // [P][NCELLS + 1 + cap2]: cell_start, items
    int32_t* cnt;   // [P][cap1]: list length, 0 = no search, SI_FLAG = direct walk
    int32_t* cand;  // [P][cap1][SI_CAP]: F2 index << 9 | distance
};

__host__ __device__ inline size_t si_grid_ints(int cap2) { return (size_t)NCELLS + 1 + (size_t)cap2; }

__device__ __forceinline__ int clampn(int n, int cap) { return min(max(n, 0), cap); }

// F2's level-0 grid (Frame.cc:100-131 with PosInGrid, :367-377). The placement
// by atomics is unordered, so every cell is sorted afterwards.
__global__ __launch_bounds__(SI_GRID_T) void k_si_grid(SIArgs A) {
    __shared__ int cs[NCELLS + 1];
    __shared__ short cell_of[KP_MAX], items[KP_MAX];
    const int p = blockIdx.x, tid = threadIdx.x;
    const int n2 = clampn(A.n2[p], A.cap2);
    const gf_keypoint* K2 = A.K2 + (size_t)p * A.cap2;
    int32_t* g = A.grid + (size_t)p * si_grid_ints(A.cap2);
    for (int c = tid; c < NCELLS + 1; c += SI_GRID_T) cs[c] = 0;
    __syncthreads();
    for (int i = tid; i < n2; i += SI_GRID_T) {
        const gf_keypoint kp = K2[i];
        const int px = (int)roundf((kp.x - A.fc.min_x) * A.fc.invW);
        const int py = (int)roundf((kp.y - A.fc.min_y) * A.fc.invH);
        const bool in = !(px < 0 || px >= GRID_COLS || py < 0 || py >= GRID_ROWS) && kp.octave == 0;
        const int c = in ? px * GRID_ROWS + py : -1;
        cell_of[i] = (short)c;
        if (in) atomicAdd(&cs[c + 1], 1);
    }
    __syncthreads();
    if (tid < 64) {  // inclusive scan of the 3072 counts: cs[c + 1] = end of cell c
        int carry = 0;
        for (int base = 0; base < NCELLS; base += 64) {
            int x = cs[base + 1 + tid];
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int y = __shfl_up(x, o, 64);
                if (tid >= o) x += y;
            }
            cs[base + 1 + tid] = carry + x;
            carry += __shfl(x, 63, 64);
        }
    }
    __syncthreads();
    const int total = cs[NCELLS];  // the end of the last cell
    __syncthreads();
    // cs[c + 1] counts down from the cell's end to its start while its keypoints are placed
    for (int i = tid; i < n2; i += SI_GRID_T) {
        const int c = cell_of[i];
        if (c >= 0) items[atomicSub(&cs[c + 1], 1) - 1] = (short)i;
    }
    __syncthreads();
    // now cs[c + 1] = start of cell c; its end = start of cell c + 1, or the total for the last one
    for (int c = tid; c < NCELLS; c += SI_GRID_T) {
        const int s = cs[c + 1], e = c + 1 < NCELLS ? cs[c + 2] : total;
        for (int a = s + 1; a < e; a++) {
            const short v = items[a];
            int b = a - 1;
            while (b >= s && items[b] > v) {
                items[b + 1] = items[b];
                b--;
            }
            items[b + 1] = v;
        }
    }
    __syncthreads();
    for (int c = tid; c < NCELLS; c += SI_GRID_T) g[c] = cs[c + 1];
    if (tid == 0) g[NCELLS] = total;
    for (int i = tid; i < total; i += SI_GRID_T) g[NCELLS + 1 + i] = items[i];
}

// The cells of one window in walk order c = (ix - cx0) * ncy + (iy - cy0),
// dealt to the lanes in turn. f(idx, c, j) for each level-0 keypoint of F2
// inside the square, j its rank in its cell.
template <typename F>
__device__ __forceinline__ void si_walk(const int32_t* cs, const int32_t* items, const gf_keypoint* K2, int cx0,
                                        int cy0, int ncy, int nc, float x, float y, float r, int lane, F&& f) {
    for (int c = lane; c < nc; c += SI_T) {
        const int cell = (cx0 + c / ncy) * GRID_ROWS + cy0 + c % ncy;
        const int s = cs[cell], e = cs[cell + 1];
        for (int j = s; j < e; j++) {
            const int idx = items[j];
            const gf_keypoint k = K2[idx];
            if (fabsf(k.x - x) > r || fabsf(k.y - y) > r) continue;
            f(idx, c, j - s);
        }
    }
}

__global__ __launch_bounds__(SI_T* SI_QW) void k_si_cand(SIArgs A) {
    const int p = blockIdx.y, lane = threadIdx.x & 63;
    const int i1 = (int)blockIdx.x * SI_QW + (int)(threadIdx.x >> 6);
    if (i1 >= A.cap1) return;  // wave-uniform
    const int n1 = clampn(A.n1[p], A.cap1), n2 = clampn(A.n2[p], A.cap2);
    int32_t* cnt = A.cnt + (size_t)p * A.cap1 + i1;
    const size_t q = (size_t)p * A.cap1 + min(i1, max(n1 - 1, 0));  // cap1 >= 1: row 0 exists
    const gf_keypoint k1 = A.K1[q];
    const float x = A.prev[2 * q], y = A.prev[2 * q + 1];
    const uint4* pd = (const uint4*)(A.D1 + 32 * q);
    const uint4 a0 = pd[0], a1 = pd[1];
    int cx0 = 0, cx1 = 0, cy0 = 0, cy1 = 0;
    const bool win = grid_window(A.fc, x, y, A.window, cx0, cx1, cy0, cy1);
    if (!(i1 < n1 && k1.octave == 0 && n2 > 0 && win)) {
        if (lane == 0) *cnt = 0;
        return;
    }
    if (A.direct) {
        if (lane == 0) *cnt = SI_FLAG;
        return;
    }
    const int32_t* cs = A.grid + (size_t)p * si_grid_ints(A.cap2);
    const int32_t* items = cs + NCELLS + 1;
    const gf_keypoint* K2 = A.K2 + (size_t)p * A.cap2;
    const uint8_t* D2 = A.D2 + 32 * (size_t)p * A.cap2;
    int32_t* out = A.cand + ((size_t)p * A.cap1 + i1) * SI_CAP;
    const int ncy = cy1 - cy0 + 1, nc = (cx1 - cx0 + 1) * ncy;
    const float r = A.window;
    int base = 0;
    for (int c0 = 0; c0 < nc && base <= SI_CAP; c0 += SI_T) {
        const int c = c0 + lane, cc = min(c, nc - 1);
        const int cell = (cx0 + cc / ncy) * GRID_ROWS + cy0 + cc % ncy;
        const int s = cs[cell], e0 = cs[cell + 1], e = c < nc ? e0 : s;
        int k = 0;
        for (int j = s; j < e; j++) {
            const gf_keypoint kp = K2[items[j]];
            k += !(fabsf(kp.x - x) > r || fabsf(kp.y - y) > r);
        }
        int incl = k;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int v = __shfl_up(incl, o, 64);
            if (lane >= o) incl += v;
        }
        int pos = base + incl - k;
        base += __shfl(incl, 63, 64);
        if (k) {
            for (int j = s; j < e; j++) {
                const int idx = items[j];
                const gf_keypoint kp = K2[idx];
                const uint4* pb = (const uint4*)(D2 + 32 * (size_t)idx);
                const int d = hamming_regs(a0, a1, pb[0], pb[1]);
                const bool in = !(fabsf(kp.x - x) > r || fabsf(kp.y - y) > r);
                if (in && pos < SI_CAP) out[pos] = (idx << 9) | d;
                pos += in;
            }
        }
    }
    if (lane == 0) *cnt = base > SI_CAP ? SI_FLAG : base;
}

__global__ __launch_bounds__(SI_T) void k_si_resolve(SIArgs A) {
    __shared__ unsigned short s_md[KP_MAX];  // vMatchedDistance, 0xffff = INT_MAX
    __shared__ short s_21[KP_MAX];           // vnMatches21
    __shared__ short s_12[KP_MAX];           // vnMatches12, filled at the end
    __shared__ int s_rec[KP_MAX];            // accepts in order: bin << 24 | i1 << 12 | i2
    __shared__ int s_hist[HISTO_LENGTH], s_keep[3];
    const int p = blockIdx.x, lane = threadIdx.x;
    const int n1 = clampn(A.n1[p], A.cap1), n2 = clampn(A.n2[p], A.cap2);
    const gf_keypoint* K1 = A.K1 + (size_t)p * A.cap1;
    const gf_keypoint* K2 = A.K2 + (size_t)p * A.cap2;
    const uint8_t* D1 = A.D1 + 32 * (size_t)p * A.cap1;
    const uint8_t* D2 = A.D2 + 32 * (size_t)p * A.cap2;
    float* prev = A.prev + 2 * (size_t)p * A.cap1;
    const int32_t* cnt = A.cnt + (size_t)p * A.cap1;
    const int32_t* cand = A.cand + (size_t)p * A.cap1 * SI_CAP;
    const int32_t* cs = A.grid + (size_t)p * si_grid_ints(A.cap2);
    const int32_t* items = cs + NCELLS + 1;
    for (int i = lane; i < KP_MAX; i += SI_T) {
        s_md[i] = 0xffff;
        s_21[i] = -1;
        s_12[i] = -1;
    }
    __syncthreads();
    int nrec = 0;
    int cn = cnt[min(lane, A.cap1 - 1)];
    if (lane >= n1) cn = 0;
    // under GF_SI_DIRECT no list exists: the list loads read the scratch's first row and are not used
    const size_t lrow = A.direct ? 0 : SI_CAP;
    for (int b0 = 0; b0 < n1; b0 += SI_T) {
        const int c = cn;
        {  // the next 64 counts, before this chunk's walk
            const int i = b0 + SI_T + lane;
            cn = cnt[min(i, A.cap1 - 1)];
            if (i >= n1) cn = 0;
        }
        unsigned long long todo = __ballot(c != 0);
        // the first list of the chunk; then each query loads the next one's before its own reduction
        int l = todo ? __ffsll((long long)todo) - 1 : 0;
        int v = cand[(size_t)min(b0 + l, A.cap1 - 1) * lrow + lane];
        while (todo) {
            todo &= todo - 1;
            const int i1 = b0 + l, ci = __builtin_amdgcn_readfirstlane(__shfl(c, l, 64)), vc = v;
            l = todo ? __ffsll((long long)todo) - 1 : l;
            v = cand[(size_t)min(b0 + l, A.cap1 - 1) * lrow + lane];
            Top2 t = top2_init();
            if (ci <= SI_CAP) {
                const int idx = (vc >> 9) & (KP_MAX - 1), d = vc & 511;
                if (lane < ci && (int)s_md[idx] > d) t = Top2{d, lane, idx, INT_MAX};
            } else {
                const float x = prev[2 * i1], y = prev[2 * i1 + 1];
                const uint4* pa = (const uint4*)(D1 + 32 * (size_t)i1);
                const uint4 a0 = pa[0], a1 = pa[1];
                int cx0 = 0, cx1 = 0, cy0 = 0, cy1 = 0;
                if (grid_window(A.fc, x, y, A.window, cx0, cx1, cy0, cy1)) {
                    const int ncy = cy1 - cy0 + 1, nc = (cx1 - cx0 + 1) * ncy;
                    si_walk(cs, items, K2, cx0, cy0, ncy, nc, x, y, A.window, lane, [&](int idx, int cc, int j) {
                        const uint4* pb = (const uint4*)(D2 + 32 * (size_t)idx);
                        const int d = hamming_regs(a0, a1, pb[0], pb[1]);
                        if ((int)s_md[idx] <= d) return;
                        top2_push(t, d, (cc << 12) | j, idx);
                    });
                }
            }
            t = top2_reduce(t);
            // the same in every lane after the reduction; read from lane 0 so that the branch is scalar
            if (__builtin_amdgcn_readfirstlane((int)(t.d1 <= SI_TH_LOW && (float)t.d1 < (float)t.d2 * A.nnratio))) {
                if (lane == 0) {  // the steal is the overwrite: vnMatches12 is read off vnMatches21 at the end
                    s_21[t.i1] = (short)i1;
                    s_md[t.i1] = (unsigned short)t.d1;
                    s_rec[nrec] = (i1 << 12) | t.i1;
                }
                nrec++;
                __syncthreads();
            }
        }
    }
    __syncthreads();
    if (A.check_ori) {
        for (int i = lane; i < HISTO_LENGTH; i += SI_T) s_hist[i] = 0;
        __syncthreads();
        for (int r = lane; r < nrec; r += SI_T) {  // every accept counts, also one robbed later
            const int rec = s_rec[r], i1 = rec >> 12, i2 = rec & (KP_MAX - 1);
            // angles of the extractor lie in [0, 360): bins 0..12; anything else trips the reference's ROS_ASSERT
            const int bin = min(max(rot_bin(K1[i1].angle, K2[i2].angle), 0), HISTO_LENGTH - 1);
            s_rec[r] = rec | (bin << 24);
            atomicAdd(&s_hist[bin], 1);
        }
        __syncthreads();
        if (lane == 0) three_maxima(s_hist, s_keep);
        __syncthreads();
        for (int r = lane; r < nrec; r += SI_T) {
            const int rec = s_rec[r], bin = rec >> 24, i1 = (rec >> 12) & (KP_MAX - 1), i2 = rec & (KP_MAX - 1);
            if (bin == s_keep[0] || bin == s_keep[1] || bin == s_keep[2]) continue;
            if (s_21[i2] == i1) s_21[i2] = -1;  // a robbed query is at -1 already
        }
        __syncthreads();
    }
    int nm = 0;
    for (int i = lane; i < n2; i += SI_T) {
        const int o = s_21[i];
        if (o >= 0) {
            s_12[o] = (short)i;
            nm++;
        }
    }
    nm = gfd::warp_sum(nm);
    __syncthreads();
    int32_t* m12 = A.m12 + (size_t)p * A.cap1;
    for (int i = lane; i < A.cap1; i += SI_T) {
        const int m = i < n1 ? s_12[i] : -1;
        const gf_keypoint k2 = K2[max(m, 0)];  // cap2 >= 1
        m12[i] = m;
        if (m >= 0) {
            prev[2 * i] = k2.x;
            prev[2 * i + 1] = k2.y;
        }
    }
    if (lane == 0) A.nm[p] = nm;
}

// Tracking::Initialize (Tracking.cc:999-1017) after the matcher has run.
__global__ __launch_bounds__(SI_GRID_T) void k_si_gate(const int32_t* n2, int cap1, int thres, const float* prev_before,
                                                      float* prev, int32_t* m12, int32_t* nm, int32_t* status,
                                                      int32_t* init_m12) {
    const int p = blockIdx.x;
    const bool few_kp = n2[p] <= thres;
    const int st = few_kp ? GF_SI_FEW_KEYPOINTS : nm[p] < thres ? GF_SI_FEW_MATCHES : GF_SI_OK;
    for (int i = threadIdx.x; i < cap1; i += SI_GRID_T) {
        const size_t q = (size_t)p * cap1 + i;
        const int m = m12[q];
        const float bx = prev_before[2 * q], by = prev_before[2 * q + 1];
        if (few_kp) {  // the reference returns before the matcher: fill(mvIniMatches, -1), mvbPrevMatched kept
            m12[q] = -1;
            prev[2 * q] = bx;
            prev[2 * q + 1] = by;
        }
        init_m12[q] = st == GF_SI_OK ? m : -1;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        status[p] = st;
        if (few_kp) nm[p] = 0;
    }
}

int check_fi(const gf_frame_info* fi) {
    GF_CHECK(fi && fi->nlevels >= 1 && fi->nlevels <= 16 && fi->max_x > fi->min_x && fi->max_y > fi->min_y, GF_ERR_ARG,
             "bad frame info");
    return GF_OK;
}

}  // namespace

extern "C" {

int gf_search_for_initialization_batch_dev(gf_ctx* ctx, const gf_frame_info* fi, int nprob, const gf_keypoint* d_kps1,
                                           const uint8_t* d_desc1, int cap1, const int32_t* d_n1,
                                           const gf_keypoint* d_kps2, const uint8_t* d_desc2, int cap2,
                                           const int32_t* d_n2, int window, float nnratio, int check_ori, int flags,
                                           float* d_prev_matched, int32_t* d_matches12, int32_t* d_nmatches,
                                           void* stream) {
    GF_CHECK(ctx, GF_ERR_ARG, "null ctx");
    int rc = check_fi(fi);
    if (rc) return rc;
    if (nprob <= 0) return GF_OK;
    GF_CHECK(cap1 >= 1 && cap2 >= 1 && cap1 <= KP_MAX && cap2 <= KP_MAX, GF_ERR_UNSUPPORTED,
             "a frame holds 1 to 4096 keypoint rows");
    GF_CHECK(d_kps1 && d_desc1 && d_n1 && d_kps2 && d_desc2 && d_n2 && d_prev_matched && d_matches12 && d_nmatches,
             GF_ERR_ARG, "null arg");
    GF_CHECK(window >= 0 && (flags & ~GF_SI_DIRECT) == 0, GF_ERR_ARG, "bad window or flags");
    hipStream_t s = (hipStream_t)stream;
    const bool direct = flags & GF_SI_DIRECT;
    void *g, *c, *l;
    if ((rc = gf::ws_get(ctx, 21, sizeof(int32_t) * si_grid_ints(cap2) * nprob, &g)) ||
        (rc = gf::ws_get(ctx, 22, sizeof(int32_t) * (size_t)cap1 * nprob, &c)) ||
        (rc = gf::ws_get(ctx, 23, direct ? 256 : sizeof(int32_t) * (size_t)cap1 * SI_CAP * nprob, &l)))
        return rc;
    SIArgs A{};
    A.fc = gf::make_frame_const(fi);
    A.K1 = d_kps1;
    A.D1 = d_desc1;
    A.n1 = d_n1;
    A.cap1 = cap1;
    A.K2 = d_kps2;
    A.D2 = d_desc2;
    A.n2 = d_n2;
    A.cap2 = cap2;
    A.prev = d_prev_matched;
    A.m12 = d_matches12;
    A.nm = d_nmatches;
    A.window = (float)window;
    A.nnratio = nnratio;
    A.check_ori = check_ori;
    A.direct = direct;
    A.grid = (int32_t*)g;
    A.cnt = (int32_t*)c;
    A.cand = (int32_t*)l;
    {
        GF_PROF(ctx, s, "k_si_grid");
        GF_LAUNCH(k_si_grid, nprob, SI_GRID_T, 0, s, A);
    }
    {
        GF_PROF(ctx, s, direct ? "k_si_cand_direct" : "k_si_cand");
        GF_LAUNCH(k_si_cand, dim3((cap1 + SI_QW - 1) / SI_QW, nprob), SI_T * SI_QW, 0, s, A);
    }
    {
        GF_PROF(ctx, s, direct ? "k_si_resolve_direct" : "k_si_resolve");
        GF_LAUNCH(k_si_resolve, nprob, SI_T, 0, s, A);
    }
    GF_HIP(hipGetLastError());
    return GF_OK;
}

int gf_tracking_initialize_gate_dev(gf_ctx* ctx, int nprob, const int32_t* d_n2, int cap1, int thres,
                                    const float* d_prev_before, float* d_prev_matched, int32_t* d_matches12,
                                    int32_t* d_nmatches, int32_t* d_status, int32_t* d_init_matches12, void* stream) {
    GF_CHECK(ctx, GF_ERR_ARG, "null ctx");
    if (nprob <= 0) return GF_OK;
    GF_CHECK(cap1 >= 1 && d_n2 && d_prev_before && d_prev_matched && d_matches12 && d_nmatches && d_status &&
                 d_init_matches12,
             GF_ERR_ARG, "null arg");
    hipStream_t s = (hipStream_t)stream;
    GF_PROF(ctx, s, "k_si_gate");
    GF_LAUNCH(k_si_gate, nprob, SI_GRID_T, 0, s, d_n2, cap1, thres, d_prev_before, d_prev_matched, d_matches12,
              d_nmatches, d_status, d_init_matches12);
    GF_HIP(hipGetLastError());
    return GF_OK;
}

int gf_search_for_initialization(gf_ctx* ctx, const gf_frame_info* fi, const gf_keypoint* kps1, const uint8_t* desc1,
                                 int n1, const gf_keypoint* kps2, const uint8_t* desc2, int n2, int window,
                                 float nnratio, int check_ori, int flags, float* prev_matched, int32_t* matches12,
                                 int* nmatches) {
    GF_CHECK(ctx && nmatches, GF_ERR_ARG, "null arg");
    GF_CHECK(n1 >= 0 && n1 <= KP_MAX && (n1 == 0 || (kps1 && desc1 && prev_matched && matches12)), GF_ERR_ARG,
             "bad first frame");
    GF_CHECK(n2 >= 0 && n2 <= KP_MAX && (n2 == 0 || (kps2 && desc2)), GF_ERR_ARG, "bad second frame");
    GF_HIP(hipSetDevice(ctx->device));
    const int c1 = std::max(n1, 1), c2 = std::max(n2, 1);
    void *k1, *d1, *k2, *d2, *pv, *m, *cn;
    int rc;
    if ((rc = gf::ws_get(ctx, 0, sizeof(gf_keypoint) * c1, &k1)) || (rc = gf::ws_get(ctx, 1, 32 * (size_t)c1, &d1)) ||
        (rc = gf::ws_get(ctx, 2, sizeof(gf_keypoint) * c2, &k2)) || (rc = gf::ws_get(ctx, 3, 32 * (size_t)c2, &d2)) ||
        (rc = gf::ws_get(ctx, 4, 8 * (size_t)c1, &pv)) || (rc = gf::ws_get(ctx, 5, 4 * (size_t)c1, &m)) ||
        (rc = gf::ws_get(ctx, 6, 12, &cn)))
        return rc;
    hipStream_t s = ctx->stream;
    const int32_t counts[3] = {n1, n2, 0};
    GF_HIP(hipMemcpyAsync(cn, counts, 12, hipMemcpyHostToDevice, s));
    if (n1) {
        GF_HIP(hipMemcpyAsync(k1, kps1, sizeof(gf_keypoint) * n1, hipMemcpyHostToDevice, s));
        GF_HIP(hipMemcpyAsync(d1, desc1, 32 * (size_t)n1, hipMemcpyHostToDevice, s));
        GF_HIP(hipMemcpyAsync(pv, prev_matched, 8 * (size_t)n1, hipMemcpyHostToDevice, s));
    }
    if (n2) {
        GF_HIP(hipMemcpyAsync(k2, kps2, sizeof(gf_keypoint) * n2, hipMemcpyHostToDevice, s));
        GF_HIP(hipMemcpyAsync(d2, desc2, 32 * (size_t)n2, hipMemcpyHostToDevice, s));
    }
    int32_t* dc = (int32_t*)cn;
    rc = gf_search_for_initialization_batch_dev(ctx, fi, 1, (const gf_keypoint*)k1, (const uint8_t*)d1, c1, dc,
                                                (const gf_keypoint*)k2, (const uint8_t*)d2, c2, dc + 1, window,
                                                nnratio, check_ori, flags, (float*)pv, (int32_t*)m, dc + 2, s);
    if (rc) return rc;
    int32_t nm = 0;
    if (n1) {
        GF_HIP(hipMemcpyAsync(matches12, m, 4 * (size_t)n1, hipMemcpyDeviceToHost, s));
        GF_HIP(hipMemcpyAsync(prev_matched, pv, 8 * (size_t)n1, hipMemcpyDeviceToHost, s));
    }
    GF_HIP(hipMemcpyAsync(&nm, dc + 2, 4, hipMemcpyDeviceToHost, s));
    GF_HIP(hipStreamSynchronize(s));
    *nmatches = nm;
    return GF_OK;
}

}  // extern "C"
