// The graph assembly of Optimizer::LocalBundleAdjustment (src/Optimizer.cc:
// 1517-1675) over the flat map tables of kfcull.hip, without a sort and without
// an atomic whose result depends on arrival order:
//
//   k_lba_setup: the walk. Slot i of the j-th local keyframe has the position
//     w = (keypoint counts of the local keyframes before j) + i, which is the
//     order in which :1534-1548 meets the slots.
//   k_lba_mark: atomicMin(first[p], w) over the slots with a live point: an
//     integer minimum is the same whatever the arrival order. The position
//     with first[p] == w owns p: it is where p enters lLocalMapPoints.
//   k_lba_rows: every owner counts the live entries of its point's row (:1644)
//     and marks the observers that are not local as fixed cameras (:1552-1566;
//     plain byte stores of the same value). The keyframe of a global keypoint
//     index is found by binary search in kf_off.
//   k_lba_scan: exclusive scans over the walk positions (edge offsets), the
//     point plane (problem point index) and the keyframe plane (problem
//     keyframe index), one workgroup each; the totals are the three counts.
//   k_lba_vertices: the keyframe and point arrays, gathered.
//   k_lba_edges: every owner writes its row at its offset (:1640-1674).
//
// Every id is bounds-tested where it is read (a slot against [0, nmp), a row
// against [0, nobs), an entry against [0, nkp)) and skipped like a tombstone.
#include <vector>

#include "common.h"

#define LG_THREADS 256
#define LG_BATCH 8
#define LG_MAX_KP 4096
#define LG_MAX_LOCAL 33  // 32 keyframes of kind 0 (the solver's limit) and the first keyframe
#define LG_SCAN 1024
#define LG_NONE 0x7f7f7f7f  // first[] after the byte clear: above every walk position

namespace {

typedef float lg_f2 __attribute__((ext_vector_type(2)));
typedef float lg_f4 __attribute__((ext_vector_type(4)));

struct LgLocal {
    int n;
    int kf[LG_MAX_LOCAL];
};

struct LgWork {
    int32_t* first;    // nmp: lowest walk position of the point
    uint8_t* is_local; // nkf
    uint8_t* is_fixed; // nkf
    int32_t* woff;     // LG_MAX_LOCAL + 1: walk offsets of the local keyframes
    int32_t* cnt;      // wcap: live row entries of an owner, 0 elsewhere
    int32_t* eoff;     // wcap: exclusive scan of cnt
    int32_t* pidx;     // nmp: problem index of a local point
    int32_t* kidx;     // nkf: problem index of a problem keyframe
};

__global__ __launch_bounds__(64) void k_lba_setup(gf_lba_tables T, LgLocal L, LgWork W) {
    const int j = threadIdx.x;
    int n = 0;
    if (j < L.n) {
        const int k = L.kf[j];
        const int s0 = min(max(gfd::ldg(T.kf_off + k), 0), T.nkp);
        const int s1 = min(max(gfd::ldg(T.kf_off + k + 1), s0), T.nkp);
        n = min(s1 - s0, LG_MAX_KP);
        W.is_local[k] = 1;
    }
    int inc = n;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(inc, o, 64);
        if (j >= o) inc += v;
    }
    if (j < L.n) W.woff[j] = inc - n;
    if (j == L.n - 1) W.woff[L.n] = inc;
}

// the walk position and slot of this lane: false outside the keyframe
__device__ __forceinline__ bool lg_slot(const gf_lba_tables& T, const LgLocal& L, const LgWork& W, int& w, int& g) {
    const int j = blockIdx.y, i = blockIdx.x * LG_THREADS + threadIdx.x;
    const int w0 = gfd::ldg(W.woff + j), w1 = gfd::ldg(W.woff + j + 1);
    const int s0 = min(max(gfd::ldg(T.kf_off + L.kf[j]), 0), T.nkp);
    w = w0 + i;
    g = s0 + i;
    return i < w1 - w0;
}

__global__ __launch_bounds__(LG_THREADS) void k_lba_mark(gf_lba_tables T, LgLocal L, LgWork W) {
    int w, g;
    if (!lg_slot(T, L, W, w, g)) return;
    const int p = gfd::ldg(T.slots + g);
    if (p < 0 || p >= T.nmp) return;       // pMP (:1540), or an id past the map
    if (gfd::ldg(T.mp_bad + p)) return;    // :1541
    atomicMin(W.first + p, w);
}

// the keyframe of global keypoint index g in [0, nkp): the last k with kf_off[k] <= g
__device__ __forceinline__ void lg_find_kf(const int32_t* __restrict__ kf_off, int nkf, const int (&g)[LG_BATCH],
                                           int (&kf)[LG_BATCH]) {
    int lo[LG_BATCH], hi[LG_BATCH];
#pragma unroll
    for (int j = 0; j < LG_BATCH; j++) lo[j] = 0, hi[j] = nkf;  // kf_off[lo] <= g < kf_off[hi]
    for (int span = nkf; span > 1; span = (span + 1) >> 1) {
        int mid[LG_BATCH], v[LG_BATCH];
#pragma unroll
        for (int j = 0; j < LG_BATCH; j++) {
            mid[j] = (lo[j] + hi[j]) >> 1;
            v[j] = gfd::ldg(kf_off + mid[j]);
        }
#pragma unroll
        for (int j = 0; j < LG_BATCH; j++) {
            if (hi[j] - lo[j] > 1) {
                if (v[j] <= g[j]) lo[j] = mid[j];
                else hi[j] = mid[j];
            }
        }
    }
#pragma unroll
    for (int j = 0; j < LG_BATCH; j++) kf[j] = lo[j];
}

// one batch of row [r, r1): the entries, their keyframes and whether each is a live edge (:1644)
__device__ __forceinline__ void lg_batch(const gf_lba_tables& T, int r, int r1, int (&g)[LG_BATCH], int (&kf)[LG_BATCH],
                                         bool (&live)[LG_BATCH]) {
    int gs[LG_BATCH];
#pragma unroll
    for (int j = 0; j < LG_BATCH; j++) g[j] = r + j < r1 ? gfd::ldg(T.obs_gkp + r + j) : -1;
#pragma unroll
    for (int j = 0; j < LG_BATCH; j++) {
        if (g[j] >= T.nkp) g[j] = -1;
        gs[j] = max(g[j], 0);
    }
    lg_find_kf(T.kf_off, T.nkf, gs, kf);
    uint8_t bad[LG_BATCH];
#pragma unroll
    for (int j = 0; j < LG_BATCH; j++) bad[j] = gfd::ldg(T.kf_bad + kf[j]);
#pragma unroll
    for (int j = 0; j < LG_BATCH; j++) live[j] = g[j] >= 0 && !bad[j];
}

// the point this position owns, with its row: -1 when it owns none
__device__ __forceinline__ int lg_owned(const gf_lba_tables& T, const LgWork& W, int w, int g, int& r0, int& r1) {
    const int p = gfd::ldg(T.slots + g);
    if (p < 0 || p >= T.nmp) return -1;
    const int bad = gfd::ldg(T.mp_bad + p), f = gfd::ldg(W.first + p);
    r0 = min(max(gfd::ldg(T.obs_off + p), 0), T.nobs);
    r1 = min(max(gfd::ldg(T.obs_off + p + 1), r0), T.nobs);
    return !bad && f == w ? p : -1;
}

__global__ __launch_bounds__(LG_THREADS) void k_lba_rows(gf_lba_tables T, LgLocal L, LgWork W) {
    int w, g;
    if (!lg_slot(T, L, W, w, g)) return;
    int r0 = 0, r1 = 0, n = 0;
    if (lg_owned(T, W, w, g, r0, r1) >= 0) {
        for (int r = r0; r < r1; r += LG_BATCH) {
            int e[LG_BATCH], kf[LG_BATCH];
            bool live[LG_BATCH];
            lg_batch(T, r, r1, e, kf, live);
            uint8_t loc[LG_BATCH];
#pragma unroll
            for (int j = 0; j < LG_BATCH; j++) loc[j] = gfd::ldg(W.is_local + kf[j]);
#pragma unroll
            for (int j = 0; j < LG_BATCH; j++) {
                n += live[j];
                if (live[j] && !loc[j]) W.is_fixed[kf[j]] = 1;  // lFixedCameras (:1559-1563)
            }
        }
    }
    W.cnt[w] = n;
}

// Exclusive scans, one workgroup each: 0 = cnt over the walk -> eoff and
// nedges, 1 = local points over the point plane -> pidx and npts, 2 = problem
// keyframes over the keyframe plane -> kidx and nkf.
__global__ __launch_bounds__(LG_SCAN) void k_lba_scan(gf_lba_tables T, LgLocal L, LgWork W, int32_t* __restrict__ counts) {
    __shared__ int wsum[LG_SCAN / 64];
    const int which = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int n = which == 0 ? gfd::ldg(W.woff + L.n) : which == 1 ? T.nmp : T.nkf;
    int32_t* out = which == 0 ? W.eoff : which == 1 ? W.pidx : W.kidx;
    int carry = 0;
    for (int base = 0; base < n; base += LG_SCAN) {
        const int i = base + tid;
        int v = 0;
        if (i < n) {
            if (which == 0) v = gfd::ldg(W.cnt + i);
            else if (which == 1) v = gfd::ldg(W.first + i) != LG_NONE;
            else v = (gfd::ldg(W.is_local + i) | gfd::ldg(W.is_fixed + i)) != 0;
        }
        int inc = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int u = __shfl_up(inc, o, 64);
            if (lane >= o) inc += u;
        }
        if (lane == 63) wsum[wv] = inc;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int q = 0; q < LG_SCAN / 64; q++) {
            const int s = wsum[q];
            before += q < wv ? s : 0;
            total += s;
        }
        if (i < n) out[i] = carry + before + inc - v;
        carry += total;
        __syncthreads();
    }
    if (tid == 0) counts[2 - which] = carry;  // nkf, npts, nedges
}

__global__ __launch_bounds__(LG_THREADS) void k_lba_vertices(gf_lba_tables T, LgWork W, gf_lba_graph_out O) {
    const int t = blockIdx.x * LG_THREADS + threadIdx.x;
    if (t < T.nmp) {
        const int f = gfd::ldg(W.first + t), q = gfd::ldg(W.pidx + t);
        const float x = gfd::ldg(T.mp_pos + 3 * (size_t)t), y = gfd::ldg(T.mp_pos + 3 * (size_t)t + 1),
                    z = gfd::ldg(T.mp_pos + 3 * (size_t)t + 2);
        if (f != LG_NONE && q >= 0 && q < T.nmp) {
            O.prob_pt[q] = t;
            O.pt_pos[3 * (size_t)q] = x;
            O.pt_pos[3 * (size_t)q + 1] = y;
            O.pt_pos[3 * (size_t)q + 2] = z;
        }
    }
    if (t < T.nkf) {
        const int loc = gfd::ldg(W.is_local + t), fix = gfd::ldg(W.is_fixed + t), q = gfd::ldg(W.kidx + t);
        if ((loc | fix) && q >= 0 && q < T.nkf) {
            const lg_f4* src = (const lg_f4*)(T.kf_Tcw + 16 * (size_t)t);
            const lg_f4 a = gfd::ldg(src), b = gfd::ldg(src + 1), c = gfd::ldg(src + 2), d = gfd::ldg(src + 3);
            lg_f4* dst = (lg_f4*)(O.kf_Tcw + 16 * (size_t)q);
            dst[0] = a, dst[1] = b, dst[2] = c, dst[3] = d;
            *(lg_f4*)(O.kf_cam + 4 * (size_t)q) = (lg_f4){T.cam[0], T.cam[1], T.cam[2], T.cam[3]};
            O.prob_kf[q] = t;
            O.kf_kind[q] = loc ? (t == T.kf0 ? 1 : 0) : 2;  // vSE3->setFixed(mnId == 0) (:1591); lFixedCameras
        }
    }
}

__global__ __launch_bounds__(LG_THREADS) void k_lba_edges(gf_lba_tables T, LgLocal L, LgWork W, gf_lba_graph_out O) {
    int w, g;
    if (!lg_slot(T, L, W, w, g)) return;
    int r0 = 0, r1 = 0;
    const int p = lg_owned(T, W, w, g, r0, r1);
    if (p < 0) return;
    int e = gfd::ldg(W.eoff + w);
    const int pq = gfd::ldg(W.pidx + p);
    for (int r = r0; r < r1; r += LG_BATCH) {
        int en[LG_BATCH], kf[LG_BATCH], kq[LG_BATCH], lev[LG_BATCH];
        bool live[LG_BATCH];
        lg_f2 z[LG_BATCH];
        lg_batch(T, r, r1, en, kf, live);
#pragma unroll
        for (int j = 0; j < LG_BATCH; j++) {
            const int gs = max(en[j], 0);
            kq[j] = gfd::ldg(W.kidx + kf[j]);
            lev[j] = min((int)gfd::ldg(T.octave + gs), T.nlevels - 1);
            z[j] = gfd::ldg((const lg_f2*)T.kp_xy + gs);
        }
        float s2[LG_BATCH];
#pragma unroll
        for (int j = 0; j < LG_BATCH; j++) s2[j] = gfd::ldg(T.inv_sigma2 + lev[j]);
#pragma unroll
        for (int j = 0; j < LG_BATCH; j++) {
            if (!live[j] || e < 0 || e >= T.nobs) continue;
            O.edge_pt[e] = pq;
            O.edge_kf[e] = kq[j];
            *((lg_f2*)O.edge_z + e) = z[j];  // kpUn.pt (:1647-1648)
            O.edge_inv_sigma2[e] = s2[j];     // GetInvSigma2(kpUn.octave) (:1656)
            O.edge_gkp[e] = en[j];
            e++;
        }
    }
}

int check_local(const gf_lba_tables* T, int nlocal, const int32_t* local, LgLocal* L) {
    GF_CHECK(T->nkf >= 0 && T->nkp >= 0 && T->nmp >= 0 && T->nobs >= 0, GF_ERR_ARG, "gf_lba_graph: negative size");
    GF_CHECK(T->nlevels >= 1 && T->nlevels <= 16, GF_ERR_ARG, "gf_lba_graph: nlevels outside [1, 16]");
    GF_CHECK(T->kf0 >= -1 && T->kf0 < T->nkf, GF_ERR_ARG, "gf_lba_graph: kf0 outside [-1, nkf)");
    GF_CHECK(nlocal >= 1 && local, GF_ERR_ARG, "gf_lba_graph: the local list holds at least the current keyframe");
    int nfree = 0;
    for (int j = 0; j < nlocal; j++) {
        GF_CHECK(local[j] >= 0 && local[j] < T->nkf, GF_ERR_ARG, "gf_lba_graph: local keyframe outside [0, nkf)");
        for (int i = 0; i < j; i++) GF_CHECK(local[i] != local[j], GF_ERR_ARG, "gf_lba_graph: local keyframe listed twice");
        nfree += local[j] != T->kf0;
        GF_CHECK(nfree <= 32, GF_ERR_ARG, "gf_lba_graph: more than 32 local (non-fixed) keyframes");
    }
    L->n = nlocal;  // at most 32 + the first keyframe
    for (int j = 0; j < LG_MAX_LOCAL; j++) L->kf[j] = j < nlocal ? local[j] : 0;
    return GF_OK;
}

size_t up16(size_t b) { return (b + 15) & ~(size_t)15; }

}  // namespace

extern "C" {

// Optimizer.cc:1517-1675 on device tables: the gather, the vertices and the edges
int gf_lba_graph_dev(gf_ctx* ctx, const gf_lba_tables* d_tables, int nlocal, const int32_t* local,
                     const gf_lba_graph_out* d_out, void* stream) {
    GF_CHECK(ctx && d_tables && d_out, GF_ERR_ARG, "gf_lba_graph_dev: null arg");
    const gf_lba_tables& T = *d_tables;
    const gf_lba_graph_out& O = *d_out;
    LgLocal L;
    int rc = check_local(d_tables, nlocal, local, &L);
    if (rc) return rc;
    GF_CHECK(T.kf_off && T.kf_bad && T.kf_Tcw && T.inv_sigma2, GF_ERR_ARG, "gf_lba_graph_dev: null keyframe table");
    GF_CHECK(T.nkp == 0 || (T.octave && T.slots && T.kp_xy), GF_ERR_ARG, "gf_lba_graph_dev: null keypoint table");
    GF_CHECK(T.nmp == 0 || (T.mp_bad && T.mp_pos && T.obs_off), GF_ERR_ARG, "gf_lba_graph_dev: null point table");
    GF_CHECK(T.nobs == 0 || T.obs_gkp, GF_ERR_ARG, "gf_lba_graph_dev: null observation table");
    GF_CHECK(O.counts && O.prob_kf && O.kf_kind && O.kf_Tcw && O.kf_cam, GF_ERR_ARG, "gf_lba_graph_dev: null output");
    GF_CHECK(T.nmp == 0 || (O.prob_pt && O.pt_pos), GF_ERR_ARG, "gf_lba_graph_dev: null point output");
    GF_CHECK(T.nobs == 0 || (O.edge_pt && O.edge_kf && O.edge_z && O.edge_inv_sigma2 && O.edge_gkp), GF_ERR_ARG,
             "gf_lba_graph_dev: null edge output");
    // workspace: [first | woff | cnt | eoff | pidx | kidx | is_local | is_fixed]; the last two are cleared, first is
    // set to LG_NONE
    const size_t NK = (size_t)T.nkf, NM = (size_t)T.nmp;
    const size_t wcap = (size_t)nlocal * LG_MAX_KP;  // every keyframe is walked up to LG_MAX_KP slots
    const size_t o_first = 0, o_woff = o_first + up16(4 * NM), o_cnt = o_woff + up16(4 * (LG_MAX_LOCAL + 1)),
                 o_eoff = o_cnt + up16(4 * wcap), o_pidx = o_eoff + up16(4 * wcap), o_kidx = o_pidx + up16(4 * NM),
                 o_loc = o_kidx + up16(4 * NK), o_fix = o_loc + up16(NK), total = o_fix + up16(NK);
    void* dbuf;
    rc = gf::ws_get(ctx, 70, total, &dbuf);
    if (rc) return rc;
    uint8_t* base = (uint8_t*)dbuf;
    LgWork W;
    W.first = (int32_t*)(base + o_first);
    W.woff = (int32_t*)(base + o_woff);
    W.cnt = (int32_t*)(base + o_cnt);
    W.eoff = (int32_t*)(base + o_eoff);
    W.pidx = (int32_t*)(base + o_pidx);
    W.kidx = (int32_t*)(base + o_kidx);
    W.is_local = base + o_loc;
    W.is_fixed = base + o_fix;
    hipStream_t s = (hipStream_t)stream;
    if (NM) GF_HIP(hipMemsetAsync(W.first, 0x7f, 4 * NM, s));
    GF_HIP(hipMemsetAsync(W.is_local, 0, (o_fix - o_loc) + up16(NK), s));
    GF_PROF(ctx, s, "k_lba_graph");
    const dim3 walk(LG_MAX_KP / LG_THREADS, nlocal);
    GF_LAUNCH(k_lba_setup, 1, 64, 0, s, T, L, W);
    GF_LAUNCH(k_lba_mark, walk, LG_THREADS, 0, s, T, L, W);
    GF_LAUNCH(k_lba_rows, walk, LG_THREADS, 0, s, T, L, W);
    GF_LAUNCH(k_lba_scan, 3, LG_SCAN, 0, s, T, L, W, O.counts);
    const int nv = std::max(T.nmp, T.nkf);
    GF_LAUNCH(k_lba_vertices, (nv + LG_THREADS - 1) / LG_THREADS, LG_THREADS, 0, s, T, W, O);
    GF_LAUNCH(k_lba_edges, walk, LG_THREADS, 0, s, T, L, W, O);
    GF_HIP(hipGetLastError());
    return GF_OK;
}

// Optimizer.cc:1517-1675 on host arrays, synchronous
int gf_lba_graph(gf_ctx* ctx, const gf_lba_tables* tables, int nlocal, const int32_t* local,
                 const gf_lba_graph_out* out) {
    GF_CHECK(ctx && tables && out, GF_ERR_ARG, "gf_lba_graph: null arg");
    const gf_lba_tables& T = *tables;
    const gf_lba_graph_out& O = *out;
    LgLocal L;
    int rc = check_local(tables, nlocal, local, &L);
    if (rc) return rc;
    GF_CHECK(T.kf_off && T.kf_bad && T.kf_Tcw && T.inv_sigma2, GF_ERR_ARG, "gf_lba_graph: null keyframe table");
    GF_CHECK(T.nkp == 0 || (T.octave && T.slots && T.kp_xy), GF_ERR_ARG, "gf_lba_graph: null keypoint table");
    GF_CHECK(T.nmp == 0 || (T.mp_bad && T.mp_pos && T.obs_off), GF_ERR_ARG, "gf_lba_graph: null point table");
    GF_CHECK(T.nobs == 0 || T.obs_gkp, GF_ERR_ARG, "gf_lba_graph: null observation table");
    GF_CHECK(O.counts && O.prob_kf && O.kf_kind && O.kf_Tcw && O.kf_cam, GF_ERR_ARG, "gf_lba_graph: null output");
    GF_CHECK(T.nmp == 0 || (O.prob_pt && O.pt_pos), GF_ERR_ARG, "gf_lba_graph: null point output");
    GF_CHECK(T.nobs == 0 || (O.edge_pt && O.edge_kf && O.edge_z && O.edge_inv_sigma2 && O.edge_gkp), GF_ERR_ARG,
             "gf_lba_graph: null edge output");
    GF_CHECK(T.kf_off[0] == 0, GF_ERR_ARG, "gf_lba_graph: kf_off[0] must be 0");
    for (int k = 0; k < T.nkf; k++) {
        GF_CHECK(T.kf_off[k + 1] >= T.kf_off[k], GF_ERR_ARG, "gf_lba_graph: kf_off must be non-decreasing");
        GF_CHECK(T.kf_off[k + 1] - T.kf_off[k] <= LG_MAX_KP, GF_ERR_ARG, "gf_lba_graph: at most 4096 keypoints per keyframe");
    }
    GF_CHECK(T.kf_off[T.nkf] == T.nkp, GF_ERR_ARG, "gf_lba_graph: kf_off must end at nkp");
    for (int i = 0; i < T.nkp; i++) GF_CHECK(T.octave[i] < T.nlevels, GF_ERR_ARG, "gf_lba_graph: octave >= nlevels");
    if (T.nmp) {
        GF_CHECK(T.obs_off[0] == 0, GF_ERR_ARG, "gf_lba_graph: obs_off[0] must be 0");
        for (int p = 0; p < T.nmp; p++)
            GF_CHECK(T.obs_off[p + 1] >= T.obs_off[p], GF_ERR_ARG, "gf_lba_graph: obs_off must be non-decreasing");
        GF_CHECK(T.obs_off[T.nmp] == T.nobs, GF_ERR_ARG, "gf_lba_graph: obs_off must end at nobs");
    } else {
        GF_CHECK(T.nobs == 0, GF_ERR_ARG, "gf_lba_graph: observations without points");
    }
    for (int o = 0; o < T.nobs; o++)
        GF_CHECK(T.obs_gkp[o] >= -1 && T.obs_gkp[o] < T.nkp, GF_ERR_ARG, "gf_lba_graph: observation entry out of range");
    GF_HIP(hipSetDevice(ctx->device));
    // one scratch block: the twelve tables, then the twelve outputs
    const size_t NK = (size_t)T.nkf, NP = (size_t)T.nkp, NM = (size_t)T.nmp, NO = (size_t)T.nobs;
    const void* in[11] = {T.kf_off, T.octave, T.slots, T.kf_bad, T.kp_xy, T.kf_Tcw, T.mp_bad, T.mp_pos,
                          NM ? T.obs_off : nullptr, T.obs_gkp, T.inv_sigma2};
    const size_t in_b[11] = {4 * (NK + 1), NP, 4 * NP, NK, 8 * NP, 64 * NK, NM, 12 * NM, NM ? 4 * (NM + 1) : 0, 4 * NO,
                             4 * (size_t)T.nlevels};
    void* outp[12] = {O.counts, O.prob_kf, O.kf_kind, O.kf_Tcw, O.kf_cam, O.prob_pt, O.pt_pos, O.edge_pt, O.edge_kf,
                      O.edge_z, O.edge_inv_sigma2, O.edge_gkp};
    // bytes per problem keyframe / point / edge of every output (counts: 12 bytes flat)
    const size_t out_unit[12] = {0, 4, 1, 64, 16, 4, 12, 4, 4, 8, 4, 4};
    const int out_of[12] = {-1, 0, 0, 0, 0, 1, 1, 2, 2, 2, 2, 2};
    const size_t bound[3] = {NK, NM, NO};
    size_t off = 0, in_o[11], out_o[12];
    for (int i = 0; i < 11; i++) in_o[i] = off, off += up16(in_b[i]);
    for (int i = 0; i < 12; i++) out_o[i] = off, off += up16(i ? out_unit[i] * bound[out_of[i]] : 12);
    void* dbuf;
    rc = gf::ws_get(ctx, 71, off, &dbuf);
    if (rc) return rc;
    uint8_t* base = (uint8_t*)dbuf;
    hipStream_t s = ctx->stream;
    for (int i = 0; i < 11; i++)
        if (in_b[i] && in[i]) GF_HIP(hipMemcpyAsync(base + in_o[i], in[i], in_b[i], hipMemcpyHostToDevice, s));
    gf_lba_tables D = T;
    D.kf_off = (const int32_t*)(base + in_o[0]), D.octave = base + in_o[1], D.slots = (const int32_t*)(base + in_o[2]);
    D.kf_bad = base + in_o[3], D.kp_xy = (const float*)(base + in_o[4]), D.kf_Tcw = (const float*)(base + in_o[5]);
    D.mp_bad = base + in_o[6], D.mp_pos = (const float*)(base + in_o[7]), D.obs_off = (const int32_t*)(base + in_o[8]);
    D.obs_gkp = (const int32_t*)(base + in_o[9]), D.inv_sigma2 = (const float*)(base + in_o[10]);
    gf_lba_graph_out DO;
    DO.counts = (int32_t*)(base + out_o[0]), DO.prob_kf = (int32_t*)(base + out_o[1]), DO.kf_kind = base + out_o[2];
    DO.kf_Tcw = (float*)(base + out_o[3]), DO.kf_cam = (float*)(base + out_o[4]);
    DO.prob_pt = (int32_t*)(base + out_o[5]), DO.pt_pos = (float*)(base + out_o[6]);
    DO.edge_pt = (int32_t*)(base + out_o[7]), DO.edge_kf = (int32_t*)(base + out_o[8]);
    DO.edge_z = (float*)(base + out_o[9]), DO.edge_inv_sigma2 = (float*)(base + out_o[10]);
    DO.edge_gkp = (int32_t*)(base + out_o[11]);
    rc = gf_lba_graph_dev(ctx, &D, nlocal, local, &DO, s);
    if (rc) return rc;
    int32_t n[3];
    GF_HIP(hipMemcpyAsync(n, base + out_o[0], 12, hipMemcpyDeviceToHost, s));
    GF_HIP(hipStreamSynchronize(s));
    for (int c = 0; c < 3; c++)
        GF_CHECK(n[c] >= 0 && (size_t)n[c] <= bound[c], GF_ERR_HIP, "gf_lba_graph: a count left its bound");
    for (int i = 1; i < 12; i++) {
        const size_t b = out_unit[i] * (size_t)n[out_of[i]];
        if (b) GF_HIP(hipMemcpyAsync(outp[i], base + out_o[i], b, hipMemcpyDeviceToHost, s));
    }
    GF_HIP(hipStreamSynchronize(s));
    O.counts[0] = n[0], O.counts[1] = n[1], O.counts[2] = n[2];
    return GF_OK;
}

}  // extern "C"
