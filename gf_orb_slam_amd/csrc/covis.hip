// The counting and ordering of KeyFrame::UpdateConnections (src/KeyFrame.cc:
// 332-403) for any number of query keyframes in one launch, over the flat map
// tables of kfcull.hip:
//
//   k_update_connections: one workgroup per query, the query's slots spread
//     over the lanes, two per lane and step. A slot's point gives its
//     observation row, a row's entries are loaded eight at a time and their
//     keyframes found together by a branch-free binary search in kf_off, so
//     the chain slot -> row -> entry -> keyframe waits once per stage and not
//     once per observation. The keyframe counter
//     (KFcounter) is a histogram in LDS of UC_TILE keyframes; a map with more
//     keyframes is counted tile by tile, the slots walked once per tile (the
//     tables stay in cache), so no add ever leaves the workgroup and every
//     number is an integer sum whatever the arrival order. With nkf <= UC_TILE
//     kf_off is staged in LDS and the search runs there.
//   The ordering (:369-403) is a rank by count: a listed keyframe's place is
//     the number of listed (weight, index) pairs above it. Up to UC_LIST listed
//     keyframes are ranked from a list in LDS, more than that from the weight
//     row the workgroup wrote, staged through LDS a tile at a time.
//
// The graph updates of :376-418 (AddConnection on the others, the keyframe's
// own containers, the first-connection parent) are map surgery and stay with
// the caller (gf_orb_slam_amd/loopmap.py: apply_connections).
#include <vector>

#include "common.h"

#define UC_THREADS 256
#define UC_BATCH 8
#define UC_MAX_KP 4096
#define UC_TILE 1024  // keyframes per LDS histogram
#define UC_LIST 256   // listed keyframes ranked from LDS
#define UC_TH 15      // th of :369

namespace {

// the keyframe of global keypoint index g in [0, nkp): the last k in [0, nkf) with off[k] <= g (off[0] = 0), by
// steps top, top / 2, ..., 1 with top the largest power of two below nkf; no branch, one load per entry and step
template <bool SMALL>
__device__ __forceinline__ void uc_find_kf(const int32_t* __restrict__ kf_off, const int* s_off, int nkf, int top,
                                           const int (&g)[UC_BATCH], int (&kf)[UC_BATCH]) {
#pragma unroll
    for (int j = 0; j < UC_BATCH; j++) kf[j] = 0;
    for (int step = top; step > 0; step >>= 1) {
        int v[UC_BATCH];
#pragma unroll
        for (int j = 0; j < UC_BATCH; j++) {
            const int m = min(kf[j] + step, nkf);  // off has nkf + 1 entries
            v[j] = SMALL ? s_off[m] : gfd::ldg(kf_off + m);
        }
#pragma unroll
        for (int j = 0; j < UC_BATCH; j++) kf[j] = kf[j] + step < nkf && v[j] <= g[j] ? kf[j] + step : kf[j];
    }
}

// (weight, index) above (w, k) in the reversed sort of (int, KeyFrame*) pairs (:391-398)
__device__ __forceinline__ int uc_above(int w2, int k2, int w, int k) { return w2 > w || (w2 == w && k2 > k); }

template <bool SMALL>
__global__ __launch_bounds__(UC_THREADS) void k_update_connections(
    int nkf, int nkp, const int32_t* __restrict__ kf_off, const int32_t* __restrict__ slots, int nmp,
    const uint8_t* __restrict__ mp_bad, const int32_t* __restrict__ obs_off, const int32_t* __restrict__ obs_gkp,
    int nobs, const int32_t* __restrict__ query, int32_t* weights, int32_t* __restrict__ n_ordered,
    int32_t* __restrict__ ordered_kf, int32_t* __restrict__ ordered_w) {
    __shared__ int hist[UC_TILE];
    __shared__ int s_off[SMALL ? UC_TILE + 1 : 1];
    __shared__ int list_k[UC_LIST], list_w[UC_LIST];
    __shared__ int s_listed;
    __shared__ unsigned long long s_best;  // (weight << 32) | ~index: the heaviest, the lowest index among equals (:378)
    const int tid = threadIdx.x;
    const int K = gfd::ldg(query + blockIdx.x);
    int32_t* W = weights + (size_t)blockIdx.x * nkf;
    int32_t* OK = ordered_kf + (size_t)blockIdx.x * nkf;
    int32_t* OW = ordered_w + (size_t)blockIdx.x * nkf;
    int s0 = 0, s1 = 0;
    if (K >= 0 && K < nkf) {
        s0 = min(max(gfd::ldg(kf_off + K), 0), nkp);
        s1 = min(max(gfd::ldg(kf_off + K + 1), s0), nkp);
        s1 = min(s1, s0 + UC_MAX_KP);
    }
    if (SMALL)
        for (int k = tid; k <= nkf; k += UC_THREADS) s_off[k] = gfd::ldg(kf_off + k);
    if (tid == 0) s_listed = 0, s_best = 0ull;
    const int top = nkf > 1 ? 1 << (31 - __clz(nkf - 1)) : 0;  // uc_find_kf's first step
    for (int t0 = 0; t0 < nkf; t0 += UC_TILE) {
        const int tn = min(UC_TILE, nkf - t0);
        for (int k = tid; k < tn; k += UC_THREADS) hist[k] = 0;
        __syncthreads();
        // one batch of row entries [r, r1), loaded together
        auto load = [&](int r, int r1, int(&g)[UC_BATCH]) {
#pragma unroll
            for (int j = 0; j < UC_BATCH; j++) g[j] = j < r1 - r ? gfd::ldg(obs_gkp + r + j) : -1;
        };
        // their keyframes, found together, and the adds of this tile
        auto count = [&](int(&g)[UC_BATCH]) {
            int gs[UC_BATCH], kf[UC_BATCH];
#pragma unroll
            for (int j = 0; j < UC_BATCH; j++) {
                if (g[j] >= nkp) g[j] = -1;
                gs[j] = max(g[j], 0);
            }
            uc_find_kf<SMALL>(kf_off, s_off, nkf, top, gs, kf);
#pragma unroll
            for (int j = 0; j < UC_BATCH; j++) {
                const int rel = kf[j] - t0;
                // mit->first->mnId == mnId (:359) leaves the query itself out
                if (g[j] >= 0 && kf[j] != K && rel >= 0 && rel < tn) atomicAdd(&hist[rel], 1);
            }
        };
        // two slots per lane and step: their points, their rows and the rows' first batches each wait once for both
        for (int i = s0 + tid; i < s1; i += 2 * UC_THREADS) {
            int p[2], bad[2] = {1, 1}, r0[2] = {0, 0}, r1[2] = {0, 0};
#pragma unroll
            for (int u = 0; u < 2; u++) p[u] = u * UC_THREADS < s1 - i ? gfd::ldg(slots + i + u * UC_THREADS) : -1;
#pragma unroll
            for (int u = 0; u < 2; u++) {
                const bool has = p[u] >= 0 && p[u] < nmp;  // pMP (:349), or an id past the map
                const int ps = has ? p[u] : 0;
                if (nmp > 0) {
                    bad[u] = gfd::ldg(mp_bad + ps);
                    r0[u] = gfd::ldg(obs_off + ps);
                    r1[u] = gfd::ldg(obs_off + ps + 1);
                }
                if (!has) bad[u] = 1;
            }
#pragma unroll
            for (int u = 0; u < 2; u++) {
                r0[u] = min(max(r0[u], 0), nobs);
                r1[u] = !bad[u] ? min(max(r1[u], r0[u]), nobs) : r0[u];  // isBad() (:352)
            }
            int ga[UC_BATCH], gb[UC_BATCH];
            load(r0[0], r1[0], ga);
            load(r0[1], r1[1], gb);
            count(ga);
            count(gb);
#pragma unroll
            for (int u = 0; u < 2; u++)
                for (int r = r0[u]; r1[u] - r > UC_BATCH;) {
                    r += UC_BATCH;
                    load(r, r1[u], ga);
                    count(ga);
                }
        }
        __syncthreads();
        for (int k = tid; k < tn; k += UC_THREADS) {
            const int w = hist[k];
            W[t0 + k] = w;
            if (w > 0)
                atomicMax(&s_best, ((unsigned long long)(unsigned)w << 32) | (unsigned)(0x7fffffff - (t0 + k)));
            if (w >= UC_TH) {
                const int at = atomicAdd(&s_listed, 1);
                if (at < UC_LIST) list_k[at] = t0 + k, list_w[at] = w;
            }
        }
        __syncthreads();
    }
    __syncthreads();  // nkf == 0: s_listed and s_best
    const int listed = s_listed;
    const unsigned long long best = s_best;
    int n_out = listed;
    if (listed == 0) {  // none reaches th: the single heaviest (:385-389), or an empty counter (:365)
        n_out = best ? 1 : 0;
        if (best && tid == 0) {
            OK[0] = 0x7fffffff - (int)(unsigned)(best & 0xffffffffull);
            OW[0] = (int)(best >> 32);
        }
    } else if (listed <= UC_LIST) {
        for (int j = tid; j < listed; j += UC_THREADS) {
            const int k = list_k[j], w = list_w[j];
            int rank = 0;
            for (int i = 0; i < listed; i++) rank += uc_above(list_w[i], list_k[i], w, k);
            OK[rank] = k;
            OW[rank] = w;
        }
    } else {  // from the weight row this workgroup wrote above (visible to it after the barrier), a tile at a time in LDS
        for (int k0 = 0; k0 < nkf; k0 += UC_THREADS) {
            const int k = k0 + tid;
            const int w = k < nkf ? W[k] : 0;
            int rank = 0;
            for (int t0 = 0; t0 < nkf; t0 += UC_TILE) {
                const int tn = min(UC_TILE, nkf - t0);
                __syncthreads();
                for (int i = tid; i < tn; i += UC_THREADS) hist[i] = W[t0 + i];
                __syncthreads();
                if (w >= UC_TH)
                    for (int i = 0; i < tn; i++) {
                        const int w2 = hist[i];
                        rank += w2 >= UC_TH && uc_above(w2, t0 + i, w, k);
                    }
            }
            if (w >= UC_TH) OK[rank] = k, OW[rank] = w;
        }
    }
    for (int k = n_out + tid; k < nkf; k += UC_THREADS) OK[k] = -1, OW[k] = 0;
    if (tid == 0) n_ordered[blockIdx.x] = n_out;
}

}  // namespace

extern "C" {

// KeyFrame.cc:332-403, the counting and ordering of every query in one launch on device tables
int gf_update_connections_dev(gf_ctx* ctx, int nkf, int nkp, const int32_t* d_kf_off, const int32_t* d_slots, int nmp,
                              const uint8_t* d_mp_bad, const int32_t* d_obs_off, const int32_t* d_obs_gkp, int nobs,
                              int nq, const int32_t* d_query, int32_t* d_weights, int32_t* d_n_ordered,
                              int32_t* d_ordered_kf, int32_t* d_ordered_w, void* stream) {
    GF_CHECK(ctx, GF_ERR_ARG, "gf_update_connections_dev: null arg");
    if (nq <= 0) return GF_OK;
    GF_CHECK(nkf >= 0 && nkp >= 0 && nmp >= 0 && nobs >= 0, GF_ERR_ARG, "gf_update_connections_dev: negative size");
    GF_CHECK(d_kf_off && d_query && d_n_ordered, GF_ERR_ARG, "gf_update_connections_dev: null buffer");
    GF_CHECK(nkf == 0 || (d_weights && d_ordered_kf && d_ordered_w), GF_ERR_ARG,
             "gf_update_connections_dev: null output");
    GF_CHECK(nkp == 0 || d_slots, GF_ERR_ARG, "gf_update_connections_dev: null keyframe table");
    GF_CHECK(nmp == 0 || (d_mp_bad && d_obs_off), GF_ERR_ARG, "gf_update_connections_dev: null point table");
    GF_CHECK(nobs == 0 || d_obs_gkp, GF_ERR_ARG, "gf_update_connections_dev: null observation table");
    hipStream_t s = (hipStream_t)stream;
    GF_PROF(ctx, s, "k_update_connections");
    if (nkf <= UC_TILE)
        GF_LAUNCH(k_update_connections<true>, nq, UC_THREADS, 0, s, nkf, nkp, d_kf_off, d_slots, nmp, d_mp_bad,
                  d_obs_off, d_obs_gkp, nobs, d_query, d_weights, d_n_ordered, d_ordered_kf, d_ordered_w);
    else
        GF_LAUNCH(k_update_connections<false>, nq, UC_THREADS, 0, s, nkf, nkp, d_kf_off, d_slots, nmp, d_mp_bad,
                  d_obs_off, d_obs_gkp, nobs, d_query, d_weights, d_n_ordered, d_ordered_kf, d_ordered_w);
    GF_HIP(hipGetLastError());
    return GF_OK;
}

// KeyFrame.cc:332-403, the counting and ordering on host arrays, synchronous
int gf_update_connections(gf_ctx* ctx, int nkf, const int32_t* kf_off, const int32_t* slots, int nmp,
                          const uint8_t* mp_bad, const int32_t* obs_off, const int32_t* obs_gkp, int nq,
                          const int32_t* query, int32_t* weights, int32_t* n_ordered, int32_t* ordered_kf,
                          int32_t* ordered_w) {
    GF_CHECK(ctx, GF_ERR_ARG, "gf_update_connections: null arg");
    if (nq <= 0) return GF_OK;
    GF_CHECK(nkf >= 0 && nmp >= 0, GF_ERR_ARG, "gf_update_connections: negative size");
    GF_CHECK(kf_off && query && n_ordered, GF_ERR_ARG, "gf_update_connections: null buffer");
    GF_CHECK(nkf == 0 || (weights && ordered_kf && ordered_w), GF_ERR_ARG, "gf_update_connections: null output");
    GF_CHECK(kf_off[0] == 0, GF_ERR_ARG, "kf_off[0] must be 0");
    for (int k = 0; k < nkf; k++) {
        GF_CHECK(kf_off[k + 1] >= kf_off[k], GF_ERR_ARG, "kf_off must be non-decreasing");
        GF_CHECK(kf_off[k + 1] - kf_off[k] <= UC_MAX_KP, GF_ERR_CAP, "at most 4096 keypoints per keyframe");
    }
    const int nkp = kf_off[nkf];
    GF_CHECK(nkp == 0 || slots, GF_ERR_ARG, "gf_update_connections: null keyframe table");
    GF_CHECK(nmp == 0 || (mp_bad && obs_off), GF_ERR_ARG, "gf_update_connections: null point table");
    int nobs = 0;
    if (nmp) {
        GF_CHECK(obs_off[0] == 0, GF_ERR_ARG, "obs_off[0] must be 0");
        for (int p = 0; p < nmp; p++)
            GF_CHECK(obs_off[p + 1] >= obs_off[p], GF_ERR_ARG, "obs_off must be non-decreasing");
        nobs = obs_off[nmp];
    }
    GF_CHECK(nobs == 0 || obs_gkp, GF_ERR_ARG, "gf_update_connections: null observation table");
    GF_HIP(hipSetDevice(ctx->device));
    // one scratch block: [kf_off | slots | mp_bad | obs_off | obs_gkp | query | n_ordered | weights | ordered_kf |
    // ordered_w]
    size_t off = 0;
    std::vector<std::pair<const void*, size_t>> parts;
    auto add = [&](const void* h, size_t bytes) {
        const size_t o = off;
        parts.push_back({h, bytes});
        off += (bytes + 15) & ~(size_t)15;
        return o;
    };
    const size_t NK = (size_t)nkp, NM = (size_t)nmp, NQ = (size_t)nq, row = 4 * NQ * (size_t)nkf;
    const size_t o_ko = add(kf_off, 4 * ((size_t)nkf + 1)), o_sl = add(slots, 4 * NK), o_mb = add(mp_bad, NM),
                 o_oo = add(nmp ? obs_off : nullptr, nmp ? 4 * (NM + 1) : 0), o_og = add(obs_gkp, 4 * (size_t)nobs),
                 o_q = add(query, 4 * NQ), o_n = add(nullptr, 4 * NQ), o_w = add(nullptr, row),
                 o_k = add(nullptr, row), o_v = add(nullptr, row);
    void* dbuf;
    int rc = gf::ws_get(ctx, 72, off, &dbuf);
    if (rc) return rc;
    uint8_t* base = (uint8_t*)dbuf;
    hipStream_t s = ctx->stream;
    size_t cur = 0;
    for (auto& pr : parts) {
        if (pr.second && pr.first) GF_HIP(hipMemcpyAsync(base + cur, pr.first, pr.second, hipMemcpyHostToDevice, s));
        cur += (pr.second + 15) & ~(size_t)15;
    }
    rc = gf_update_connections_dev(ctx, nkf, nkp, (const int32_t*)(base + o_ko), (const int32_t*)(base + o_sl), nmp,
                                   base + o_mb, (const int32_t*)(base + o_oo), (const int32_t*)(base + o_og), nobs, nq,
                                   (const int32_t*)(base + o_q), (int32_t*)(base + o_w), (int32_t*)(base + o_n),
                                   (int32_t*)(base + o_k), (int32_t*)(base + o_v), s);
    if (rc) return rc;
    GF_HIP(hipMemcpyAsync(n_ordered, base + o_n, 4 * NQ, hipMemcpyDeviceToHost, s));
    if (row) {
        GF_HIP(hipMemcpyAsync(weights, base + o_w, row, hipMemcpyDeviceToHost, s));
        GF_HIP(hipMemcpyAsync(ordered_kf, base + o_k, row, hipMemcpyDeviceToHost, s));
        GF_HIP(hipMemcpyAsync(ordered_w, base + o_v, row, hipMemcpyDeviceToHost, s));
    }
    GF_HIP(hipStreamSynchronize(s));
    return GF_OK;
}

}  // extern "C"
