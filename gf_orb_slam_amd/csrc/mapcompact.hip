// Map compaction: the requests of gf_frontend_compact_maps applied in place to
// the front end's stream maps and keyframe graphs (Map::EraseMapPoint /
// Map::EraseKeyFrame, Map.cc, as the tracker would see them through MapPoint* /
// KeyFrame*). grid.y is the listed stream; every kernel reads its stream's
// McHdr from the staging buffer:
//   k_mc_mark      keep flags: 1 everywhere, 0 for the listed drops, then 1
//                  again for what frame state still holds (the pins)
//   k_mc_scan      the flags scanned into the remap tables (new index, -1
//                  dropped), the new counts, the listed items that were pinned
//   k_mc_move      one workgroup per section: each per-point array, the slot
//                  rows, the keyframe rows with the covisibility lists, the
//                  index holders, and the scan of the new observation offsets
//   k_mc_obs_rows  the filtered observation rows into the staging table
//   k_mc_finish    staging table and offsets home, the counts the step reads
// Rows move down in place (new index <= old index), so a destination can be a
// source that another lane has not read yet: a section is walked by one
// workgroup in ascending chunks, all loads of a chunk before the barrier that
// precedes its stores. A chunk's stores land below the next chunk's sources.
// The packed mp_obs CSR changes row lengths, hence scan / rows / home as in
// mapupdate.hip. No kernel waits on another workgroup and there are no
// atomics: every destination has one writer, except the pin marks, where every
// writer stores the same 1.
#include "mapcompact.h"

namespace {

using gf::MapCompactArgs;
using gf::McHdr;

constexpr int MC_U = 4;                  // loads in flight per thread
constexpr int MC_CHUNK = 256 * MC_U;     // elements per chunk of a section
constexpr int KC = 64;                   // keyframes per stream graph (one wave)
constexpr int SCAN_PTS = 4;              // points per thread and round of a scan
constexpr int OBS_PTS = 256;             // points per workgroup of k_mc_obs_rows
constexpr int MC_FIRST = gf::MC_RES_N - 1;  // res word: the first point that moves

// sections of k_mc_move along blockIdx.x
enum {
    SEC_MAP = 0, SEC_DESC, SEC_POS, SEC_VIEWS, SEC_H, SEC_INFO, SEC_INFO_LT, SEC_UV, SEC_UPD, SEC_UPDATED, SEC_MP_BAD,
    SEC_SLOTS, SEC_KF, SEC_INDEX, SEC_OBS_SCAN, SEC_N
};

__device__ __forceinline__ const McHdr* hdr_of(const MapCompactArgs& A, int l) {
    return reinterpret_cast<const McHdr*>(A.stage) + l;
}
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// Sum over the workgroup (256 threads); every thread gets it.
__device__ __forceinline__ int block_sum(int v, int* s_wave) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = v;
    __syncthreads();
    return s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
}
__device__ __forceinline__ int block_min(int v, int* s_wave) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = v;
    __syncthreads();
    return min(min(s_wave[0], s_wave[1]), min(s_wave[2], s_wave[3]));
}

// keep[v] = 1 for every map index the n entries of `held` name
__device__ __forceinline__ void pin_points(const int32_t* held, int n, int32_t* keep, int nmp) {
    for (int i0 = threadIdx.x; i0 < n; i0 += MC_CHUNK) {
        int v[MC_U];
#pragma unroll
        for (int u = 0; u < MC_U; u++) v[u] = held[min(i0 + 256 * u, n - 1)];
#pragma unroll
        for (int u = 0; u < MC_U; u++)
            if (i0 + 256 * u < n && v[u] >= 0 && v[u] < nmp) keep[v[u]] = 1;
    }
}

__device__ __forceinline__ bool kf_pending(const MapCompactArgs& A, int b) {
    return A.kf_state && A.kf_state[(size_t)b * GF_KF_N + GF_KF_PENDING] != 0;
}

__global__ __launch_bounds__(256) void k_mc_mark(MapCompactArgs A) {
    const int l = blockIdx.x, t = threadIdx.x;
    const McHdr* H = hdr_of(A, l);
    const int b = H->stream, n = H->nmp0, nk = H->nkf0;
    int32_t* km = A.mp_remap + (long long)l * A.M;
    int32_t* kk = A.kf_remap + (long long)l * A.kf_cap;
    for (int i = t; i < n; i += 256) km[i] = 1;
    if (t < nk) kk[t] = 1;
    __syncthreads();
    const int32_t* dm = A.stage + H->drop_mp;
    const int32_t* dk = A.stage + H->drop_kf;
    for (int i = t; i < H->n_drop_mp; i += 256) km[dm[i]] = 0;
    for (int i = t; i < H->n_drop_kf; i += 256) kk[dk[i]] = 0;
    __syncthreads();
    // what the next step can still read through frame state stays
    const long long ko = (long long)b * A.cap;
    pin_points(A.kp2mp + ko, clampi(A.nkp[b], 0, A.cap), km, n);
    pin_points(A.last_kp2mp + ko, clampi(A.last_nkp[b], 0, A.cap), km, n);
    if (kf_pending(A, b)) pin_points(A.out_slots + ko, clampi(A.out_hdr[b].n, 0, A.cap), km, n);
    if (t == 0) {
        const int r = A.ref_kf[b];
        if (r >= 0 && r < nk) kk[r] = 1;
        // mpLastKeyFrame of a pending ForceRelocalisation: the next step's candidate list starts from it
        const int32_t* T = A.track + (size_t)b * GF_TR_N;
        const int f = T[GF_TR_FORCE_KF];
        if (T[GF_TR_FORCE] && f >= 0 && f < nk) kk[f] = 1;
    }
}

__global__ __launch_bounds__(256) void k_mc_scan(MapCompactArgs A) {
    __shared__ int s_wave[4];
    const int l = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const McHdr* H = hdr_of(A, l);
    const int n = H->nmp0, nk = H->nkf0;
    int32_t* km = A.mp_remap + (long long)l * A.M;
    int32_t* kk = A.kf_remap + (long long)l * A.kf_cap;
    int32_t* R = A.res + (long long)l * gf::MC_RES_N;
    int carry = 0, first = n;
    for (int base = 0; base < n; base += 256 * SCAN_PTS) {
        const int p0 = base + SCAN_PTS * t;
        int f[SCAN_PTS];
#pragma unroll
        for (int k = 0; k < SCAN_PTS; k++) f[k] = p0 + k < n ? km[p0 + k] : 0;
        int sum = 0;
#pragma unroll
        for (int k = 0; k < SCAN_PTS; k++) sum += f[k];
        int v = sum;  // inclusive scan over the wave, then over the four waves through LDS
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int u = __shfl_up(v, o, 64);
            if (lane >= o) v += u;
        }
        if (lane == 63) s_wave[wave] = v;
        __syncthreads();
        int wbase = 0, total = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            if (i < wave) wbase += s_wave[i];
            total += s_wave[i];
        }
        int run = carry + wbase + v - sum;
#pragma unroll
        for (int k = 0; k < SCAN_PTS; k++) {
            if (p0 + k < n) {
                km[p0 + k] = f[k] ? run : -1;
                if (!f[k] || run != p0 + k) first = min(first, p0 + k);
            }
            run += f[k];
        }
        carry += total;
        __syncthreads();
    }
    first = block_min(first, s_wave);
    // the keyframes: one wave
    int nkf1 = 0;
    if (wave == 0) {
        const int f = lane < nk ? kk[lane] : 0;
        int v = f;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int u = __shfl_up(v, o, 64);
            if (lane >= o) v += u;
        }
        nkf1 = __shfl(v, 63, 64);
        if (lane < nk) kk[lane] = f ? v - 1 : -1;
    }
    __syncthreads();
    // listed items that stayed
    const int32_t* dm = A.stage + H->drop_mp;
    const int32_t* dk = A.stage + H->drop_kf;
    int cm = 0, ck = 0;
    for (int i = t; i < H->n_drop_mp; i += 256) cm += km[dm[i]] >= 0;
    for (int i = t; i < H->n_drop_kf; i += 256) ck += kk[dk[i]] >= 0;
    cm = block_sum(cm, s_wave);
    ck = block_sum(ck, s_wave);
    if (t == 0) {
        R[gf::MC_NKF] = nkf1;
        R[gf::MC_NMP] = carry;
        R[gf::MC_KEPT_KF] = ck;
        R[gf::MC_KEPT_MP] = cm;
        R[MC_FIRST] = first;
    }
}

// Rows of W elements of T, row r to row remap[r] (< 0: the row goes), in
// ascending chunks from row `first` (the rows below it stay where they are).
template <typename T, int W>
__device__ __forceinline__ void move_rows(T* base, const int32_t* __restrict__ remap, int first, int n) {
    constexpr int ROWS = MC_CHUNK / W;
    static_assert(ROWS >= 1, "a row fits a chunk");
    const int t = threadIdx.x;
    for (int r0 = first; r0 < n; r0 += ROWS) {
        const int ne = min(ROWS, n - r0) * W;
        T v[MC_U];
        long long d[MC_U];
#pragma unroll
        for (int u = 0; u < MC_U; u++) {
            const int e = t + 256 * u, ec = min(e, ne - 1), rr = ec / W, c = ec - rr * W, row = r0 + rr;
            v[u] = base[(long long)row * W + c];
            const int nr = remap[row];
            d[u] = e < ne && nr >= 0 && nr != row ? (long long)nr * W + c : -1;
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < MC_U; u++)
            if (d[u] >= 0) base[d[u]] = v[u];
    }
}

// map index v through the table (an index outside the old map stays as it is)
__device__ __forceinline__ int renum(int v, const int32_t* __restrict__ remap, int n) {
    return v >= 0 && v < n ? remap[v] : v;
}
__device__ __forceinline__ void renumber(int32_t* a, int n, const int32_t* __restrict__ remap, int nmp) {
    for (int i0 = threadIdx.x; i0 < n; i0 += MC_CHUNK) {
        int v[MC_U];
#pragma unroll
        for (int u = 0; u < MC_U; u++) v[u] = a[min(i0 + 256 * u, n - 1)];
#pragma unroll
        for (int u = 0; u < MC_U; u++) v[u] = renum(v[u], remap, nmp);
#pragma unroll
        for (int u = 0; u < MC_U; u++)
            if (i0 + 256 * u < n) a[i0 + 256 * u] = v[u];
    }
}

// KeyFrame::mvpMapPoints: rows of dropped keyframes go, kept rows close up,
// values renumbered (a slot that named a dropped point: -1).
__device__ void move_slots(const MapCompactArgs& A, const McHdr* H, const int32_t* km, const int32_t* kk,
                           int32_t* R) {
    __shared__ int s_old[KC + 1], s_new[KC + 1], s_kr[KC];
    const int t = threadIdx.x, b = H->stream, nk = H->nkf0, n = H->nmp0;
    int32_t* off = A.kf_mp_off + (long long)b * (A.kf_cap + 1);
    int32_t* slots = A.kf_mp + (long long)b * A.slot_cap;
    if (t <= nk) s_old[t] = nk ? clampi(off[t], 0, (int)A.slot_cap) : 0;
    if (t < nk) s_kr[t] = kk[t];
    __syncthreads();
    if (t == 0) {
        int run = 0, k1 = 0;
        for (int k = 0; k < nk; k++)
            if (s_kr[k] >= 0) {
                s_new[k1++] = run;
                run += max(s_old[k + 1] - s_old[k], 0);
            }
        s_new[k1] = run;
        R[gf::MC_NS] = run;
    }
    __syncthreads();
    const int ns0 = s_old[nk], nk1 = R[gf::MC_NKF];
    for (int i0 = 0; i0 < ns0; i0 += MC_CHUNK) {
        int v[MC_U], d[MC_U];
#pragma unroll
        for (int u = 0; u < MC_U; u++) {
            const int i = min(i0 + t + 256 * u, ns0 - 1);
            v[u] = slots[i];
            int lo = 0, hi = nk;  // the last k with s_old[k] <= i: its row holds i (empty rows share an offset)
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (s_old[mid] <= i) lo = mid; else hi = mid;
            }
            const int kn = s_kr[lo];
            d[u] = i0 + t + 256 * u < ns0 && kn >= 0 ? s_new[kn] + (i - s_old[lo]) : -1;
        }
#pragma unroll
        for (int u = 0; u < MC_U; u++) v[u] = v[u] >= 0 && v[u] < n ? km[v[u]] : -1;
        __syncthreads();
#pragma unroll
        for (int u = 0; u < MC_U; u++)
            if (d[u] >= 0) slots[d[u]] = v[u];
    }
    if (t <= nk1) off[t] = s_new[t];
}

// kf_bad and GF_FE_RELOC rows with their keyframe; mvpOrderedConnectedKeyFrames
// filtered in order and renumbered.
__device__ void move_keyframes(const MapCompactArgs& A, const McHdr* H, const int32_t* kk, int32_t* R) {
    __shared__ int s_cov[KC * KC];
    __shared__ int s_off[KC + 1], s_noff[KC + 1], s_kr[KC], s_len[KC];
    const int t = threadIdx.x, b = H->stream, nk = H->nkf0;
    int32_t* off = A.kf_cov_off + (long long)b * (A.kf_cap + 1);
    int32_t* cov = A.kf_cov + (long long)b * A.kf_cap * A.kf_cap;
    uint8_t* bad = A.kf_bad + (long long)b * A.kf_cap;
    gf_reloc_kf* rl = A.reloc + (long long)b * A.kf_cap;
    if (t <= nk) s_off[t] = nk ? clampi(off[t], 0, KC * KC) : 0;
    if (t < nk) s_kr[t] = kk[t];
    __syncthreads();
    const int nc0 = s_off[nk];
    for (int i = t; i < nc0; i += 256) s_cov[i] = clampi(cov[i], 0, max(nk - 1, 0));
    uint8_t vb = 0;
    gf_reloc_kf vr{};
    if (t < nk) {
        vb = bad[t];
        vr = rl[t];
    }
    __syncthreads();
    if (t < nk) {
        const int kn = s_kr[t];
        if (kn >= 0 && kn != t) {
            bad[kn] = vb;
            rl[kn] = vr;
        }
        int len = 0;
        if (kn >= 0)
            for (int e = s_off[t]; e < s_off[t + 1]; e++) len += s_kr[s_cov[e]] >= 0;
        s_len[t] = len;
    }
    __syncthreads();
    if (t == 0) {
        int run = 0, k1 = 0;
        for (int k = 0; k < nk; k++)
            if (s_kr[k] >= 0) {
                s_noff[k1++] = run;
                run += s_len[k];
            }
        s_noff[k1] = run;
        R[gf::MC_NC] = run;
    }
    __syncthreads();
    if (t < nk && s_kr[t] >= 0) {
        int j = s_noff[s_kr[t]];
        for (int e = s_off[t]; e < s_off[t + 1]; e++) {
            const int kn = s_kr[s_cov[e]];
            if (kn >= 0) cov[j++] = kn;
        }
    }
    if (t <= R[gf::MC_NKF]) off[t] = s_noff[t];
}

// The index holders outside the map: pinned ones through the table, the last
// step's outputs with a dropped entry turned into -1.
__device__ void renumber_holders(const MapCompactArgs& A, const McHdr* H, const int32_t* km, const int32_t* kk) {
    const int b = H->stream, n = H->nmp0, nk = H->nkf0;
    const long long ko = (long long)b * A.cap;
    renumber(A.kp2mp + ko, clampi(A.nkp[b], 0, A.cap), km, n);
    renumber(A.last_kp2mp + ko, clampi(A.last_nkp[b], 0, A.cap), km, n);
    renumber(A.left + (long long)b * A.M, clampi(A.nleft[b], 0, A.M), km, n);
    if (kf_pending(A, b)) renumber(A.out_slots + ko, clampi(A.out_hdr[b].n, 0, A.cap), km, n);
    if (threadIdx.x == 0) {
        A.ref_kf[b] = renum(A.ref_kf[b], kk, nk);
        int32_t* T = A.track + (size_t)b * GF_TR_N;
        if (T[GF_TR_FORCE]) T[GF_TR_FORCE_KF] = renum(T[GF_TR_FORCE_KF], kk, nk);  // pinned: never -1
        if (A.kf_state) {
            int32_t* S = A.kf_state + (size_t)b * GF_KF_N;
            S[GF_KF_REF] = renum(S[GF_KF_REF], kk, nk);
        }
    }
}

// New observation row lengths (kept keyframes of a kept point's row) scanned
// into the new offsets, at the points' new indices.
__device__ void scan_observations(const MapCompactArgs& A, const McHdr* H, int l, const int32_t* km, const int32_t* kk,
                                  int32_t* R) {
    __shared__ int s_wave[4];
    __shared__ int s_kr[KC];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int b = H->stream, n = H->nmp0, nk = H->nkf0;
    const int32_t* ooff = A.mp_obs_off + (long long)b * (A.M + 1);
    const int32_t* obs = A.mp_obs + (long long)b * A.slot_cap;
    int32_t* out = A.obs_off_new + (long long)l * (A.M + 1);
    if (t < KC) s_kr[t] = t < nk ? kk[t] : -1;
    __syncthreads();
    int carry = 0;
    for (int base = 0; base < n; base += 256 * SCAN_PTS) {
        const int p0 = base + SCAN_PTS * t;
        int len[SCAN_PTS], to[SCAN_PTS];
#pragma unroll
        for (int k = 0; k < SCAN_PTS; k++) {
            const int p = p0 + k;
            len[k] = 0;
            to[k] = p < n ? km[p] : -1;
            if (to[k] < 0) continue;
            const int e0 = clampi(ooff[p], 0, (int)A.slot_cap), e1 = clampi(ooff[p + 1], e0, (int)A.slot_cap);
            for (int e = e0; e < e1; e++) len[k] += s_kr[clampi(obs[e], 0, KC - 1)] >= 0;
        }
        int sum = 0;
#pragma unroll
        for (int k = 0; k < SCAN_PTS; k++) sum += len[k];
        int v = sum;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int u = __shfl_up(v, o, 64);
            if (lane >= o) v += u;
        }
        if (lane == 63) s_wave[wave] = v;
        __syncthreads();
        int wbase = 0, total = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            if (i < wave) wbase += s_wave[i];
            total += s_wave[i];
        }
        int run = carry + wbase + v - sum;
#pragma unroll
        for (int k = 0; k < SCAN_PTS; k++) {
            if (to[k] >= 0) out[to[k]] = run;
            run += len[k];
        }
        carry += total;
        __syncthreads();
    }
    if (t == 0) {
        out[R[gf::MC_NMP]] = carry;
        R[gf::MC_NO] = carry;
    }
}

__global__ __launch_bounds__(256) void k_mc_move(MapCompactArgs A) {
    const int l = blockIdx.y;
    const McHdr* H = hdr_of(A, l);
    const long long om = (long long)H->stream * A.M;
    const int32_t* km = A.mp_remap + (long long)l * A.M;
    const int32_t* kk = A.kf_remap + (long long)l * A.kf_cap;
    int32_t* R = A.res + (long long)l * gf::MC_RES_N;
    const int n = H->nmp0, first = clampi(R[MC_FIRST], 0, n);
    switch (blockIdx.x) {  // uniform
    case SEC_MAP: move_rows<uint4, 2>(reinterpret_cast<uint4*>(A.map + om), km, first, n); break;
    case SEC_DESC: move_rows<uint4, 2>(reinterpret_cast<uint4*>(A.desc + om * 32), km, first, n); break;
    case SEC_POS: move_rows<float, 3>(A.pos + om * 3, km, first, n); break;
    case SEC_VIEWS:
        move_rows<uint32_t, sizeof(gf_mp_view) / 4>(reinterpret_cast<uint32_t*>(A.views + om), km, first, n);
        break;
    case SEC_H: move_rows<uint4, 7>(reinterpret_cast<uint4*>(A.H + om * 14), km, first, n); break;
    case SEC_INFO: move_rows<double, 49>(A.info + om * 49, km, first, n); break;  // 392-byte rows: 8-byte aligned only
    case SEC_INFO_LT: move_rows<uint4, 16>(reinterpret_cast<uint4*>(A.info_lt + om * 32), km, first, n); break;
    case SEC_UV: move_rows<float2, 1>(reinterpret_cast<float2*>(A.uv + om * 2), km, first, n); break;
    case SEC_UPD: move_rows<int32_t, 1>(A.upd + om, km, first, n); break;
    case SEC_UPDATED: move_rows<uint8_t, 1>(A.updated + om, km, first, n); break;
    case SEC_MP_BAD: move_rows<uint8_t, 1>(A.mp_bad + om, km, first, n); break;
    case SEC_SLOTS: move_slots(A, H, km, kk, R); break;
    case SEC_KF: move_keyframes(A, H, kk, R); break;
    case SEC_INDEX: renumber_holders(A, H, km, kk); break;
    default: scan_observations(A, H, l, km, kk, R); break;
    }
}

// One thread per old point: its row's kept keyframes, renumbered, at the new offset.
__global__ __launch_bounds__(256) void k_mc_obs_rows(MapCompactArgs A) {
    __shared__ int s_kr[KC];
    const int l = blockIdx.y, t = threadIdx.x;
    const McHdr* H = hdr_of(A, l);
    const int n = H->nmp0, nk = H->nkf0, p0 = blockIdx.x * OBS_PTS;
    if (p0 >= n) return;  // uniform
    const int32_t* kk = A.kf_remap + (long long)l * A.kf_cap;
    if (t < KC) s_kr[t] = t < nk ? kk[t] : -1;
    __syncthreads();
    const int p = p0 + t;
    if (p >= n) return;
    const int to = A.mp_remap[(long long)l * A.M + p];
    if (to < 0) return;
    const long long b = H->stream;
    const int32_t* ooff = A.mp_obs_off + b * (A.M + 1);
    const int32_t* obs = A.mp_obs + b * A.slot_cap;
    const int e0 = clampi(ooff[p], 0, (int)A.slot_cap), e1 = clampi(ooff[p + 1], e0, (int)A.slot_cap);
    int j = A.obs_off_new[(long long)l * (A.M + 1) + to];
    int32_t* dst = A.obs_new + (long long)l * A.slot_cap;
    for (int e = e0; e < e1; e++) {
        const int kn = s_kr[clampi(obs[e], 0, KC - 1)];
        if (kn >= 0) dst[j++] = kn;  // j stays below the old total: the rows only shrink
    }
}

__global__ __launch_bounds__(256) void k_mc_finish(MapCompactArgs A) {
    const int l = blockIdx.y, t = threadIdx.x;
    const McHdr* H = hdr_of(A, l);
    const long long b = H->stream;
    const int32_t* R = A.res + (long long)l * gf::MC_RES_N;
    const int no = clampi(R[gf::MC_NO], 0, (int)A.slot_cap), nmp1 = R[gf::MC_NMP];
    const int32_t* src = A.obs_new + (long long)l * A.slot_cap;
    int32_t* dst = A.mp_obs + b * A.slot_cap;
    const int32_t* so = A.obs_off_new + (long long)l * (A.M + 1);
    int32_t* dof = A.mp_obs_off + b * (A.M + 1);
    for (int k0 = blockIdx.x * MC_CHUNK; k0 < max(no, nmp1 + 1); k0 += gridDim.x * MC_CHUNK) {
        int v[MC_U], w[MC_U];
#pragma unroll
        for (int u = 0; u < MC_U; u++) {
            const int i = k0 + t + 256 * u;
            v[u] = src[min(i, max(no - 1, 0))];
            w[u] = so[min(i, nmp1)];
        }
#pragma unroll
        for (int u = 0; u < MC_U; u++) {
            const int i = k0 + t + 256 * u;
            if (i < no) dst[i] = v[u];
            if (i <= nmp1) dof[i] = w[u];
        }
    }
    if (blockIdx.x == 0 && t == 0) {
        A.nmp[b] = nmp1;
        A.kfc[b] = R[gf::MC_NKF];
        A.covis[b].nkf = R[gf::MC_NKF];
        A.covis[b].nmp = nmp1;
    }
}

inline int cdiv(int a, int b) { return (a + b - 1) / b; }

}  // namespace

namespace gf {

int map_compact_launch(gf_ctx* ctx, const MapCompactArgs& a, hipStream_t s) {
    GF_CHECK(a.kf_cap == KC, GF_ERR_UNSUPPORTED, "map compaction is built for 64 keyframes per stream graph");
    GF_CHECK(a.L > 0, GF_ERR_ARG, "no stream listed");
    {
        GF_PROF(ctx, s, "k_mc_mark");
        GF_LAUNCH(k_mc_mark, a.L, 256, 0, s, a);
        GF_HIP(hipGetLastError());
    }
    {
        GF_PROF(ctx, s, "k_mc_scan");
        GF_LAUNCH(k_mc_scan, a.L, 256, 0, s, a);
        GF_HIP(hipGetLastError());
    }
    {
        GF_PROF(ctx, s, "k_mc_move");
        GF_LAUNCH(k_mc_move, dim3(SEC_N, a.L), 256, 0, s, a);
        GF_HIP(hipGetLastError());
    }
    {
        GF_PROF(ctx, s, "k_mc_obs_rows");
        GF_LAUNCH(k_mc_obs_rows, dim3(cdiv(a.M, OBS_PTS), a.L), 256, 0, s, a);
        GF_HIP(hipGetLastError());
    }
    GF_PROF(ctx, s, "k_mc_finish");
    GF_LAUNCH(k_mc_finish, dim3(std::max(1, std::min(16, cdiv((int)a.slot_cap, 8 * MC_CHUNK))), a.L), 256, 0, s, a);
    GF_HIP(hipGetLastError());
    return GF_OK;
}

}  // namespace gf
