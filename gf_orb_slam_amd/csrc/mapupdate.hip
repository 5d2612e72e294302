// Map feedback: the deltas of gf_frontend_update_maps applied in place to the
// front end's stream maps and keyframe graphs (what Tracking reads through
// MapPoint* / KeyFrame* after LocalMapping wrote it: MapPoint.cc:77-170, Map.cc,
// KeyFrame.cc:126-160, 332-421 as seen from Tracking.cc:3689-3852). Grids are
// (chunk x listed stream); every kernel reads its stream's MuHdr from the
// staging buffer:
//   k_mu_rows      appended points (state of a fresh point), rewritten points,
//                  appended keyframe slot rows at the tail of kf_mp, slot
//                  writes, the covisibility table
//   k_mu_obs_scan  new observation row lengths (the replaced length, else the
//                  old one) scanned into new offsets (one workgroup per stream)
//   k_mu_obs_rows  the rows into the staging table at the new offsets
//   k_mu_finish    staging table and offsets home into the same buffers, the
//                  bad flags, GF_FE_LAST_POS of the last frame's points, the
//                  counts (g_nmp, d_kfc, nkf / nmp of the device gf_covis_map)
// The packed mp_obs CSR cannot be edited in place, hence scan / rows / home;
// no buffer pointer changes, so a captured step graph stays valid. No atomics:
// the host has checked that every destination has one writer, so the results
// do not depend on scheduling.
#include "mapupdate.h"

namespace {

using gf::MapUpdateArgs;
using gf::MuHdr;

constexpr int MU_U = 4;                  // loads in flight per thread, as k_fe_end's END_U
constexpr int PT_ROWS = 128;             // point rows per workgroup: two uint4 per 32-byte row, one per thread
constexpr int WG_WORDS = 256 * MU_U * 4; // words a workgroup copies of a flat section
constexpr int SLOT_WRITES = 256 * MU_U;  // slot writes per workgroup
constexpr int SCAN_PTS = 4;              // points per thread and round of the offset scan
constexpr int OBS_PTS = 256;             // points per workgroup of k_mu_obs_rows

// exclusive ends of the sections' chunk ranges along blockIdx.x
struct RowSeg {
    int e_new, e_set, e_kf, e_slot, e_cov;
};
struct FinSeg {
    int e_home, e_last, e_flags;
};

__device__ __forceinline__ const MuHdr* hdr_of(const MapUpdateArgs& A, int l) {
    return reinterpret_cast<const MuHdr*>(A.stage) + l;
}
template <typename T>
__device__ __forceinline__ const T* sec(const MapUpdateArgs& A, int64_t off) {
    return reinterpret_cast<const T*>(A.stage + off);
}

// n elements from src to dst: each round MU_U loads (clamped, unconditional),
// then their stores, so the loads of a round do not wait on one another.
template <typename T>
__device__ __forceinline__ void copy_words(const T* __restrict__ src, T* __restrict__ dst, int n) {
    for (int i0 = threadIdx.x; i0 < n; i0 += 256 * MU_U) {
        T v[MU_U];
#pragma unroll
        for (int u = 0; u < MU_U; u++) v[u] = src[min(i0 + 256 * u, n - 1)];
#pragma unroll
        for (int u = 0; u < MU_U; u++)
            if (i0 + 256 * u < n) dst[i0 + 256 * u] = v[u];
    }
}

__global__ __launch_bounds__(256) void k_mu_rows(MapUpdateArgs A, RowSeg G) {
    const int l = blockIdx.y, t = threadIdx.x;
    const MuHdr* H = hdr_of(A, l);
    const int b = H->stream;
    const long long om = (long long)b * A.M;
    int x = blockIdx.x;
    if (x < G.e_new) {
        // Map::AddMapPoint: rows nmp0 .. nmp1 - 1, contiguous on both sides
        const int n = H->nmp1 - H->nmp0, k0 = x * PT_ROWS;
        if (k0 >= n) return;
        const int np = min(PT_ROWS, n - k0), nw = 2 * np, w = min(t, nw - 1);
        const long long d0 = om + H->nmp0 + k0;
        const uint4* sm = sec<uint4>(A, H->new_mp) + 2 * (long long)k0;
        const uint4* sd = sec<uint4>(A, H->new_desc) + 2 * (long long)k0;
        const float* sf = reinterpret_cast<const float*>(sm);
        const uint4 vm = sm[w], vd = sd[w];
        float pv[2];
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const int q = min(t + 256 * u, 3 * np - 1), r = q / 3;
            pv[u] = sf[8 * r + (q - 3 * r)];
        }
        const uint8_t bad = sec<uint8_t>(A, H->new_bad)[k0 + min(t, np - 1)];
        if (t < nw) {
            reinterpret_cast<uint4*>(A.map + d0)[t] = vm;
            reinterpret_cast<uint4*>(A.desc + d0 * 32)[t] = vd;
        }
#pragma unroll
        for (int u = 0; u < 2; u++)
            if (t + 256 * u < 3 * np) A.pos[3 * d0 + t + 256 * u] = pv[u];
        if (t < np) {
            A.mp_bad[d0 + t] = bad;
            A.upd[d0 + t] = -1000;  // updateAtFrameId of a point no frame has seen
        }
        uint32_t* vw = reinterpret_cast<uint32_t*>(A.views + d0);
        constexpr int VW = sizeof(gf_mp_view) / 4;
#pragma unroll
        for (int u = 0; u < (VW * PT_ROWS + 255) / 256; u++)
            if (t + 256 * u < VW * np) vw[t + 256 * u] = 0u;
        return;
    }
    x -= G.e_new;
    if (x < G.e_set - G.e_new) {
        // SetWorldPos / UpdateNormalAndDepth / ComputeDistinctiveDescriptors: scattered rows
        const int n = H->n_set, k0 = x * PT_ROWS;
        if (k0 >= n) return;
        const int np = min(PT_ROWS, n - k0), nw = 2 * np, w = min(t, nw - 1), r = w >> 1, h = w & 1;
        const int32_t* si = sec<int32_t>(A, H->set_idx) + k0;
        const uint4* sm = sec<uint4>(A, H->set_mp) + 2 * (long long)k0;
        const uint4* sd = sec<uint4>(A, H->set_desc) + 2 * (long long)k0;
        const float* sf = reinterpret_cast<const float*>(sm);
        const int idx = si[r];
        const uint4 vm = sm[w], vd = sd[w];
        float pv[2];
        int pi[2], pe[2];
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const int q = min(t + 256 * u, 3 * np - 1), rr = q / 3;
            pe[u] = q - 3 * rr;
            pi[u] = si[rr];
            pv[u] = sf[8 * rr + pe[u]];
        }
        if (t < nw) {
            reinterpret_cast<uint4*>(A.map + om + idx)[h] = vm;
            reinterpret_cast<uint4*>(A.desc + (om + idx) * 32)[h] = vd;
        }
#pragma unroll
        for (int u = 0; u < 2; u++)
            if (t + 256 * u < 3 * np) A.pos[3 * (om + pi[u]) + pe[u]] = pv[u];
        return;
    }
    x -= G.e_set - G.e_new;
    const long long ok = (long long)b * (A.kf_cap + 1);
    if (x < G.e_kf - G.e_set) {
        // Map::AddKeyFrame: slot rows at the tail of kf_mp, their offsets and flags
        const int nk = H->nkf1 - H->nkf0;
        if (nk <= 0) return;
        const int n = H->ns1 - H->ns0, k0 = x * WG_WORDS;
        if (x == 0) {
            const int tc = min(t, nk);
            const int off = sec<int32_t>(A, H->kf_off)[tc];
            const uint8_t bad = sec<uint8_t>(A, H->kf_bad)[min(t, nk - 1)];
            if (t <= nk) {
                A.kf_mp_off[ok + H->nkf0 + t] = off;
                if (!H->has_cov) A.kf_cov_off[ok + H->nkf0 + t] = H->nc0;  // empty lists
            }
            if (t < nk) A.kf_bad[(long long)b * A.kf_cap + H->nkf0 + t] = bad;
        }
        if (k0 < n)
            copy_words(sec<int32_t>(A, H->kf_mp) + k0, A.kf_mp + (long long)b * A.slot_cap + H->ns0 + k0,
                       min(WG_WORDS, n - k0));
        return;
    }
    x -= G.e_kf - G.e_set;
    if (x < G.e_slot - G.e_kf) {
        // AddMapPoint / ReplaceMapPointMatch / EraseMapPointMatch on existing keyframes
        const int n = H->n_slot, k0 = x * SLOT_WRITES;
        if (k0 >= n) return;
        const int32_t* sp = sec<int32_t>(A, H->slot_pos);
        const int32_t* sv = sec<int32_t>(A, H->slot_val);
        int32_t* dst = A.kf_mp + (long long)b * A.slot_cap;
        int p[MU_U], v[MU_U];
#pragma unroll
        for (int u = 0; u < MU_U; u++) {
            const int i = min(k0 + t + 256 * u, n - 1);
            p[u] = sp[i];
            v[u] = sv[i];
        }
#pragma unroll
        for (int u = 0; u < MU_U; u++)
            if (k0 + t + 256 * u < n) dst[p[u]] = v[u];
        return;
    }
    x -= G.e_slot - G.e_kf;
    // mvpOrderedConnectedKeyFrames of every keyframe
    if (!H->has_cov) return;
    if (x == 0) {
        const int v = sec<int32_t>(A, H->cov_off)[min(t, H->nkf1)];
        if (t <= H->nkf1) A.kf_cov_off[ok + t] = v;
    }
    const int n = H->nc1, k0 = x * WG_WORDS;
    if (k0 < n)
        copy_words(sec<int32_t>(A, H->cov) + k0, A.kf_cov + (long long)b * A.kf_cap * A.kf_cap + k0,
                   min(WG_WORDS, n - k0));
}

// Row length of point p after the delta, from its replaced row or its old one.
__global__ __launch_bounds__(256) void k_mu_obs_scan(MapUpdateArgs A) {
    __shared__ int s_wave[4];
    const int l = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const MuHdr* H = hdr_of(A, l);
    if (!H->do_obs) return;  // uniform
    const int n = H->nmp1, n0 = H->nmp0;
    const int32_t* row_of = sec<int32_t>(A, H->row_of);
    const int32_t* doff = sec<int32_t>(A, H->obs_off);
    const int32_t* ooff = A.mp_obs_off + (long long)H->stream * (A.M + 1);
    int32_t* out = A.obs_off_new + (long long)l * (A.M + 1);
    int carry = 0;
    for (int base = 0; base < n; base += 256 * SCAN_PTS) {
        const int p0 = base + SCAN_PTS * t;
        int ro[SCAN_PTS], oo[SCAN_PTS + 1], len[SCAN_PTS];
#pragma unroll
        for (int k = 0; k < SCAN_PTS; k++) ro[k] = row_of[min(p0 + k, n - 1)];
#pragma unroll
        for (int k = 0; k <= SCAN_PTS; k++) oo[k] = n0 > 0 ? ooff[min(p0 + k, n0)] : 0;
#pragma unroll
        for (int k = 0; k < SCAN_PTS; k++) {
            const int r = max(ro[k], 0);
            const int dl = doff[r + 1] - doff[r];  // row 0 exists whenever a row is replaced; unused otherwise
            len[k] = p0 + k >= n ? 0 : (ro[k] >= 0 ? dl : (p0 + k < n0 ? oo[k + 1] - oo[k] : 0));
        }
        int sum = 0;
#pragma unroll
        for (int k = 0; k < SCAN_PTS; k++) sum += len[k];
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
            if (p0 + k < n) out[p0 + k] = run;
            run += len[k];
        }
        carry += total;
        __syncthreads();
    }
    if (t == 0) out[n] = carry;
}

__global__ __launch_bounds__(256) void k_mu_obs_rows(MapUpdateArgs A) {
    __shared__ int s_new[OBS_PTS + 1];
    __shared__ int s_src[OBS_PTS];  // >= 0: offset in the old table; < 0: -(offset in the delta's rows) - 1
    const int l = blockIdx.y, t = threadIdx.x;
    const MuHdr* H = hdr_of(A, l);
    if (!H->do_obs) return;  // uniform
    const int p0 = blockIdx.x * OBS_PTS;
    if (p0 >= H->nmp1) return;
    const int np = min(OBS_PTS, H->nmp1 - p0), n0 = H->nmp0;
    const long long b = H->stream;
    const int32_t* off_new = A.obs_off_new + (long long)l * (A.M + 1) + p0;
    const int32_t* old_obs = A.mp_obs + b * A.slot_cap;
    const int32_t* new_obs = sec<int32_t>(A, H->obs_kf);
    {
        const int p = p0 + min(t, np - 1);
        const int ro = sec<int32_t>(A, H->row_of)[p];
        const int oo = n0 > 0 ? A.mp_obs_off[b * (A.M + 1) + min(p, n0)] : 0;
        const int dn = sec<int32_t>(A, H->obs_off)[max(ro, 0)];
        const int on = off_new[min(t, np)];
        const int last = off_new[np];
        s_src[t] = ro >= 0 ? -dn - 1 : oo;
        s_new[t] = on;
        if (t == 0) s_new[np] = last;
    }
    __syncthreads();
    const int j0 = s_new[0], cnt = s_new[np] - j0;
    int32_t* dst = A.obs_new + (long long)l * A.slot_cap + j0;
    for (int i0 = t; i0 < cnt; i0 += 256 * MU_U) {
        int v[MU_U];
#pragma unroll
        for (int u = 0; u < MU_U; u++) {
            const int j = j0 + min(i0 + 256 * u, cnt - 1);
            int lo = 0, hi = np;  // the last q with s_new[q] <= j: its row holds j (empty rows share an offset)
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (s_new[mid] <= j) lo = mid; else hi = mid;
            }
            const int src = s_src[lo], k = j - s_new[lo];
            v[u] = src >= 0 ? old_obs[src + k] : new_obs[-src - 1 + k];
        }
#pragma unroll
        for (int u = 0; u < MU_U; u++)
            if (i0 + 256 * u < cnt) dst[i0 + 256 * u] = v[u];
    }
}

__global__ __launch_bounds__(256) void k_mu_finish(MapUpdateArgs A, FinSeg G) {
    const int l = blockIdx.y, t = threadIdx.x;
    const MuHdr* H = hdr_of(A, l);
    const long long b = H->stream, om = b * A.M;
    int x = blockIdx.x;
    if (x < G.e_home) {
        // the rebuilt rows home (both sides 16-byte aligned: slot_cap is a multiple of 64) and their offsets
        if (!H->do_obs) return;
        const int n = H->no1, nv = n >> 2, k0 = x * (WG_WORDS / 4);
        const int32_t* src = A.obs_new + (long long)l * A.slot_cap;
        int32_t* dst = A.mp_obs + b * A.slot_cap;
        if (k0 < nv)
            copy_words(reinterpret_cast<const uint4*>(src) + k0, reinterpret_cast<uint4*>(dst) + k0,
                       min(WG_WORDS / 4, nv - k0));
        if (x == 0) {
            const int tail = n & 3, i = 4 * nv + min(t, max(tail - 1, 0));
            const int v = n > 0 ? src[min(i, n - 1)] : 0;
            if (t < tail) dst[i] = v;
        }
        const int no = H->nmp1 + 1, o0 = x * WG_WORDS;
        if (o0 < no)
            copy_words(A.obs_off_new + (long long)l * (A.M + 1) + o0, A.mp_obs_off + b * (A.M + 1) + o0,
                       min(WG_WORDS, no - o0));
        return;
    }
    x -= G.e_home;
    if (x < G.e_last - G.e_home) {
        // mLastFrame's points read their position through the MapPoint*: refresh the cache
        if (H->n_set <= 0) return;
        const int n = min(max(A.last_nkp[b], 0), A.cap), k0 = x * SLOT_WRITES;
        if (k0 >= n) return;
        const long long o = b * A.cap;
        int mp[MU_U];
        float3 pos[MU_U];
#pragma unroll
        for (int u = 0; u < MU_U; u++) mp[u] = A.last_kp2mp[o + min(k0 + t + 256 * u, n - 1)];
#pragma unroll
        for (int u = 0; u < MU_U; u++) {
            const gf_map_point& P = A.map[om + min(max(mp[u], 0), A.M - 1)];
            pos[u] = make_float3(P.pos[0], P.pos[1], P.pos[2]);
        }
#pragma unroll
        for (int u = 0; u < MU_U; u++) {
            const int i = k0 + t + 256 * u;
            if (i >= n || mp[u] < 0 || mp[u] >= A.M) continue;
            float* p = A.last_pos + 3 * (o + i);
            p[0] = pos[u].x;
            p[1] = pos[u].y;
            p[2] = pos[u].z;
        }
        return;
    }
    // SetBadFlag of points and keyframes, and the counts the step reads
    for (int i0 = t; i0 < H->n_bad_mp; i0 += 256 * MU_U) {
        int v[MU_U];
#pragma unroll
        for (int u = 0; u < MU_U; u++) v[u] = sec<int32_t>(A, H->bad_mp)[min(i0 + 256 * u, H->n_bad_mp - 1)];
#pragma unroll
        for (int u = 0; u < MU_U; u++)
            if (i0 + 256 * u < H->n_bad_mp) A.mp_bad[om + v[u]] = 1;
    }
    if (t < H->n_bad_kf) A.kf_bad[b * A.kf_cap + sec<int32_t>(A, H->bad_kf)[t]] = 1;
    if (t == 0) {
        A.nmp[b] = H->nmp1;
        A.kfc[b] = H->nkf1;
        A.covis[b].nkf = H->nkf1;
        A.covis[b].nmp = H->nmp1;
    }
}

inline int cdiv(int a, int b) { return (a + b - 1) / b; }

}  // namespace

namespace gf {

int map_update_launch(gf_ctx* ctx, const MapUpdateArgs& a, const MapUpdateShape& sh, hipStream_t s) {
    RowSeg r;
    r.e_new = cdiv(sh.new_mp, PT_ROWS);
    r.e_set = r.e_new + cdiv(sh.set_mp, PT_ROWS);
    r.e_kf = r.e_set + (sh.any_new_kf ? std::max(1, cdiv(sh.new_slots, WG_WORDS)) : 0);
    r.e_slot = r.e_kf + cdiv(sh.slot_writes, SLOT_WRITES);
    r.e_cov = r.e_slot + (sh.any_cov ? std::max(1, cdiv(sh.cov, WG_WORDS)) : 0);
    if (r.e_cov > 0) {
        GF_PROF(ctx, s, "k_mu_rows");
        GF_LAUNCH(k_mu_rows, dim3(r.e_cov, a.L), 256, 0, s, a, r);
        GF_HIP(hipGetLastError());
    }
    if (sh.any_obs) {
        {
            GF_PROF(ctx, s, "k_mu_obs_scan");
            GF_LAUNCH(k_mu_obs_scan, a.L, 256, 0, s, a);
            GF_HIP(hipGetLastError());
        }
        GF_PROF(ctx, s, "k_mu_obs_rows");
        GF_LAUNCH(k_mu_obs_rows, dim3(std::max(1, cdiv(sh.nmp1, OBS_PTS)), a.L), 256, 0, s, a);
        GF_HIP(hipGetLastError());
    }
    FinSeg f;
    f.e_home = sh.any_obs ? std::max(1, std::max(cdiv(sh.no1, WG_WORDS), cdiv(sh.nmp1 + 1, WG_WORDS))) : 0;
    f.e_last = f.e_home + (sh.set_mp > 0 ? cdiv(a.cap, SLOT_WRITES) : 0);
    f.e_flags = f.e_last + 1;
    GF_PROF(ctx, s, "k_mu_finish");
    GF_LAUNCH(k_mu_finish, dim3(f.e_flags, a.L), 256, 0, s, a, f);
    GF_HIP(hipGetLastError());
    return GF_OK;
}

}  // namespace gf
