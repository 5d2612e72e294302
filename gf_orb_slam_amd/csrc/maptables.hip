// Resident map tables: the flat tables of kfcull.hip / covis.hip / lbagraph.hip
// kept on the device and updated in place by a journal of the map's own writes
// (gf_orb_slam_amd/maptables.py). The observation table is a slack CSR:
// obs_off[p] .. obs_off[p + 1] is the capacity of row p, inside it the live
// entries in ascending order of the global keypoint index (= observation-map
// order), then -1 up to the capacity. The consumers skip -1 and need no change.
//
//   k_tables_apply: one journal. The first nrows workgroups own one touched
//     row each (a workgroup is one wavefront, so its barrier is a wave barrier):
//     the row's live entries are compacted into LDS by ballot and prefix
//     popcount, the row's ops are applied serially in journal order
//     (MapPoint::AddObservation, which overwrites, src/MapPoint.cc:77-81;
//     EraseObservation's erase, :83-103; the clear() of SetBadFlag, :117-131,
//     and Replace, :136-170) and the whole capacity is written back, live
//     entries first. The place of a new entry is the number of entries below
//     its keyframe's range, counted by ballot over 64-entry chunks; the tail is
//     shifted a chunk at a time. The workgroups after those scatter the slot
//     writes (KeyFrame::AddMapPoint / EraseMapPointMatch /
//     ReplaceMapPointMatch) and the bad flags, one lane per op.
//   k_tables_move: the regrow. Eight lanes per row (rows average eight
//     entries), two passes over the old row: the live count, then the compacted
//     copy to the row's new start and -1 over the rest of the new capacity.
//
// Every id is bounds-tested where it is read; the two counters of status are
// integer atomic adds, so they do not depend on the order of arrival.
#include <vector>

#include "common.h"

#define MT_THREADS 64
#define MT_ROW GF_MT_ROW
#define MT_SUB 8  // lanes per row of k_tables_move
#define MT_MOVE_THREADS 256

namespace {

__device__ __forceinline__ int mt_below(unsigned long long mask, int lane) {
    return __popcll(mask & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(MT_THREADS) void k_tables_apply(
    int nkf, int nkp, const int32_t* __restrict__ kf_off, int32_t* __restrict__ slots, int nmp,
    uint8_t* __restrict__ mp_bad, const int32_t* __restrict__ obs_off, int32_t* obs_gkp, int nobs, int nslot,
    const int32_t* __restrict__ slot_g, const int32_t* __restrict__ slot_v, int nbad, const int32_t* __restrict__ bad_p,
    int nrows, const int32_t* __restrict__ row_ids, const int32_t* __restrict__ row_op_off, int nops,
    const int32_t* __restrict__ ops, int32_t* status) {
    __shared__ int buf[MT_ROW];
    const int lane = threadIdx.x, b = blockIdx.x;
    if (b >= nrows) {  // the slot and bad-flag scatter: unique targets, one lane per op
        const int i = (b - nrows) * MT_THREADS + lane;
        int skipped = 0;
        if (i < nslot) {
            const int g = gfd::ldg(slot_g + i), v = gfd::ldg(slot_v + i);
            if (g >= 0 && g < nkp)
                slots[g] = v;
            else
                skipped = 1;
        } else if (i - nslot < nbad) {
            const int p = gfd::ldg(bad_p + (i - nslot));
            if (p >= 0 && p < nmp)
                mp_bad[p] = 1;
            else
                skipped = 1;
        }
        skipped = gfd::warp_sum(skipped);
        if (lane == 0 && skipped) atomicAdd(status + 1, skipped);
        return;
    }
    // one touched row; everything below but `lane` is the same in every lane
    const int p = gfd::ldg(row_ids + b);
    const int o0 = min(max(gfd::ldg(row_op_off + b), 0), nops);
    const int o1 = min(max(gfd::ldg(row_op_off + b + 1), o0), nops);
    if (p < 0 || p >= nmp) {
        if (lane == 0 && o1 > o0) atomicAdd(status + 1, o1 - o0);
        return;
    }
    const int r0 = min(max(gfd::ldg(obs_off + p), 0), nobs);
    const int r1 = min(max(gfd::ldg(obs_off + p + 1), r0), nobs);
    const int cap = r1 - r0;
    int n = 0;
    for (int c = 0; c < cap; c += MT_THREADS) {
        const int v = c + lane < cap ? gfd::ldg(obs_gkp + r0 + c + lane) : -1;
        const unsigned long long m = __ballot(v >= 0);
        const int at = n + mt_below(m, lane);
        if (v >= 0 && at < MT_ROW) buf[at] = v;
        n += __popcll(m);
    }
    bool over = n > MT_ROW;
    int skipped = 0;
    __syncthreads();
    for (int j = o0; j < o1 && !over; j++) {
        const int kind = gfd::ldg(ops + 3 * (size_t)j), kf = gfd::ldg(ops + 3 * (size_t)j + 1),
                  idx = gfd::ldg(ops + 3 * (size_t)j + 2);
        if (kind == GF_MT_OBS_CLEAR) {
            n = 0;
            continue;
        }
        if ((kind != GF_MT_OBS_SET && kind != GF_MT_OBS_ERASE) || kf < 0 || kf >= nkf) {
            skipped++;
            continue;
        }
        const int lo = gfd::ldg(kf_off + kf), hi = gfd::ldg(kf_off + kf + 1);
        if (kind == GF_MT_OBS_SET && (idx < 0 || idx >= hi - lo || lo < 0 || hi > nkp)) {
            skipped++;
            continue;
        }
        // the entry of this keyframe, and how many entries lie below its range
        int below = 0, hit = -1;
        for (int c = 0; c < n; c += MT_THREADS) {
            const int v = c + lane < n ? buf[c + lane] : 0x7fffffff;
            below += __popcll(__ballot(v < lo));
            const unsigned long long h = __ballot(v >= lo && v < hi);
            if (h && hit < 0) hit = c + __ffsll((long long)h) - 1;
        }
        if (kind == GF_MT_OBS_SET) {
            if (hit < 0) {
                if (n + 1 > MT_ROW) {
                    over = true;
                    break;
                }
                for (int e = n; e > below; e -= MT_THREADS) {  // the tail one place up, the top chunk first
                    const int i = e - 1 - lane;
                    const int v = i >= below ? buf[i] : 0;
                    __syncthreads();
                    if (i >= below) buf[i + 1] = v;
                    __syncthreads();
                }
                hit = below;
                n++;
            }
            if (lane == 0) buf[hit] = lo + idx;
            __syncthreads();
        } else if (hit >= 0) {
            for (int c = hit; c < n - 1; c += MT_THREADS) {  // the tail one place down, the bottom chunk first
                const int i = c + lane;
                const int v = i + 1 < n ? buf[i + 1] : 0;
                __syncthreads();
                if (i + 1 < n) buf[i] = v;
                __syncthreads();
            }
            n--;
        }
    }
    if (lane == 0 && skipped) atomicAdd(status + 1, skipped);
    if (over || n > cap) {  // nothing of the row was written
        if (lane == 0) atomicAdd(status, 1);
        return;
    }
    for (int i = lane; i < cap; i += MT_THREADS) obs_gkp[r0 + i] = i < n ? buf[i] : -1;
}

__global__ __launch_bounds__(MT_MOVE_THREADS) void k_tables_move(
    int nmp, const int32_t* __restrict__ old_off, const int32_t* __restrict__ old_gkp, int nobs_old,
    const int32_t* __restrict__ new_off, int32_t* __restrict__ new_gkp, int nobs_new, int32_t* status) {
    const int p = (int)(((size_t)blockIdx.x * MT_MOVE_THREADS + threadIdx.x) / MT_SUB);
    const int sub = threadIdx.x % MT_SUB;
    const int shift = (threadIdx.x & 63) - sub;  // the first lane of this row's group in the wavefront
    const bool has = p < nmp;
    int o0 = 0, o1 = 0, n0 = 0, n1 = 0;
    if (has) {
        o0 = min(max(gfd::ldg(old_off + p), 0), nobs_old);
        o1 = min(max(gfd::ldg(old_off + p + 1), o0), nobs_old);
        n0 = min(max(gfd::ldg(new_off + p), 0), nobs_new);
        n1 = min(max(gfd::ldg(new_off + p + 1), n0), nobs_new);
    }
    const int ocap = o1 - o0, ncap = n1 - n0;
    int live = 0;
    for (int c = 0; __any(c < ocap); c += MT_SUB) {
        const int v = c + sub < ocap ? gfd::ldg(old_gkp + o0 + c + sub) : -1;
        live += __popc((unsigned)(__ballot(v >= 0) >> shift) & 0xffu);
    }
    const bool fits = live <= ncap;
    if (has && !fits && sub == 0) atomicAdd(status, 1);
    int n = 0;
    for (int c = 0; __any(fits && c < ocap); c += MT_SUB) {
        const int v = fits && c + sub < ocap ? gfd::ldg(old_gkp + o0 + c + sub) : -1;
        const unsigned m = (unsigned)(__ballot(v >= 0) >> shift) & 0xffu;
        if (v >= 0) new_gkp[n0 + n + __popc(m & ((1u << sub) - 1u))] = v;
        n += __popc(m);
    }
    for (int i = n + sub; i < ncap; i += MT_SUB) new_gkp[n0 + i] = -1;
}

}  // namespace

extern "C" {

// one journal applied to device tables (MapPoint.cc:77-81, :83-103, :117-131, :136-170; KeyFrame::AddMapPoint,
// EraseMapPointMatch, ReplaceMapPointMatch)
int gf_map_tables_apply_dev(gf_ctx* ctx, int nkf, int nkp, const int32_t* d_kf_off, int32_t* d_slots, int nmp,
                            uint8_t* d_mp_bad, const int32_t* d_obs_off, int32_t* d_obs_gkp, int nobs, int nslot,
                            const int32_t* d_slot_g, const int32_t* d_slot_v, int nbad, const int32_t* d_bad_p,
                            int nrows, const int32_t* d_row_ids, const int32_t* d_row_op_off, int nops,
                            const int32_t* d_ops, int32_t* d_status, void* stream) {
    GF_CHECK(ctx && d_status, GF_ERR_ARG, "gf_map_tables_apply_dev: null arg");
    GF_CHECK(nkf >= 0 && nkp >= 0 && nmp >= 0 && nobs >= 0 && nslot >= 0 && nbad >= 0 && nrows >= 0 && nops >= 0,
             GF_ERR_ARG, "gf_map_tables_apply_dev: negative size");
    GF_CHECK(nslot == 0 || (d_slot_g && d_slot_v), GF_ERR_ARG, "gf_map_tables_apply_dev: null slot ops");
    GF_CHECK(nbad == 0 || d_bad_p, GF_ERR_ARG, "gf_map_tables_apply_dev: null bad ops");
    GF_CHECK(nrows == 0 || (d_row_ids && d_row_op_off && d_kf_off), GF_ERR_ARG, "gf_map_tables_apply_dev: null row ops");
    GF_CHECK(nops == 0 || d_ops, GF_ERR_ARG, "gf_map_tables_apply_dev: null ops");
    GF_CHECK(nkp == 0 || d_slots, GF_ERR_ARG, "gf_map_tables_apply_dev: null keyframe table");
    GF_CHECK(nmp == 0 || (d_mp_bad && d_obs_off), GF_ERR_ARG, "gf_map_tables_apply_dev: null point table");
    GF_CHECK(nobs == 0 || d_obs_gkp, GF_ERR_ARG, "gf_map_tables_apply_dev: null observation table");
    hipStream_t s = (hipStream_t)stream;
    GF_HIP(hipMemsetAsync(d_status, 0, 2 * sizeof(int32_t), s));
    const long long scatter = ((long long)nslot + nbad + MT_THREADS - 1) / MT_THREADS;
    if (nrows + scatter == 0) return GF_OK;
    GF_PROF(ctx, s, "k_tables_apply");
    GF_LAUNCH(k_tables_apply, (unsigned)(nrows + scatter), MT_THREADS, 0, s, nkf, nkp, d_kf_off, d_slots, nmp, d_mp_bad,
              d_obs_off, d_obs_gkp, nobs, nslot, d_slot_g, d_slot_v, nbad, d_bad_p, nrows, d_row_ids, d_row_op_off, nops,
              d_ops, d_status);
    GF_HIP(hipGetLastError());
    return GF_OK;
}

// the regrow of the slack CSR on device tables
int gf_map_tables_move_dev(gf_ctx* ctx, int nmp, const int32_t* d_old_off, const int32_t* d_old_gkp, int nobs_old,
                           const int32_t* d_new_off, int32_t* d_new_gkp, int nobs_new, int32_t* d_status,
                           void* stream) {
    GF_CHECK(ctx && d_status, GF_ERR_ARG, "gf_map_tables_move_dev: null arg");
    GF_CHECK(nmp >= 0 && nobs_old >= 0 && nobs_new >= 0, GF_ERR_ARG, "gf_map_tables_move_dev: negative size");
    GF_CHECK(nmp == 0 || (d_old_off && d_new_off), GF_ERR_ARG, "gf_map_tables_move_dev: null offsets");
    GF_CHECK(nobs_old == 0 || d_old_gkp, GF_ERR_ARG, "gf_map_tables_move_dev: null old table");
    GF_CHECK(nobs_new == 0 || d_new_gkp, GF_ERR_ARG, "gf_map_tables_move_dev: null new table");
    hipStream_t s = (hipStream_t)stream;
    GF_HIP(hipMemsetAsync(d_status, 0, sizeof(int32_t), s));
    if (nmp == 0) return GF_OK;
    const long long blocks = ((long long)nmp * MT_SUB + MT_MOVE_THREADS - 1) / MT_MOVE_THREADS;
    GF_PROF(ctx, s, "k_tables_move");
    GF_LAUNCH(k_tables_move, (unsigned)blocks, MT_MOVE_THREADS, 0, s, nmp, d_old_off, d_old_gkp, nobs_old, d_new_off,
              d_new_gkp, nobs_new, d_status);
    GF_HIP(hipGetLastError());
    return GF_OK;
}

}  // extern "C"

namespace {

// offsets that start at 0 and do not decrease -> their total, or -1
long long mt_total(const int32_t* off, int n) {
    if (off[0] != 0) return -1;
    for (int i = 0; i < n; i++)
        if (off[i + 1] < off[i]) return -1;
    return off[n];
}

struct Parts {
    size_t off = 0;
    std::vector<std::pair<const void*, size_t>> parts;
    size_t add(const void* h, size_t bytes) {
        const size_t o = off;
        parts.push_back({h, bytes});
        off += (bytes + 15) & ~(size_t)15;
        return o;
    }
    int upload(uint8_t* base, hipStream_t s) const {
        size_t cur = 0;
        for (auto& pr : parts) {
            if (pr.second && pr.first) GF_HIP(hipMemcpyAsync(base + cur, pr.first, pr.second, hipMemcpyHostToDevice, s));
            cur += (pr.second + 15) & ~(size_t)15;
        }
        return GF_OK;
    }
};

}  // namespace

extern "C" {

// one journal on host arrays, synchronous
int gf_map_tables_apply(gf_ctx* ctx, int nkf, const int32_t* kf_off, int32_t* slots, int nmp, uint8_t* mp_bad,
                        const int32_t* obs_off, int32_t* obs_gkp, int nslot, const int32_t* slot_g,
                        const int32_t* slot_v, int nbad, const int32_t* bad_p, int nrows, const int32_t* row_ids,
                        const int32_t* row_op_off, int nops, const int32_t* ops, int32_t* status) {
    GF_CHECK(ctx && status && kf_off, GF_ERR_ARG, "gf_map_tables_apply: null arg");
    GF_CHECK(nkf >= 0 && nmp >= 0 && nslot >= 0 && nbad >= 0 && nrows >= 0 && nops >= 0, GF_ERR_ARG,
             "gf_map_tables_apply: negative size");
    const long long nkp = mt_total(kf_off, nkf);
    GF_CHECK(nkp >= 0, GF_ERR_ARG, "kf_off must start at 0 and be non-decreasing");
    GF_CHECK(nkp == 0 || slots, GF_ERR_ARG, "gf_map_tables_apply: null keyframe table");
    GF_CHECK(nmp == 0 || (mp_bad && obs_off), GF_ERR_ARG, "gf_map_tables_apply: null point table");
    const long long nobs = nmp ? mt_total(obs_off, nmp) : 0;
    GF_CHECK(nobs >= 0, GF_ERR_ARG, "obs_off must start at 0 and be non-decreasing");
    GF_CHECK(nobs == 0 || obs_gkp, GF_ERR_ARG, "gf_map_tables_apply: null observation table");
    GF_CHECK(nslot == 0 || (slot_g && slot_v), GF_ERR_ARG, "gf_map_tables_apply: null slot ops");
    GF_CHECK(nbad == 0 || bad_p, GF_ERR_ARG, "gf_map_tables_apply: null bad ops");
    GF_CHECK(nrows == 0 || (row_ids && row_op_off), GF_ERR_ARG, "gf_map_tables_apply: null row ops");
    GF_CHECK(nops == 0 || ops, GF_ERR_ARG, "gf_map_tables_apply: null ops");
    if (nrows) GF_CHECK(mt_total(row_op_off, nrows) == nops, GF_ERR_ARG, "row_op_off must start at 0 and end at nops");
    else GF_CHECK(nops == 0, GF_ERR_ARG, "ops without rows");
    for (int r = 1; r < nrows; r++) GF_CHECK(row_ids[r] > row_ids[r - 1], GF_ERR_ARG, "row_ids must strictly increase");
    {
        std::vector<uint8_t> seen((size_t)nkp, 0);
        for (int i = 0; i < nslot; i++) {
            const int g = slot_g[i];
            if (g < 0 || g >= nkp) continue;
            GF_CHECK(!seen[g], GF_ERR_ARG, "a slot is written twice in one journal");
            seen[g] = 1;
        }
    }
    status[0] = status[1] = 0;
    if (nrows + nslot + nbad == 0) return GF_OK;
    GF_HIP(hipSetDevice(ctx->device));
    // one scratch block: [kf_off | slots | mp_bad | obs_off | obs_gkp | slot_g | slot_v | bad_p | row_ids | row_op_off |
    // ops | status]
    Parts P;
    const size_t NK = (size_t)nkp, NM = (size_t)nmp, NO = (size_t)nobs;
    const size_t o_ko = P.add(kf_off, 4 * ((size_t)nkf + 1)), o_sl = P.add(slots, 4 * NK), o_mb = P.add(mp_bad, NM),
                 o_oo = P.add(nmp ? obs_off : nullptr, nmp ? 4 * (NM + 1) : 0), o_og = P.add(obs_gkp, 4 * NO),
                 o_sg = P.add(slot_g, 4 * (size_t)nslot), o_sv = P.add(slot_v, 4 * (size_t)nslot),
                 o_bp = P.add(bad_p, 4 * (size_t)nbad), o_ri = P.add(row_ids, 4 * (size_t)nrows),
                 o_ro = P.add(nrows ? row_op_off : nullptr, nrows ? 4 * ((size_t)nrows + 1) : 0),
                 o_op = P.add(ops, 12 * (size_t)nops), o_st = P.add(nullptr, 8);
    void* dbuf;
    int rc = gf::ws_get(ctx, 73, P.off, &dbuf);
    if (rc) return rc;
    uint8_t* base = (uint8_t*)dbuf;
    hipStream_t s = ctx->stream;
    rc = P.upload(base, s);
    if (rc) return rc;
    auto I = [&](size_t o) { return (int32_t*)(base + o); };
    rc = gf_map_tables_apply_dev(ctx, nkf, (int)nkp, I(o_ko), I(o_sl), nmp, base + o_mb, I(o_oo), I(o_og), (int)nobs,
                                 nslot, I(o_sg), I(o_sv), nbad, I(o_bp), nrows, I(o_ri), I(o_ro), nops, I(o_op),
                                 I(o_st), s);
    if (rc) return rc;
    if (NK) GF_HIP(hipMemcpyAsync(slots, base + o_sl, 4 * NK, hipMemcpyDeviceToHost, s));
    if (NM) GF_HIP(hipMemcpyAsync(mp_bad, base + o_mb, NM, hipMemcpyDeviceToHost, s));
    if (NO) GF_HIP(hipMemcpyAsync(obs_gkp, base + o_og, 4 * NO, hipMemcpyDeviceToHost, s));
    GF_HIP(hipMemcpyAsync(status, base + o_st, 8, hipMemcpyDeviceToHost, s));
    GF_HIP(hipStreamSynchronize(s));
    return GF_OK;
}

// the regrow on host arrays, synchronous
int gf_map_tables_move(gf_ctx* ctx, int nmp, const int32_t* old_off, const int32_t* old_gkp, const int32_t* new_off,
                       int32_t* new_gkp, int32_t* status) {
    GF_CHECK(ctx && status, GF_ERR_ARG, "gf_map_tables_move: null arg");
    GF_CHECK(nmp >= 0, GF_ERR_ARG, "gf_map_tables_move: negative size");
    status[0] = 0;
    if (nmp == 0) return GF_OK;
    GF_CHECK(old_off && new_off, GF_ERR_ARG, "gf_map_tables_move: null offsets");
    const long long no = mt_total(old_off, nmp), nn = mt_total(new_off, nmp);
    GF_CHECK(no >= 0 && nn >= 0, GF_ERR_ARG, "the offsets must start at 0 and be non-decreasing");
    GF_CHECK((no == 0 || old_gkp) && (nn == 0 || new_gkp), GF_ERR_ARG, "gf_map_tables_move: null table");
    GF_HIP(hipSetDevice(ctx->device));
    // one scratch block: [old_off | old_gkp | new_off | new_gkp | status]
    Parts P;
    const size_t NM = (size_t)nmp;
    const size_t o_oo = P.add(old_off, 4 * (NM + 1)), o_og = P.add(old_gkp, 4 * (size_t)no),
                 o_no = P.add(new_off, 4 * (NM + 1)), o_ng = P.add(nullptr, 4 * (size_t)nn), o_st = P.add(nullptr, 4);
    void* dbuf;
    int rc = gf::ws_get(ctx, 74, P.off, &dbuf);
    if (rc) return rc;
    uint8_t* base = (uint8_t*)dbuf;
    hipStream_t s = ctx->stream;
    rc = P.upload(base, s);
    if (rc) return rc;
    auto I = [&](size_t o) { return (int32_t*)(base + o); };
    rc = gf_map_tables_move_dev(ctx, nmp, I(o_oo), I(o_og), (int)no, I(o_no), I(o_ng), (int)nn, I(o_st), s);
    if (rc) return rc;
    if (nn) GF_HIP(hipMemcpyAsync(new_gkp, base + o_ng, 4 * (size_t)nn, hipMemcpyDeviceToHost, s));
    GF_HIP(hipMemcpyAsync(status, base + o_st, 4, hipMemcpyDeviceToHost, s));
    GF_HIP(hipStreamSynchronize(s));
    return GF_OK;
}

}  // extern "C"
