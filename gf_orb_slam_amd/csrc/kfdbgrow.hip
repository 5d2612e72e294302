// A relocalisation keyframe database that grows (gf_kfdb_create_growable,
// gf_kfdb_append, gf_frontend_update_maps_kfdb): KeyFrameDatabase::add
// (KeyFrameDatabase.cc:39-45) for the keyframes the mapper hands back, on the
// layout reloc_candidates_wave reads (reloc.hip): inv_words ascending, the CSR
// inv_off / inv_kf, every word's list in keyframe-index order.
//
// The host validates the new keyframes' rows and merges their BowVectors into a
// delta inverted file (u ascending, CSR uoff / ukf: the cost of the new rows
// alone). The device merges it into the resident one. A new keyframe has the
// highest index, so it joins the tail of every list it is on; with E[u] the
// number of new-only words among u[0 .. u) and p(w) the words of the old file
// below w:
//   old word i      -> word i + E[c], list start inv_off[i] + uoff[c],
//                      c = the delta words below it
//   new-only word u -> word p + E[u], list start inv_off[p] + uoff[u]
//   delta list u    -> behind the old list of its word, if it has one
// Every destination has one writer (no atomics), and the shifts overlap, so the
// merged file is written into the database's second set of buffers and the
// record the step reads (KfdbDev, in device memory) is flipped last.
//   k_kg_scan    one workgroup per database: each delta word's place in the old
//                file by binary search, the new-only flags scanned (wave scan,
//                four waves through LDS) into E
//   k_kg_merge   (chunk x database): the keyframes' rows to the tails of the
//                row arrays with their offsets rebased, then the merged file
//   k_kg_finish  one wave per database: the record(s) flipped, the appended
//                keyframes' query state zeroed (mnRelocQuery of a new KeyFrame)
// Grids are (chunk x database), so the streams of one update_maps call share
// one set of launches.
#include <algorithm>
#include <cstring>

#include "reloc.h"

namespace {

using gf::KfdbDev;

constexpr int KG_NSEC = 10;      // row sections of a database
constexpr int KG_CHUNK = 1024;   // items per workgroup the merge grid is sized for
constexpr int KG_MAX_X = 32;     // merge workgroups per database at most

// n words from the staging image at src to dst, each plus add (the rebase of an offset section)
struct KgSec {
    int64_t src;
    int32_t* dst;
    int32_t n, add;
};

// One database of a call, at the head of the staging image; section offsets in
// bytes from its base, 16-byte aligned.
struct KgHdr {
    KfdbDev* rec[2];  // the records to flip: the database's own, the front end's stream record or null
    KfdbDev next;     // the record after the append but for nw
    int32_t *inv_words1, *inv_off1, *inv_kf1;  // the merged file's buffers (= next's)
    int32_t *scan, *pos;                       // E [nu + 1]; p or ~p (new-only) [nu]
    gf_reloc_kf* rkf;                          // the stream's query state or null
    int32_t nkf0, nkn, nu, ni0;                // keyframes before, appended; delta words; old list entries
    int64_t u, uoff, ukf;
    KgSec sec[KG_NSEC];
};

inline size_t a16(size_t n) { return (n + 15) & ~(size_t)15; }

__device__ __forceinline__ int lower_bound_w(const int32_t* a, int n, int w) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < w) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void k_kg_scan(const uint8_t* stage) {
    __shared__ int s_wave[4];
    const KgHdr* H = reinterpret_cast<const KgHdr*>(stage) + blockIdx.x;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const KfdbDev* cur = H->rec[0];
    const int nw0 = cur->nw, nu = H->nu;
    const int32_t* W0 = cur->inv_words;
    const int32_t* U = reinterpret_cast<const int32_t*>(stage + H->u);
    int carry = 0;
    for (int base = 0; base < nu; base += 256) {
        const int u = base + t;
        int flag = 0, p = 0;
        if (u < nu) {
            const int w = U[u];
            p = lower_bound_w(W0, nw0, w);
            flag = !(p < nw0 && W0[p] == w);
        }
        int v = flag;  // inclusive scan over the wave, then over the four waves through LDS
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int x = __shfl_up(v, o, 64);
            if (lane >= o) v += x;
        }
        if (lane == 63) s_wave[wave] = v;
        __syncthreads();
        int wbase = 0, total = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            if (i < wave) wbase += s_wave[i];
            total += s_wave[i];
        }
        if (u < nu) {
            H->scan[u] = carry + wbase + v - flag;
            H->pos[u] = flag ? ~p : p;
        }
        carry += total;
        __syncthreads();
    }
    if (t == 0) H->scan[nu] = carry;
}

__global__ __launch_bounds__(256) void k_kg_merge(const uint8_t* stage) {
    const KgHdr* H = reinterpret_cast<const KgHdr*>(stage) + blockIdx.y;
    const int g = blockIdx.x * 256 + threadIdx.x, G = gridDim.x * 256;
    // KeyFrame rows: keypoints, descriptors, BowVector, FeatureVector to the tails
#pragma unroll 1
    for (int s = 0; s < KG_NSEC; s++) {
        const KgSec S = H->sec[s];
        const int32_t* src = reinterpret_cast<const int32_t*>(stage + S.src);
        for (int i = g; i < S.n; i += G) S.dst[i] = src[i] + S.add;
    }
    const KfdbDev* cur = H->rec[0];
    const int nw0 = cur->nw, nu = H->nu;
    const int32_t *W0 = cur->inv_words, *O0 = cur->inv_off, *K0 = cur->inv_kf;
    const int32_t* U = reinterpret_cast<const int32_t*>(stage + H->u);
    const int32_t* UO = reinterpret_cast<const int32_t*>(stage + H->uoff);
    const int32_t* UK = reinterpret_cast<const int32_t*>(stage + H->ukf);
    const int32_t *E = H->scan, *P = H->pos;
    int32_t *W1 = H->inv_words1, *O1 = H->inv_off1, *K1 = H->inv_kf1;
    // the old words and their lists (at most 64 keyframes a list)
    for (int i = g; i < nw0; i += G) {
        const int w = W0[i], o0 = O0[i], o1 = O0[i + 1];
        const int c = lower_bound_w(U, nu, w);
        const int j = i + E[c], d = o0 + UO[c];
        W1[j] = w;
        O1[j] = d;
        for (int e = o0; e < o1; e++) K1[d + e - o0] = K0[e];
    }
    // the delta's words: a new-only word with its list, else the list behind the old one
    for (int u = g; u < nu; u += G) {
        int p = P[u];
        const bool fresh = p < 0;
        if (fresh) p = ~p;
        const int a = UO[u], b = UO[u + 1];
        const int d = O0[fresh ? p : p + 1] + a;
        if (fresh) {
            const int j = p + E[u];
            W1[j] = U[u];
            O1[j] = d;
        }
        for (int e = a; e < b; e++) K1[d + e - a] = UK[e];
    }
    if (g == 0) O1[nw0 + E[nu]] = H->ni0 + UO[nu];
}

__global__ __launch_bounds__(64) void k_kg_finish(const uint8_t* stage) {
    const KgHdr* H = reinterpret_cast<const KgHdr*>(stage) + blockIdx.x;
    const int t = threadIdx.x;
    if (H->rkf) {
        uint32_t* z = reinterpret_cast<uint32_t*>(H->rkf + H->nkf0);
        const int n = H->nkn * (int)(sizeof(gf_reloc_kf) / 4);
        for (int i = t; i < n; i += 64) z[i] = 0u;
    }
    // the record word by word; the lane that holds nw reads the old count before it writes the new one
    constexpr int RW = (int)(sizeof(KfdbDev) / 4), NW_AT = (int)(offsetof(KfdbDev, nw) / 4);
    static_assert(sizeof(KfdbDev) % 4 == 0 && RW <= 64 && offsetof(KfdbDev, nw) % 4 == 0, "one record word per lane");
    if (t < RW) {
        int32_t* r0 = reinterpret_cast<int32_t*>(H->rec[0]);
        int32_t* r1 = reinterpret_cast<int32_t*>(H->rec[1]);
        int32_t w = reinterpret_cast<const int32_t*>(&H->next)[t];
        if (t == NW_AT) w = r0[NW_AT] + H->scan[H->nu];
        r0[t] = w;
        if (r1) r1[t] = w;
    }
}

inline int cdiv(int a, int b) { return (a + b - 1) / b; }

int grow_stage(gf_kfdb* d, size_t bytes) {
    if (bytes <= d->stage_bytes) return GF_OK;
    void* p = nullptr;
    GF_HIP(hipMalloc(&p, bytes));
    d->allocs.push_back(p);  // the smaller one goes with the database
    d->stage = (uint8_t*)p;
    d->stage_bytes = bytes;
    return GF_OK;
}

}  // namespace

namespace gf {

bool kfdb_growable(const gf_kfdb* db) { return db->growable; }
int kfdb_max_kf(const gf_kfdb* db) { return db->max_kf; }
bool kfdb_bound(const gf_kfdb* db) { return db->bound; }

int kfdb_bind(gf_kfdb* db, KfdbDev* rec) {
    GF_CHECK(!db->bound, GF_ERR_ARG, "a growable keyframe database belongs to one stream of one front end");
    GF_HIP(hipMemcpy(rec, db->d_rec, sizeof(KfdbDev), hipMemcpyDeviceToHost));
    db->dev = *rec;
    db->bound = true;
    return GF_OK;
}

void kfdb_unbind(gf_kfdb* db) { db->bound = false; }

KfdbHostCounts kfdb_host_counts(const gf_kfdb* db) {
    KfdbHostCounts c;
    c.nkf = db->dev.nkf;
    c.nk = db->nk;
    c.nb = db->nb;
    c.nn = db->nn;
    c.nf = db->nf;
    return c;
}

void kfdb_set_host_counts(gf_kfdb* db, const KfdbHostCounts& c) {
    db->dev.nkf = c.nkf;
    db->nk = c.nk;
    db->nb = c.nb;
    db->nn = c.nn;
    db->nf = c.nf;
}

KfdbDev* kfdb_record(gf_kfdb* db) { return db->d_rec; }

int kfdb_grow_validate(gf_kfdb* db, const gf_keyframe_db* rows, KfdbGrowPlan& P) {
    GF_CHECK(db && rows, GF_ERR_ARG, "null arg");
    GF_CHECK(db->growable, GF_ERR_ARG, "the keyframe database is fixed (gf_kfdb_create_growable makes one that grows)");
    GF_CHECK(rows->nkf >= 0, GF_ERR_ARG, "negative keyframe count");
    P.db = db;
    P.rows = rows;
    int rc = kfdb_validate(rows, P.nk, P.nb, P.nn, P.nf);
    if (rc) return rc;
    const int nkn = rows->nkf;
    if (nkn)
        GF_CHECK(rows->kp_off[0] == 0 && rows->bow_off[0] == 0 && rows->fv_off[0] == 0 && rows->fv_start[0] == 0,
                 GF_ERR_ARG, "the rows' offsets must start at 0");
    GF_CHECK(P.nb <= P.nk && P.nn <= P.nk && P.nf <= P.nk, GF_ERR_ARG,
             "a keyframe has at most one word, node and feature entry per keypoint");
    GF_CHECK((long long)db->dev.nkf + nkn <= db->max_kf, GF_ERR_CAP, "more keyframes than the database's max_kf");
    GF_CHECK((long long)db->nk + P.nk <= db->max_rows, GF_ERR_CAP, "more keypoints than the database's max_rows");
    // the new keyframes' inverted file
    std::vector<std::pair<int32_t, int32_t>> wk;
    wk.reserve(P.nb);
    for (int k = 0; k < nkn; k++)
        for (int e = rows->bow_off[k]; e < rows->bow_off[k + 1]; e++)
            wk.emplace_back(rows->bow_words[e], db->dev.nkf + k);
    std::sort(wk.begin(), wk.end());
    P.u.clear();
    P.uoff.assign(1, 0);
    P.ukf.clear();
    for (size_t i = 0; i < wk.size(); i++) {
        if (i == 0 || wk[i].first != wk[i - 1].first) {
            if (i) P.uoff.push_back((int32_t)P.ukf.size());
            P.u.push_back(wk[i].first);
        }
        P.ukf.push_back(wk[i].second);
    }
    if (!wk.empty()) P.uoff.push_back((int32_t)P.ukf.size());
    return GF_OK;
}

size_t kfdb_grow_hdr_bytes(int ndb) { return a16(sizeof(KgHdr) * (size_t)ndb); }

size_t kfdb_grow_bytes(const KfdbGrowPlan& P) {
    const size_t nkn = P.rows->nkf;
    return 3 * a16(4 * (nkn + 1)) + a16(sizeof(gf_keypoint) * (size_t)P.nk) + a16(32 * (size_t)P.nk) +
           a16(4 * (size_t)P.nb) + a16(8 * (size_t)P.nb) + a16(4 * (size_t)P.nn) + a16(4 * ((size_t)P.nn + 1)) +
           a16(4 * (size_t)P.nf) + a16(4 * P.u.size()) + a16(4 * P.uoff.size()) + a16(4 * P.ukf.size());
}

void kfdb_grow_pack(const KfdbGrowPlan& P, uint8_t* pin, int i, size_t& at, KfdbDev* fe_rec, gf_reloc_kf* rkf,
                    KfdbGrowShape& sh) {
    gf_kfdb* d = P.db;
    const gf_keyframe_db* r = P.rows;
    const int nkn = r->nkf, nkf0 = d->dev.nkf;
    auto put = [&](const void* src, size_t bytes) -> int64_t {
        const size_t o = at;
        if (bytes) memcpy(pin + o, src, bytes);
        at += a16(bytes);
        return (int64_t)o;
    };
    const size_t offs = nkn ? 4 * ((size_t)nkn + 1) : 0;
    KgHdr h{};
    const int64_t s_kp_off = put(r->kp_off, offs), s_kps = put(r->kps, sizeof(gf_keypoint) * (size_t)P.nk),
                  s_desc = put(r->desc, 32 * (size_t)P.nk), s_bow_off = put(r->bow_off, offs),
                  s_bw = put(r->bow_words, 4 * (size_t)P.nb), s_bv = put(r->bow_values, 8 * (size_t)P.nb),
                  s_fv_off = put(r->fv_off, offs), s_fn = put(r->fv_nodes, 4 * (size_t)P.nn),
                  s_fs = put(r->fv_start, nkn ? 4 * ((size_t)P.nn + 1) : 0), s_ff = put(r->fv_feats, 4 * (size_t)P.nf);
    h.u = put(P.u.data(), 4 * P.u.size());
    h.uoff = put(P.uoff.data(), 4 * P.uoff.size());
    h.ukf = put(P.ukf.data(), 4 * P.ukf.size());
    const KfdbDev& v = d->dev;
    auto W = [](const void* p) { return (int32_t*)p; };
    const int KPW = (int)(sizeof(gf_keypoint) / 4);
    // offsets skip their leading 0 and are rebased on the counts held
    h.sec[0] = {s_kp_off + 4, W(v.kp_off) + nkf0 + 1, nkn, d->nk};
    h.sec[1] = {s_kps, W(v.kps + d->nk), KPW * P.nk, 0};
    h.sec[2] = {s_desc, W(v.desc + 32 * (size_t)d->nk), 8 * P.nk, 0};
    h.sec[3] = {s_bow_off + 4, W(v.bow_off) + nkf0 + 1, nkn, d->nb};
    h.sec[4] = {s_bw, W(v.bow_words) + d->nb, P.nb, 0};
    h.sec[5] = {s_bv, W(v.bow_values + d->nb), 2 * P.nb, 0};
    h.sec[6] = {s_fv_off + 4, W(v.fv_off) + nkf0 + 1, nkn, d->nn};
    h.sec[7] = {s_fn, W(v.fv_nodes) + d->nn, P.nn, 0};
    h.sec[8] = {s_fs + 4, W(v.fv_start) + d->nn + 1, nkn ? P.nn : 0, d->nf};
    h.sec[9] = {s_ff, W(v.fv_feats) + d->nf, P.nf, 0};
    const int side1 = d->side ^ 1;
    h.rec[0] = d->d_rec;
    h.rec[1] = fe_rec;
    h.next = v;
    h.next.nkf = nkf0 + nkn;
    h.next.inv_words = h.inv_words1 = d->inv_words[side1];
    h.next.inv_off = h.inv_off1 = d->inv_off[side1];
    h.next.inv_kf = h.inv_kf1 = d->inv_kf[side1];
    h.scan = d->scan;
    h.pos = d->pos;
    h.rkf = rkf;
    h.nkf0 = nkf0;
    h.nkn = nkn;
    h.nu = (int32_t)P.u.size();
    h.ni0 = d->nb;  // one list entry per BowVector entry
    memcpy(pin + sizeof(KgHdr) * (size_t)i, &h, sizeof(h));
    sh.work = std::max(sh.work, std::max(std::max(8 * P.nk, d->nb), h.nu));
    // the host's counts follow (nw stays the device's)
    d->dev = h.next;
    d->side = side1;
    d->nk += P.nk;
    d->nb += P.nb;
    d->nn += P.nn;
    d->nf += P.nf;
}

int kfdb_grow_launch(gf_ctx* ctx, const uint8_t* stage, int ndb, const KfdbGrowShape& sh, hipStream_t s) {
    {
        GF_PROF(ctx, s, "k_kg_scan");
        GF_LAUNCH(k_kg_scan, ndb, 256, 0, s, stage);
        GF_HIP(hipGetLastError());
    }
    {
        GF_PROF(ctx, s, "k_kg_merge");
        GF_LAUNCH(k_kg_merge, dim3(std::min(KG_MAX_X, std::max(1, cdiv(sh.work, KG_CHUNK))), ndb), 256, 0, s, stage);
        GF_HIP(hipGetLastError());
    }
    GF_PROF(ctx, s, "k_kg_finish");
    GF_LAUNCH(k_kg_finish, ndb, 64, 0, s, stage);
    GF_HIP(hipGetLastError());
    return GF_OK;
}

}  // namespace gf

// ------------------------------------------------------------------ erase
// KeyFrameDatabase::erase (KeyFrameDatabase.cc:47-60) for the keyframes a map
// compaction drops (gf_frontend_compact_maps): the kept keyframes' rows close
// up in place, the inverted file is filtered and renumbered into the other
// buffer set, the record is flipped last. The host knows which keyframes go
// (the compaction has synchronised) and states old and new row offsets in the
// header; the device moves. Rows move down, so a section is walked by one
// workgroup in ascending chunks, all loads of a chunk before the barrier that
// precedes its stores (as mapcompact.hip). The renumbering is monotone, so
// every list keeps its order; a word whose list empties leaves the file.
namespace {

constexpr int KC_KF = gf::RL_NC;
constexpr int KC_U = 4, KC_CHUNK = 256 * KC_U;
enum { KC_KP = 0, KC_BOW, KC_NODE, KC_FEAT, KC_NFAM };
enum { KC_SEC_KPS = 0, KC_SEC_DESC, KC_SEC_BW, KC_SEC_BV, KC_SEC_FN, KC_SEC_FS, KC_SEC_FF, KC_SEC_INV, KC_NSEC };

struct KcHdr {
    KfdbDev cur;       // the arrays as they are
    KfdbDev next;      // the record after the call but for nw
    KfdbDev* rec[2];   // the records to flip: the database's own, the front end's stream record or null
    int32_t *scan, *pos;
    int32_t nkf0, nkf1;
    int32_t kr[KC_KF];                    // new keyframe index, -1 erased
    int32_t old_off[KC_NFAM][KC_KF + 1];  // row offsets per keyframe: keypoints, BowVector entries, nodes, features
    int32_t new_off[KC_NFAM][KC_KF + 1];  // by new keyframe index
};

// Items of W words, item j of keyframe k to new_off[kr[k]] + (j - old_off[k]); rebase: the moved values are
// fv_start entries, offsets into fv_feats that follow their keyframe's features down.
template <int W>
__device__ void kc_move(uint32_t* base, const KcHdr* H, int fam, bool rebase) {
    __shared__ int s_old[KC_KF + 1], s_new[KC_KF + 1], s_kr[KC_KF], s_sub[KC_KF];
    const int t = threadIdx.x, nk = H->nkf0;
    if (t <= KC_KF) {
        s_old[t] = H->old_off[fam][min(t, nk)];
        s_new[t] = H->new_off[fam][t];
    }
    if (t < KC_KF) {
        const int kn = t < nk ? H->kr[t] : -1;
        s_kr[t] = kn;
        s_sub[t] = rebase && kn >= 0 ? H->old_off[KC_FEAT][t] - H->new_off[KC_FEAT][kn] : 0;
    }
    __syncthreads();
    const long long total = (long long)s_old[nk] * W;
    for (long long i0 = 0; i0 < total; i0 += KC_CHUNK) {
        uint32_t v[KC_U];
        long long d[KC_U];
#pragma unroll
        for (int u = 0; u < KC_U; u++) {
            const long long i = min(i0 + t + 256 * u, total - 1);
            const int item = (int)(i / W), c = (int)(i - (long long)item * W);
            int lo = 0, hi = nk;  // the last k with s_old[k] <= item: its rows hold the item
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (s_old[mid] <= item) lo = mid; else hi = mid;
            }
            const int kn = s_kr[lo];
            v[u] = base[i] - (uint32_t)s_sub[lo];
            d[u] = i0 + t + 256 * u < total && kn >= 0 ? (long long)(s_new[kn] + item - s_old[lo]) * W + c : -1;
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < KC_U; u++)
            if (d[u] >= 0) base[d[u]] = v[u];
    }
}

// mvInvertedFile without the erased keyframes, into the other buffer set; then the record(s).
__device__ void kc_inverted(const KcHdr* H) {
    __shared__ int s_wa[4], s_wb[4], s_kr[KC_KF];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, nk = H->nkf0;
    const int nw0 = H->rec[0]->nw;
    const int32_t *W0 = H->cur.inv_words, *O0 = H->cur.inv_off, *K0 = H->cur.inv_kf;
    int32_t *W1 = const_cast<int32_t*>(H->next.inv_words), *O1 = const_cast<int32_t*>(H->next.inv_off),
            *K1 = const_cast<int32_t*>(H->next.inv_kf);
    if (t < KC_KF) s_kr[t] = t < nk ? H->kr[t] : -1;
    __syncthreads();
    int ca = 0, cb = 0;  // words and list entries so far
    for (int base = 0; base < nw0; base += 256) {
        const int i = base + t;
        int cnt = 0;
        if (i < nw0)
            for (int e = O0[i]; e < O0[i + 1]; e++) cnt += s_kr[min(max(K0[e], 0), KC_KF - 1)] >= 0;
        const int fl = cnt > 0;
        int a = fl, b = cnt;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int xa = __shfl_up(a, o, 64), xb = __shfl_up(b, o, 64);
            if (lane >= o) {
                a += xa;
                b += xb;
            }
        }
        if (lane == 63) {
            s_wa[wave] = a;
            s_wb[wave] = b;
        }
        __syncthreads();
        int ba = 0, bb = 0, ta = 0, tb = 0;
#pragma unroll
        for (int w = 0; w < 4; w++) {
            if (w < wave) {
                ba += s_wa[w];
                bb += s_wb[w];
            }
            ta += s_wa[w];
            tb += s_wb[w];
        }
        if (fl) {
            const int j = ca + ba + a - 1;
            int at = cb + bb + b - cnt;
            W1[j] = W0[i];
            O1[j] = at;
            for (int e = O0[i]; e < O0[i + 1]; e++) {
                const int kn = s_kr[min(max(K0[e], 0), KC_KF - 1)];
                if (kn >= 0) K1[at++] = kn;
            }
        }
        ca += ta;
        cb += tb;
        __syncthreads();
    }
    if (t == 0) O1[ca] = cb;
    // the record word by word, as k_kg_finish
    constexpr int RW = (int)(sizeof(KfdbDev) / 4), NW_AT = (int)(offsetof(KfdbDev, nw) / 4);
    if (t < RW) {
        int32_t* r0 = reinterpret_cast<int32_t*>(H->rec[0]);
        int32_t* r1 = reinterpret_cast<int32_t*>(H->rec[1]);
        int32_t w = reinterpret_cast<const int32_t*>(&H->next)[t];
        if (t == NW_AT) w = ca;
        r0[t] = w;
        if (r1) r1[t] = w;
    }
}

__global__ __launch_bounds__(256) void k_kc_erase(const KcHdr* H) {
    const KfdbDev& v = H->cur;
    auto W = [](const void* p) { return reinterpret_cast<uint32_t*>(const_cast<void*>(p)); };
    switch (blockIdx.x) {  // uniform
    case KC_SEC_KPS: kc_move<(int)(sizeof(gf_keypoint) / 4)>(W(v.kps), H, KC_KP, false); break;
    case KC_SEC_DESC: kc_move<8>(W(v.desc), H, KC_KP, false); break;
    case KC_SEC_BW: kc_move<1>(W(v.bow_words), H, KC_BOW, false); break;
    case KC_SEC_BV: kc_move<2>(W(v.bow_values), H, KC_BOW, false); break;
    case KC_SEC_FN: kc_move<1>(W(v.fv_nodes), H, KC_NODE, false); break;
    case KC_SEC_FS:
        kc_move<1>(W(v.fv_start), H, KC_NODE, true);
        if (threadIdx.x == 0) W(v.fv_start)[H->new_off[KC_NODE][H->nkf1]] = (uint32_t)H->new_off[KC_FEAT][H->nkf1];
        break;
    case KC_SEC_FF: kc_move<1>(W(v.fv_feats), H, KC_FEAT, false); break;
    default: kc_inverted(H); break;
    }
}

}  // namespace

namespace gf {

int kfdb_erase(gf_kfdb* d, const int32_t* kf_remap, int nkf0, KfdbDev* fe_rec, hipStream_t s) {
    GF_CHECK(d && kf_remap && d->growable, GF_ERR_ARG, "erasing keyframes needs a database that grows");
    GF_CHECK(nkf0 == d->dev.nkf && nkf0 <= KC_KF, GF_ERR_ARG, "the database and the keyframe graph differ in keyframes");
    static_assert(sizeof(gf_keypoint) % 4 == 0, "keypoints move as words");
    GF_HIP(hipSetDevice(d->device));
    GF_HIP(hipStreamSynchronize(s));
    const KfdbDev v = d->dev;
    std::vector<int32_t> off[3], fs((size_t)d->nn + 1, 0);
    const int32_t* src[3] = {v.kp_off, v.bow_off, v.fv_off};
    for (int f = 0; f < 3; f++) {
        off[f].assign(nkf0 + 1, 0);
        if (nkf0) GF_HIP(hipMemcpy(off[f].data(), src[f], 4 * off[f].size(), hipMemcpyDeviceToHost));
    }
    if (nkf0) GF_HIP(hipMemcpy(fs.data(), v.fv_start, 4 * fs.size(), hipMemcpyDeviceToHost));
    GF_CHECK(off[0][nkf0] == d->nk && off[1][nkf0] == d->nb && off[2][nkf0] == d->nn, GF_ERR_HIP,
             "database offsets on the device differ from the host's counts");
    KcHdr h{};
    int nkf1 = 0;
    for (int k = 0; k <= nkf0; k++) {
        for (int f = 0; f < 3; f++) h.old_off[f][k] = off[f][k];
        h.old_off[KC_FEAT][k] = fs[off[2][k]];
    }
    for (int k = 0; k < nkf0; k++) {
        h.kr[k] = kf_remap[k];
        if (kf_remap[k] < 0) continue;
        GF_CHECK(kf_remap[k] == nkf1, GF_ERR_ARG, "the keyframe remap is not a stable renumbering");
        for (int f = 0; f < KC_NFAM; f++)
            h.new_off[f][nkf1 + 1] = h.new_off[f][nkf1] + (h.old_off[f][k + 1] - h.old_off[f][k]);
        nkf1++;
    }
    for (int k = nkf0; k < KC_KF; k++) h.kr[k] = -1;
    for (int f = 0; f < KC_NFAM; f++)
        for (int k = nkf1 + 1; k <= KC_KF; k++) h.new_off[f][k] = h.new_off[f][nkf1];
    const int side1 = d->side ^ 1;
    h.cur = v;
    h.next = v;
    h.next.nkf = nkf1;
    h.next.inv_words = d->inv_words[side1];
    h.next.inv_off = d->inv_off[side1];
    h.next.inv_kf = d->inv_kf[side1];
    h.rec[0] = d->d_rec;
    h.rec[1] = fe_rec;
    h.scan = d->scan;
    h.pos = d->pos;
    h.nkf0 = nkf0;
    h.nkf1 = nkf1;
    int rc = grow_stage(d, sizeof(KcHdr));
    if (rc) return rc;
    GF_HIP(hipMemcpy(d->stage, &h, sizeof(h), hipMemcpyHostToDevice));
    {
        GF_PROF(d->ctx, s, "k_kc_erase");
        GF_LAUNCH(k_kc_erase, KC_NSEC, 256, 0, s, reinterpret_cast<const KcHdr*>(d->stage));
        GF_HIP(hipGetLastError());
    }
    GF_HIP(hipStreamSynchronize(s));
    // the offsets the host computed, and its counts
    int32_t* dst[3] = {(int32_t*)v.kp_off, (int32_t*)v.bow_off, (int32_t*)v.fv_off};
    for (int f = 0; f < 3; f++)
        GF_HIP(hipMemcpy(dst[f], h.new_off[f], 4 * ((size_t)nkf1 + 1), hipMemcpyHostToDevice));
    d->dev = h.next;
    d->side = side1;
    d->nk = h.new_off[KC_KP][nkf1];
    d->nb = h.new_off[KC_BOW][nkf1];
    d->nn = h.new_off[KC_NODE][nkf1];
    d->nf = h.new_off[KC_FEAT][nkf1];
    return GF_OK;
}

}  // namespace gf

extern "C" {

int gf_kfdb_create_growable(gf_ctx* ctx, const gf_keyframe_db* db, int max_kf, int max_rows, gf_kfdb** out) {
    GF_CHECK(ctx && db && out, GF_ERR_ARG, "null arg");
    const int nkf = db->nkf;
    GF_CHECK(max_kf >= 1 && max_kf <= gf::RL_NC, GF_ERR_UNSUPPORTED, "at most 64 keyframes per database");
    GF_CHECK(max_rows >= 0, GF_ERR_ARG, "negative max_rows");
    GF_CHECK(nkf >= 0, GF_ERR_ARG, "negative keyframe count");
    GF_HIP(hipSetDevice(ctx->device));
    gf_kfdb* d = new gf_kfdb();
    d->device = ctx->device;
    d->ctx = ctx;
    d->growable = true;
    d->max_kf = max_kf;
    d->max_rows = max_rows;
    const size_t R = (size_t)max_rows, K = (size_t)max_kf;
    bool ok = true;
    auto zeros = [&](size_t bytes) -> void* {  // offsets of an empty database are 0 everywhere
        void* p = nullptr;
        bytes = std::max<size_t>(bytes, 16);
        if (hipMalloc(&p, bytes) != hipSuccess) return ok = false, nullptr;
        d->allocs.push_back(p);
        if (hipMemset(p, 0, bytes) != hipSuccess) ok = false;
        return p;
    };
    gf::KfdbDev& v = d->dev;
    v.kp_off = (const int32_t*)zeros(4 * (K + 1));
    v.kps = (const gf_keypoint*)zeros(sizeof(gf_keypoint) * R);
    v.desc = (const uint8_t*)zeros(32 * R);
    v.bow_off = (const int32_t*)zeros(4 * (K + 1));
    v.bow_words = (const int32_t*)zeros(4 * R);
    v.bow_values = (const double*)zeros(8 * R);
    v.fv_off = (const int32_t*)zeros(4 * (K + 1));
    v.fv_nodes = (const int32_t*)zeros(4 * R);
    v.fv_start = (const int32_t*)zeros(4 * (R + 1));
    v.fv_feats = (const int32_t*)zeros(4 * R);
    for (int i = 0; i < 2; i++) {
        d->inv_words[i] = (int32_t*)zeros(4 * R);
        d->inv_off[i] = (int32_t*)zeros(4 * (R + 1));
        d->inv_kf[i] = (int32_t*)zeros(4 * R);
    }
    d->scan = (int32_t*)zeros(4 * (R + 1));
    d->pos = (int32_t*)zeros(4 * R);
    d->d_rec = (gf::KfdbDev*)zeros(sizeof(gf::KfdbDev));
    v.inv_words = d->inv_words[0];
    v.inv_off = d->inv_off[0];
    v.inv_kf = d->inv_kf[0];
    if (!ok || hipMemcpy(d->d_rec, &v, sizeof(v), hipMemcpyHostToDevice) != hipSuccess) {
        gf_kfdb_destroy(d);
        return gf::fail(GF_ERR_HIP, "growable keyframe database allocation");
    }
    // the keyframes given: one append into the empty database (the same path as every later one)
    const int rc = nkf ? gf_kfdb_append(d, db) : GF_OK;
    if (rc) {
        gf_kfdb_destroy(d);
        return rc;
    }
    *out = d;
    return GF_OK;
}

int gf_kfdb_append(gf_kfdb* d, const gf_keyframe_db* rows) {
    GF_CHECK(d && rows, GF_ERR_ARG, "null arg");
    GF_CHECK(d->growable, GF_ERR_ARG, "the keyframe database is fixed (gf_kfdb_create_growable makes one that grows)");
    GF_CHECK(!d->bound, GF_ERR_ARG,
             "the database is attached to a front end: its keyframes arrive with gf_frontend_update_maps_kfdb");
    gf::KfdbGrowPlan P;
    int rc = gf::kfdb_grow_validate(d, rows, P);
    if (rc) return rc;
    if (rows->nkf == 0) return GF_OK;
    GF_HIP(hipSetDevice(d->device));
    const size_t bytes = gf::kfdb_grow_hdr_bytes(1) + gf::kfdb_grow_bytes(P);
    if ((rc = grow_stage(d, bytes))) return rc;
    std::vector<uint8_t> img(bytes);
    size_t at = gf::kfdb_grow_hdr_bytes(1);
    gf::KfdbGrowShape sh;
    hipStream_t s = d->ctx->stream;
    GF_HIP(hipStreamSynchronize(s));  // the staging of an append in flight
    gf::kfdb_grow_pack(P, img.data(), 0, at, nullptr, nullptr, sh);
    GF_HIP(hipMemcpy(d->stage, img.data(), at, hipMemcpyHostToDevice));
    if ((rc = gf::kfdb_grow_launch(d->ctx, d->stage, 1, sh, s))) return rc;
    GF_HIP(hipStreamSynchronize(s));
    return GF_OK;
}

int gf_kfdb_read(gf_kfdb* d, int32_t counts[6], gf_keyframe_db* out, int32_t* inv_words, int32_t* inv_off,
                 int32_t* inv_kf, const int32_t caps[6]) {
    GF_CHECK(d && counts, GF_ERR_ARG, "null arg");
    GF_HIP(hipSetDevice(d->device));
    GF_HIP(hipDeviceSynchronize());
    gf::KfdbDev v = d->dev;
    if (d->growable) GF_HIP(hipMemcpy(&v, d->d_rec, sizeof(v), hipMemcpyDeviceToHost));
    const int nkf = v.nkf;
    GF_CHECK(nkf >= 0 && nkf <= gf::RL_NC && v.nw >= 0, GF_ERR_HIP, "database sizes out of range on the device");
    std::vector<int32_t> ko(nkf + 1, 0), bo(nkf + 1, 0), fo(nkf + 1, 0);
    auto down = [](void* dst, const void* src, size_t bytes) -> hipError_t {
        return bytes ? hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) : hipSuccess;
    };
    if (nkf) {
        GF_HIP(down(ko.data(), v.kp_off, 4 * ko.size()));
        GF_HIP(down(bo.data(), v.bow_off, 4 * bo.size()));
        GF_HIP(down(fo.data(), v.fv_off, 4 * fo.size()));
    }
    const int nk = ko[nkf], nb = bo[nkf], nn = fo[nkf];
    GF_CHECK(nk >= 0 && nb >= 0 && nn >= 0, GF_ERR_HIP, "database offsets out of range on the device");
    std::vector<int32_t> fs((size_t)nn + 1, 0);
    if (nkf) GF_HIP(down(fs.data(), v.fv_start, 4 * fs.size()));
    const int nf = fs[nn];
    GF_CHECK(nf >= 0 && v.nw <= nb, GF_ERR_HIP, "database offsets out of range on the device");
    counts[0] = nkf;
    counts[1] = nk;
    counts[2] = nb;
    counts[3] = nn;
    counts[4] = nf;
    counts[5] = v.nw;
    if (!out) return GF_OK;
    GF_CHECK(caps && inv_words && inv_off && inv_kf, GF_ERR_ARG, "null output array");
    GF_CHECK(nkf <= caps[0] && nk <= caps[1] && nb <= caps[2] && nn <= caps[3] && nf <= caps[4] && v.nw <= caps[5],
             GF_ERR_CAP, "database larger than the output capacity");
    GF_CHECK(out->kp_off && out->kps && out->desc && out->bow_off && out->bow_words && out->bow_values && out->fv_off &&
                 out->fv_nodes && out->fv_start && out->fv_feats,
             GF_ERR_ARG, "null output array");
    out->nkf = nkf;
    memcpy((void*)out->kp_off, ko.data(), 4 * ko.size());
    memcpy((void*)out->bow_off, bo.data(), 4 * bo.size());
    memcpy((void*)out->fv_off, fo.data(), 4 * fo.size());
    memcpy((void*)out->fv_start, fs.data(), 4 * fs.size());
    GF_HIP(down((void*)out->kps, v.kps, sizeof(gf_keypoint) * (size_t)nk));
    GF_HIP(down((void*)out->desc, v.desc, 32 * (size_t)nk));
    GF_HIP(down((void*)out->bow_words, v.bow_words, 4 * (size_t)nb));
    GF_HIP(down((void*)out->bow_values, v.bow_values, 8 * (size_t)nb));
    GF_HIP(down((void*)out->fv_nodes, v.fv_nodes, 4 * (size_t)nn));
    GF_HIP(down((void*)out->fv_feats, v.fv_feats, 4 * (size_t)nf));
    GF_HIP(down(inv_words, v.inv_words, 4 * (size_t)v.nw));
    GF_HIP(down(inv_off, v.inv_off, 4 * ((size_t)v.nw + 1)));
    GF_HIP(down(inv_kf, v.inv_kf, 4 * (size_t)nb));
    return GF_OK;
}

}  // extern "C"
