// Loop detection: a growable device keyframe database (gf_loopdb) and
// KeyFrameDatabase::DetectLoopCandidates (KeyFrameDatabase.cc:75-196) over it,
// L1Scoring::score (ScoringObject.cpp:23-68) on the host and on the device.
//
// The reference walks an inverted file: query words ascending, each word's
// keyframe list in add order. A keyframe enters lKFsSharingWords at its first
// encounter, so the list's order is the order of the key (smallest common
// word, add sequence number), and mnLoopWords is the number of common words.
// Both come from intersecting each listed BowVector with the query's, one wave
// per keyframe, with no inverted file on the device:
//   k_ld_common  common-word count, key and the global maximum (pass 1)
//   k_ld_score   the L1 score of the keyframes above minCommonWords (pass 2)
//   k_ld_select  covisibility sums, the 0.75 filter, order, de-duplication
//                (pass 3, one workgroup)
#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

#include "common.h"

namespace {

constexpr int LD_MAXW = 4096;  // the bow transform's cap on a BowVector
constexpr int LD_T = 256;      // threads of a pass-1 / pass-2 workgroup (4 waves)
constexpr int LD_SEL_T = 1024; // threads of the pass-3 workgroup
constexpr int LD_SORT_LDS = 2048;  // pass 3 orders lists up to this length in LDS (24 KB)
constexpr unsigned long long LD_NOKEY = ~0ull;

struct LdMeta {
    int32_t max_common;  // maxCommonWords
    int32_t min_common;  // minCommonWords (written by pass 3)
    int32_t ncand;
    int32_t pad;
};

struct LdDb {  // the database's device arrays
    const int32_t* words;
    const double* values;
    const int32_t* off;  // per slot: first entry
    const int32_t* len;  // per slot: entries
    const int32_t* seq;  // per slot: add sequence number, -1 = not in the file
    int nslots;
};

using gfd::ldg;

// Stage the query's words in LDS, padded with INT_MAX up to the power of two
// the search reads; returns the search's first step (wave-uniform).
__device__ __forceinline__ int stage_query(int32_t* qw, const int32_t* q, int nq) {
    int step0 = 1;
    while (2 * step0 - 1 < nq && step0 < LD_MAXW / 2) step0 *= 2;
    const int lim = 2 * step0;  // <= LD_MAXW; the search ends at lo <= lim - 1
    for (int i = (int)threadIdx.x; i < lim && i < LD_MAXW; i += (int)blockDim.x) {
        const int ii = i < nq ? i : 0;
        const int32_t w = nq > 0 ? ldg(q + ii) : 0;
        qw[i] = i < nq ? w : INT_MAX;
    }
    __syncthreads();
    return step0;
}

// Number of query words < w (branch-free lower bound over the padded copy);
// every index read is < 2 * step0.
__device__ __forceinline__ int lower_bound_lds(const int32_t* qw, int step0, int32_t w) {
    int lo = 0;
    for (int st = step0; st > 0; st >>= 1) lo += qw[lo + st - 1] < w ? st : 0;
    return lo;
}

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}

// L1Scoring::score(query, keyframe) by one wave: lanes take the keyframe's
// words 64 at a time, the common words' terms are added in ascending word
// order (lane order within a batch, batches in order), every lane the same sum.
__device__ __forceinline__ double wave_score(const int32_t* qw, int step0, int nq, const double* qv,
                                             const int32_t* kw, const double* kv, int len, int lane) {
    double s = 0.0;
    if (nq > 0) {
        for (int base = 0; base < len; base += 256) {
            int32_t w[4];
            double wi[4], vi[4];
            int lo[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {  // the batch's loads together, none behind a branch
                const int i = base + u * 64 + lane;
                const int ii = i < len ? i : len - 1;
                const int32_t x = ldg(kw + ii);
                wi[u] = ldg(kv + ii);
                w[u] = i < len ? x : -1;
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                lo[u] = lower_bound_lds(qw, step0, w[u]);
                if (qw[lo[u]] != w[u]) lo[u] = -1;  // the padding is INT_MAX, never a word
            }
#pragma unroll
            for (int u = 0; u < 4; u++) vi[u] = ldg(qv + (lo[u] >= 0 ? lo[u] : 0));
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const double term = fabs(vi[u] - wi[u]) - fabs(vi[u]) - fabs(wi[u]);
                unsigned long long m = __ballot(lo[u] >= 0);
                const int tlo = __double2loint(term), thi = __double2hiint(term);
                while (m) {  // wave-uniform: the lane index is scalar, so the term is read with v_readlane
                    const int l = __builtin_ctzll(m);
                    s += __hiloint2double(__builtin_amdgcn_readlane(thi, l), __builtin_amdgcn_readlane(tlo, l));
                    m &= m - 1;
                }
            }
        }
    }
    return -s / 2.0;
}

// Pass 1. One wave per slot (grid-stride): mnLoopWords, the order key and the
// maximum. Slots that are not in the file or are connected to the query get 0.
__global__ __launch_bounds__(LD_T) void k_ld_common(LdDb db, int query, const uint8_t* excl, int32_t* words_out,
                                                    float* score_out, unsigned long long* key,
                                                    unsigned long long* first_key, uint8_t* survive, LdMeta* meta) {
    __shared__ int32_t qw[LD_MAXW];
    const int nq = ldg(db.len + query);
    const int step0 = stage_query(qw, db.words + ldg(db.off + query), nq);
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int nwaves = (int)gridDim.x * (LD_T / 64);
    for (int slot = (int)blockIdx.x * (LD_T / 64) + wave; slot < db.nslots; slot += nwaves) {
        const int seq = ldg(db.seq + slot);
        const bool listed = seq >= 0 && ldg(excl + slot) == 0;
        const int len = listed ? ldg(db.len + slot) : 0;
        const int32_t* kw = db.words + ldg(db.off + slot);
        int cnt = 0, minw = INT_MAX;
        for (int base = 0; base < len; base += 256) {
            int32_t w[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {  // the batch's loads together, none behind a branch
                const int i = base + u * 64 + lane;
                const int32_t x = ldg(kw + (i < len ? i : len - 1));
                w[u] = i < len ? x : -1;
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int lo = lower_bound_lds(qw, step0, w[u]);
                const bool found = qw[lo] == w[u];
                cnt += found ? 1 : 0;
                minw = found ? min(minw, w[u]) : minw;
            }
        }
        cnt = gfd::warp_sum(cnt);
        minw = wave_min(minw);
        if (lane == 0) {
            words_out[slot] = cnt;
            score_out[slot] = 0.f;
            survive[slot] = 0;
            key[slot] = cnt > 0 ? ((unsigned long long)(unsigned)minw << 32) | (unsigned)seq : LD_NOKEY;
            first_key[slot] = LD_NOKEY;
            if (cnt > 0) atomicMax(&meta->max_common, cnt);
        }
    }
}

// Pass 2. minCommonWords on the device; one wave per slot above it: the score
// in double, its float cast (mLoopScore) and the si >= minScore test.
__global__ __launch_bounds__(LD_T) void k_ld_score(LdDb db, int query, float min_score, const int32_t* words_out,
                                                   float* score_out, uint8_t* survive, const LdMeta* meta) {
    __shared__ int32_t qw[LD_MAXW];
    const int min_common = (int)((float)ldg(&meta->max_common) * 0.8f);
    const int nq = ldg(db.len + query);
    const int qoff = ldg(db.off + query);
    const int step0 = stage_query(qw, db.words + qoff, nq);
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int nwaves = (int)gridDim.x * (LD_T / 64);
    for (int slot = (int)blockIdx.x * (LD_T / 64) + wave; slot < db.nslots; slot += nwaves) {
        if (ldg(words_out + slot) <= min_common) continue;  // wave-uniform
        const int off = ldg(db.off + slot);
        const float si = (float)wave_score(qw, step0, nq, db.values + qoff, db.words + off, db.values + off,
                                           ldg(db.len + slot), lane);
        if (lane == 0) {
            score_out[slot] = si;
            survive[slot] = si >= min_score ? 1 : 0;
        }
    }
}

// gf_loopdb_scores: the same score for a list of slots, listed or not.
__global__ __launch_bounds__(LD_T) void k_ld_scores(LdDb db, int query, const int32_t* slots, int n, float* out) {
    __shared__ int32_t qw[LD_MAXW];
    const int nq = ldg(db.len + query);
    const int qoff = ldg(db.off + query);
    const int step0 = stage_query(qw, db.words + qoff, nq);
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int nwaves = (int)gridDim.x * (LD_T / 64);
    for (int k = (int)blockIdx.x * (LD_T / 64) + wave; k < n; k += nwaves) {
        const int slot = ldg(slots + k);
        const int off = ldg(db.off + slot);
        const float si = (float)wave_score(qw, step0, nq, db.values + qoff, db.words + off, db.values + off,
                                           ldg(db.len + slot), lane);
        if (lane == 0) out[k] = si;
    }
}

// Bitonic sort of P (a power of two) keys with their payloads by one workgroup,
// ascending: log2(P) (log2(P) + 1) / 2 rounds of P / 2 compare-exchanges.
__device__ void sort_by_key(unsigned long long* k, int32_t* v, int P, int tid) {
    for (int size = 2; size <= P; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < P / 2; t += LD_SEL_T) {
                const int i = 2 * t - (t & (stride - 1)), j = i + stride;
                const unsigned long long a = k[i], b = k[j];
                if ((a > b) == ((i & size) == 0)) {
                    k[i] = b;
                    k[j] = a;
                    const int32_t x = v[i];
                    v[i] = v[j];
                    v[j] = x;
                }
            }
            __syncthreads();
        }
}

// Pass 3, one workgroup. Per surviving slot the float sum over its first ten
// ordered covisibles in their order and pBestKF; bestAccScore from minScore;
// the > 0.75f * best filter; the kept entries in key order, each pBestKF once
// (its first occurrence = the kept entry of smallest key naming it), ordered
// by a bitonic sort of the (distinct) keys.
__global__ __launch_bounds__(LD_SEL_T) void k_ld_select(int nslots, float min_score, const int32_t* cov_off,
                                                        const int32_t* cov, const int32_t* words_out,
                                                        const float* score_out, const uint8_t* survive,
                                                        const unsigned long long* key, unsigned long long* first_key,
                                                        float* acc, int32_t* best, unsigned long long* list_key,
                                                        int32_t* list_best, int32_t* cands, LdMeta* meta) {
    __shared__ float red[LD_SEL_T / 64];
    __shared__ unsigned long long sort_k[LD_SORT_LDS];
    __shared__ int32_t sort_v[LD_SORT_LDS];
    __shared__ float best_acc_s;
    __shared__ int count_s;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int min_common = (int)((float)ldg(&meta->max_common) * 0.8f);
    if (tid == 0) count_s = 0;
    float mx = min_score;
    for (int i = tid; i < nslots; i += LD_SEL_T) {
        if (!survive[i]) continue;
        const float si = score_out[i];
        float a = si, bs = si;
        int bk = i;
        const int c0 = cov_off[i], c1 = min(cov_off[i + 1], c0 + 10);
        for (int c = c0; c < c1; c++) {
            const int k2 = cov[c];
            if (words_out[k2] > min_common) {
                const float s2 = score_out[k2];
                a += s2;
                if (s2 > bs) {
                    bk = k2;
                    bs = s2;
                }
            }
        }
        acc[i] = a;
        best[i] = bk;
        mx = fmaxf(mx, a);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    if (lane == 0) red[wave] = mx;
    __syncthreads();
    if (tid == 0) {
        float m = red[0];
        for (int w = 1; w < LD_SEL_T / 64; w++) m = fmaxf(m, red[w]);
        best_acc_s = m;
    }
    __syncthreads();
    const float retain = 0.75f * best_acc_s;
    for (int i = tid; i < nslots; i += LD_SEL_T)
        if (survive[i] && acc[i] > retain) atomicMin(&first_key[best[i]], key[i]);
    __syncthreads();
    for (int i = tid; i < nslots; i += LD_SEL_T) {
        if (!(survive[i] && acc[i] > retain)) continue;
        const int b = best[i];
        if (__hip_atomic_load(&first_key[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == key[i]) {
            const int p = atomicAdd(&count_s, 1);
            list_key[p] = key[i];
            list_best[p] = b;
        }
    }
    __syncthreads();
    const int m = count_s;
    int P = 1;  // the list padded to a power of two with keys above every real one
    while (P < m) P <<= 1;
    if (P <= LD_SORT_LDS) {  // the usual case: a short list, sorted in LDS
        for (int e = tid; e < P; e += LD_SEL_T) {
            sort_k[e] = e < m ? list_key[e] : LD_NOKEY;
            sort_v[e] = e < m ? list_best[e] : -1;
        }
        __syncthreads();
        sort_by_key(sort_k, sort_v, P, tid);
        for (int e = tid; e < m; e += LD_SEL_T) cands[e] = sort_v[e];
    } else {  // up to every slot of the database: in place (the lists hold 2 * nslots entries)
        for (int e = m + tid; e < P; e += LD_SEL_T) list_key[e] = LD_NOKEY;
        __syncthreads();
        sort_by_key(list_key, list_best, P, tid);
        for (int e = tid; e < m; e += LD_SEL_T) cands[e] = list_best[e];
    }
    if (tid == 0) {
        meta->min_common = min_common;
        meta->ncand = m;
    }
}

__global__ void k_ld_set(int32_t* p, int idx, int32_t v) { p[idx] = v; }

__global__ void k_ld_fill(int32_t* p, int n, int32_t v) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i < n) p[i] = v;
}

// gf_loopdb_insert_dev: frame f's strided BowVector into the slot's storage
__global__ void k_ld_copy(const int32_t* src_w, const double* src_v, const int32_t* src_n, int cap, int32_t* dst_w,
                          double* dst_v, int32_t* len, int slot) {
    const int n = min(max(src_n[0], 0), cap);
    for (int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); i < n; i += (int)(gridDim.x * blockDim.x)) {
        dst_w[i] = src_w[i];
        dst_v[i] = src_v[i];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) len[slot] = n;
}

struct Buf {  // grow-by-doubling device array; the old storage is retired, not freed under a running kernel
    void* p = nullptr;
    size_t cap = 0;  // bytes
};

}  // namespace

struct gf_loopdb {
    gf_ctx* ctx = nullptr;
    int device = 0;
    int nslots = 0, nlisted = 0;
    int32_t next_seq = 0;
    long long nwords = 0;  // entries of the CSR storage in use
    std::vector<int32_t> h_off, h_seq;
    hipEvent_t order = nullptr;  // orders gf_loopdb_insert_dev's stream against the context's
    Buf words, values, off, len, seq;
    // per-query scratch, by slot capacity
    Buf excl, words_out, score_out, survive, key, first_key, acc, best, list_key, list_best, cands, meta, tmp_i, tmp_f;
    Buf cov_off, cov;
    std::vector<void*> retired;
};

namespace {

int reserve(gf_loopdb* d, Buf& b, size_t need, size_t keep, hipStream_t s) {
    if (need <= b.cap) return GF_OK;
    size_t cap = std::max<size_t>(b.cap * 2, 4096);
    while (cap < need) cap *= 2;
    void* p = nullptr;
    GF_HIP(hipMalloc(&p, cap));
    if (keep) {
        hipError_t e = hipMemcpyAsync(p, b.p, keep, hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) {
            (void)hipFree(p);
            GF_HIP(e);
        }
    }
    if (b.p) d->retired.push_back(b.p);
    b.p = p;
    b.cap = cap;
    return GF_OK;
}

void free_retired(gf_loopdb* d) {  // after a stream synchronisation only
    for (void* p : d->retired) (void)hipFree(p);
    d->retired.clear();
}

LdDb view(const gf_loopdb* d) {
    return LdDb{(const int32_t*)d->words.p, (const double*)d->values.p, (const int32_t*)d->off.p,
                (const int32_t*)d->len.p, (const int32_t*)d->seq.p, d->nslots};
}

// a new slot with room for `n` entries; its off is set, its seq -1
int new_slot(gf_loopdb* d, int n, int len_known, hipStream_t s, int* slot) {
    GF_CHECK(d->nwords + n <= (long long)INT_MAX, GF_ERR_CAP, "BowVector storage exceeds 2^31 entries");
    const int k = d->nslots;
    int rc;
    if ((rc = reserve(d, d->words, 4 * (size_t)(d->nwords + n), 4 * (size_t)d->nwords, s)) ||
        (rc = reserve(d, d->values, 8 * (size_t)(d->nwords + n), 8 * (size_t)d->nwords, s)) ||
        (rc = reserve(d, d->off, 4 * (size_t)(k + 1), 4 * (size_t)k, s)) ||
        (rc = reserve(d, d->len, 4 * (size_t)(k + 1), 4 * (size_t)k, s)) ||
        (rc = reserve(d, d->seq, 4 * (size_t)(k + 1), 4 * (size_t)k, s)))
        return rc;
    k_ld_set<<<1, 1, 0, s>>>((int32_t*)d->off.p, k, (int32_t)d->nwords);
    k_ld_set<<<1, 1, 0, s>>>((int32_t*)d->seq.p, k, -1);
    if (len_known >= 0) k_ld_set<<<1, 1, 0, s>>>((int32_t*)d->len.p, k, len_known);
    GF_HIP(hipGetLastError());
    d->h_off.push_back((int32_t)d->nwords);
    d->h_seq.push_back(-1);
    d->nwords += n;
    d->nslots = k + 1;
    *slot = k;
    return GF_OK;
}

int grid_for(const gf_ctx* ctx, int items) {  // workgroups of 4 waves, one item per wave, grid-stride
    return std::max(1, std::min((items + LD_T / 64 - 1) / (LD_T / 64), ctx->num_cus * 8));
}

}  // namespace

extern "C" {

int gf_loopdb_create(gf_ctx* ctx, gf_loopdb** out) {
    GF_CHECK(ctx && out, GF_ERR_ARG, "null arg");
    gf_loopdb* d = new gf_loopdb();
    d->ctx = ctx;
    d->device = ctx->device;
    GF_HIP(hipSetDevice(ctx->device));
    if (hipEventCreateWithFlags(&d->order, hipEventDisableTiming) != hipSuccess) {
        delete d;
        return gf::fail(GF_ERR_HIP, "hipEventCreateWithFlags");
    }
    *out = d;
    return GF_OK;
}

int gf_loopdb_destroy(gf_loopdb* d) {
    if (!d) return GF_OK;
    (void)hipSetDevice(d->device);
    (void)hipDeviceSynchronize();
    free_retired(d);
    if (d->order) (void)hipEventDestroy(d->order);
    for (Buf* b : {&d->words, &d->values, &d->off, &d->len, &d->seq, &d->excl, &d->words_out, &d->score_out,
                   &d->survive, &d->key, &d->first_key, &d->acc, &d->best, &d->list_key, &d->list_best, &d->cands,
                   &d->meta, &d->tmp_i, &d->tmp_f, &d->cov_off, &d->cov})
        if (b->p) (void)hipFree(b->p);
    delete d;
    return GF_OK;
}

int gf_loopdb_size(gf_loopdb* d, int* nslots, int* nlisted) {
    GF_CHECK(d, GF_ERR_ARG, "null arg");
    if (nslots) *nslots = d->nslots;
    if (nlisted) *nlisted = d->nlisted;
    return GF_OK;
}

int gf_loopdb_clear(gf_loopdb* d) {
    GF_CHECK(d, GF_ERR_ARG, "null arg");
    GF_HIP(hipSetDevice(d->device));
    if (d->nslots) {
        k_ld_fill<<<(d->nslots + 255) / 256, 256, 0, d->ctx->stream>>>((int32_t*)d->seq.p, d->nslots, -1);
        GF_HIP(hipGetLastError());
    }
    std::fill(d->h_seq.begin(), d->h_seq.end(), -1);
    d->nlisted = 0;
    d->next_seq = 0;
    return GF_OK;
}

int gf_loopdb_insert(gf_loopdb* d, const int32_t* words, const double* values, int n, int* slot) {
    GF_CHECK(d && slot && (n == 0 || (words && values)), GF_ERR_ARG, "null arg");
    GF_CHECK(n >= 0 && n <= LD_MAXW, GF_ERR_ARG, "a BowVector holds 0 to 4096 words");
    for (int i = 0; i < n; i++)
        GF_CHECK(words[i] >= 0 && words[i] < INT_MAX && (i == 0 || words[i] > words[i - 1]), GF_ERR_ARG,
                 "BowVector words must ascend");
    GF_HIP(hipSetDevice(d->device));
    hipStream_t s = d->ctx->stream;
    int k = -1;
    int rc = new_slot(d, n, n, s, &k);
    if (rc) return rc;
    if (n) {
        GF_HIP(hipMemcpyAsync((int32_t*)d->words.p + d->h_off[k], words, 4 * (size_t)n, hipMemcpyHostToDevice, s));
        GF_HIP(hipMemcpyAsync((double*)d->values.p + d->h_off[k], values, 8 * (size_t)n, hipMemcpyHostToDevice, s));
    }
    GF_HIP(hipStreamSynchronize(s));  // the caller's arrays are free again
    free_retired(d);
    *slot = k;
    return GF_OK;
}

int gf_loopdb_insert_dev(gf_loopdb* d, const int32_t* d_words, const double* d_values, const int32_t* d_nwords, int cap,
                         int frame, void* stream, int* slot) {
    GF_CHECK(d && slot && d_words && d_values && d_nwords, GF_ERR_ARG, "null arg");
    GF_CHECK(cap >= 1 && cap <= LD_MAXW && frame >= 0, GF_ERR_ARG, "cap is 1 to 4096, frame >= 0");
    GF_HIP(hipSetDevice(d->device));
    hipStream_t s = (hipStream_t)stream, cs = d->ctx->stream;
    // everything the context's stream holds for this database (add / erase
    // kernels, queries) comes before the growth copies and the new slot ...
    if (s != cs) {
        GF_HIP(hipEventRecord(d->order, cs));
        GF_HIP(hipStreamWaitEvent(s, d->order, 0));
    }
    int k = -1;
    int rc = new_slot(d, cap, -1, s, &k);
    if (rc) return rc;
    k_ld_copy<<<(cap + 255) / 256, 256, 0, s>>>(d_words + (size_t)frame * cap, d_values + (size_t)frame * cap,
                                                 d_nwords + frame, cap, (int32_t*)d->words.p + d->h_off[k],
                                                 (double*)d->values.p + d->h_off[k], (int32_t*)d->len.p, k);
    GF_HIP(hipGetLastError());
    // ... and the context's later work on it after them, so that a synchronised
    // context stream also covers the copies out of the retired blocks
    if (s != cs) {
        GF_HIP(hipEventRecord(d->order, s));
        GF_HIP(hipStreamWaitEvent(cs, d->order, 0));
    }
    *slot = k;
    return GF_OK;
}

int gf_loopdb_add(gf_loopdb* d, int slot) {
    GF_CHECK(d, GF_ERR_ARG, "null arg");
    GF_CHECK(slot >= 0 && slot < d->nslots, GF_ERR_ARG, "no such slot");
    GF_CHECK(d->h_seq[slot] < 0, GF_ERR_ARG, "the slot is already in the file");
    GF_CHECK(d->next_seq < INT_MAX, GF_ERR_CAP, "add sequence numbers exhausted");
    GF_HIP(hipSetDevice(d->device));
    k_ld_set<<<1, 1, 0, d->ctx->stream>>>((int32_t*)d->seq.p, slot, d->next_seq);
    GF_HIP(hipGetLastError());
    d->h_seq[slot] = d->next_seq++;
    d->nlisted++;
    return GF_OK;
}

int gf_loopdb_erase(gf_loopdb* d, int slot) {
    GF_CHECK(d, GF_ERR_ARG, "null arg");
    GF_CHECK(slot >= 0 && slot < d->nslots, GF_ERR_ARG, "no such slot");
    if (d->h_seq[slot] < 0) return GF_OK;  // erase of a keyframe that is in no list changes nothing
    GF_HIP(hipSetDevice(d->device));
    k_ld_set<<<1, 1, 0, d->ctx->stream>>>((int32_t*)d->seq.p, slot, -1);
    GF_HIP(hipGetLastError());
    d->h_seq[slot] = -1;
    d->nlisted--;
    return GF_OK;
}

int gf_bow_score(int scoring, const int32_t* w1, const double* v1, int n1, const int32_t* w2, const double* v2, int n2,
                 double* score) {
    GF_CHECK(score && n1 >= 0 && n2 >= 0 && (n1 == 0 || (w1 && v1)) && (n2 == 0 || (w2 && v2)), GF_ERR_ARG,
             "null arg");
    GF_CHECK(scoring == 0, GF_ERR_UNSUPPORTED, "only L1_NORM scoring (the ORB vocabulary's) is implemented");
    double s = 0;
    int i = 0, j = 0;
    while (i < n1 && j < n2) {
        if (w1[i] == w2[j]) {
            const double vi = v1[i], wi = v2[j];
            s += std::fabs(vi - wi) - std::fabs(vi) - std::fabs(wi);
            i++;
            j++;
        } else if (w1[i] < w2[j]) {
            i = (int)(std::lower_bound(w1 + i, w1 + n1, w2[j]) - w1);
        } else {
            j = (int)(std::lower_bound(w2 + j, w2 + n2, w1[i]) - w2);
        }
    }
    *score = -s / 2.0;
    return GF_OK;
}

int gf_loopdb_scores(gf_loopdb* d, int query_slot, const int32_t* slots, int n, float* out) {
    GF_CHECK(d && n >= 0 && (n == 0 || (slots && out)), GF_ERR_ARG, "null arg");
    GF_CHECK(query_slot >= 0 && query_slot < d->nslots, GF_ERR_ARG, "no such query slot");
    for (int i = 0; i < n; i++) GF_CHECK(slots[i] >= 0 && slots[i] < d->nslots, GF_ERR_ARG, "no such slot");
    if (n == 0) return GF_OK;
    GF_HIP(hipSetDevice(d->device));
    hipStream_t s = d->ctx->stream;
    int rc;
    if ((rc = reserve(d, d->tmp_i, 4 * (size_t)n, 0, s)) || (rc = reserve(d, d->tmp_f, 4 * (size_t)n, 0, s))) return rc;
    GF_HIP(hipMemcpyAsync(d->tmp_i.p, slots, 4 * (size_t)n, hipMemcpyHostToDevice, s));
    {
        GF_PROF(d->ctx, s, "k_ld_scores");
        GF_LAUNCH(k_ld_scores, grid_for(d->ctx, n), LD_T, 0, s, view(d), query_slot, (const int32_t*)d->tmp_i.p, n,
                  (float*)d->tmp_f.p);
    }
    GF_HIP(hipGetLastError());
    GF_HIP(hipMemcpyAsync(out, d->tmp_f.p, 4 * (size_t)n, hipMemcpyDeviceToHost, s));
    GF_HIP(hipStreamSynchronize(s));
    free_retired(d);
    return GF_OK;
}

int gf_detect_loop_candidates(gf_loopdb* d, int query_slot, const int32_t* connected, int nconn, const int32_t* cov_off,
                              const int32_t* cov, float min_score, int32_t* words_out, float* score_out,
                              int* min_common, int32_t* cands, int* ncand) {
    GF_CHECK(d && cov_off && words_out && score_out && min_common && cands && ncand && nconn >= 0 &&
                 (nconn == 0 || connected),
             GF_ERR_ARG, "null arg");
    const int ns = d->nslots;
    GF_CHECK(query_slot >= 0 && query_slot < ns, GF_ERR_ARG, "no such query slot");
    std::vector<uint8_t> excl((size_t)ns, 0);
    for (int i = 0; i < nconn; i++) {
        GF_CHECK(connected[i] >= 0 && connected[i] < ns, GF_ERR_ARG, "no such connected slot");
        excl[connected[i]] = 1;
    }
    GF_CHECK(cov_off[0] == 0, GF_ERR_ARG, "covisible offsets start at 0");
    for (int k = 0; k < ns; k++) GF_CHECK(cov_off[k + 1] >= cov_off[k], GF_ERR_ARG, "covisible offsets must ascend");
    const int ncov = cov_off[ns];
    GF_CHECK(ncov == 0 || cov, GF_ERR_ARG, "null covisibles");
    for (int i = 0; i < ncov; i++) GF_CHECK(cov[i] >= 0 && cov[i] < ns, GF_ERR_ARG, "bad covisible keyframe");
    GF_HIP(hipSetDevice(d->device));
    hipStream_t s = d->ctx->stream;
    const size_t n4 = 4 * (size_t)ns, n8 = 8 * (size_t)ns;
    int rc;
    if ((rc = reserve(d, d->excl, ns, 0, s)) || (rc = reserve(d, d->survive, ns, 0, s)) ||
        (rc = reserve(d, d->words_out, n4, 0, s)) || (rc = reserve(d, d->score_out, n4, 0, s)) ||
        (rc = reserve(d, d->acc, n4, 0, s)) || (rc = reserve(d, d->best, n4, 0, s)) ||
        (rc = reserve(d, d->list_best, 2 * n4, 0, s)) || (rc = reserve(d, d->cands, n4, 0, s)) ||
        (rc = reserve(d, d->key, n8, 0, s)) || (rc = reserve(d, d->first_key, n8, 0, s)) ||
        (rc = reserve(d, d->list_key, 2 * n8, 0, s)) || (rc = reserve(d, d->meta, sizeof(LdMeta), 0, s)) ||
        (rc = reserve(d, d->cov_off, n4 + 4, 0, s)) || (rc = reserve(d, d->cov, 4 * (size_t)std::max(ncov, 1), 0, s)))
        return rc;
    GF_HIP(hipMemcpyAsync(d->excl.p, excl.data(), ns, hipMemcpyHostToDevice, s));
    GF_HIP(hipMemcpyAsync(d->cov_off.p, cov_off, n4 + 4, hipMemcpyHostToDevice, s));
    if (ncov) GF_HIP(hipMemcpyAsync(d->cov.p, cov, 4 * (size_t)ncov, hipMemcpyHostToDevice, s));
    GF_HIP(hipMemsetAsync(d->meta.p, 0, sizeof(LdMeta), s));
    const LdDb v = view(d);
    const int grid = grid_for(d->ctx, ns);
    {
        GF_PROF(d->ctx, s, "k_ld_common");
        GF_LAUNCH(k_ld_common, grid, LD_T, 0, s, v, query_slot, (const uint8_t*)d->excl.p, (int32_t*)d->words_out.p,
                  (float*)d->score_out.p, (unsigned long long*)d->key.p, (unsigned long long*)d->first_key.p,
                  (uint8_t*)d->survive.p, (LdMeta*)d->meta.p);
    }
    {
        GF_PROF(d->ctx, s, "k_ld_score");
        GF_LAUNCH(k_ld_score, grid, LD_T, 0, s, v, query_slot, min_score, (const int32_t*)d->words_out.p,
                  (float*)d->score_out.p, (uint8_t*)d->survive.p, (const LdMeta*)d->meta.p);
    }
    {
        GF_PROF(d->ctx, s, "k_ld_select");
        GF_LAUNCH(k_ld_select, 1, LD_SEL_T, 0, s, ns, min_score, (const int32_t*)d->cov_off.p,
                  (const int32_t*)d->cov.p, (const int32_t*)d->words_out.p, (const float*)d->score_out.p,
                  (const uint8_t*)d->survive.p, (const unsigned long long*)d->key.p,
                  (unsigned long long*)d->first_key.p, (float*)d->acc.p, (int32_t*)d->best.p,
                  (unsigned long long*)d->list_key.p, (int32_t*)d->list_best.p, (int32_t*)d->cands.p,
                  (LdMeta*)d->meta.p);
    }
    GF_HIP(hipGetLastError());
    LdMeta m;
    GF_HIP(hipMemcpyAsync(&m, d->meta.p, sizeof(LdMeta), hipMemcpyDeviceToHost, s));
    GF_HIP(hipMemcpyAsync(words_out, d->words_out.p, n4, hipMemcpyDeviceToHost, s));
    GF_HIP(hipMemcpyAsync(score_out, d->score_out.p, n4, hipMemcpyDeviceToHost, s));
    GF_HIP(hipMemcpyAsync(cands, d->cands.p, n4, hipMemcpyDeviceToHost, s));
    GF_HIP(hipStreamSynchronize(s));
    free_retired(d);
    GF_CHECK(m.ncand >= 0 && m.ncand <= ns, GF_ERR_HIP, "candidate count out of range");
    *min_common = m.min_common;
    *ncand = m.ncand;
    return GF_OK;
}

}  // extern "C"
