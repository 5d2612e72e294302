// Track-loss paths of the tracking step (reloc.hip): TrackPreviousFrame and
// Relocalisation, the per-stream state they read and the scratch they use.
// frontend.hip fills a TrackLossArgs once per front end and launches the two
// stages inside its step.
#pragma once
#include <vector>

#include "common.h"
#include "match_common.h"

namespace gf {

constexpr int RL_NC = 64;     // relocalisation candidate slots per stream (the keyframe-graph cap)
constexpr int RL_LCAP = 300;  // PnP hypotheses one iterate() call can need (mRansacMaxIts <= 300)
constexpr int RL_WORK = 12;   // doubles per correspondence of the PnP refine buffer (pnp_core.h kWork)

// Frame grid scratch per stream: cell_start [NCELLS + 1], items / scratch /
// claim [cap] each.
__host__ __device__ inline size_t grid_ints(int cap) { return (size_t)NCELLS + 1 + 3 * (size_t)cap; }

// Device view of a keyframe database (gf_kfdb) plus its inverted file.
struct KfdbDev {
    int nkf;
    const int32_t* kp_off;
    const gf_keypoint* kps;
    const uint8_t* desc;
    const int32_t* bow_off;
    const int32_t* bow_words;
    const double* bow_values;
    const int32_t* fv_off;
    const int32_t* fv_nodes;
    const int32_t* fv_start;
    const int32_t* fv_feats;
    // mvInvertedFile: inv_words ascending, keyframes of word w at inv_kf[inv_off[w] .. inv_off[w + 1])
    int nw;
    const int32_t* inv_words;
    const int32_t* inv_off;
    const int32_t* inv_kf;
};

struct TrackLossArgs {
    int B, cap, M, budget, nlevels;
    FrameConst fc;
    float inv_sigma2[16], level_sigma2[16];
    // current frame
    const gf_keypoint* kps;
    const uint8_t* desc;
    const int32_t* nkp;
    int32_t* kp2mp;
    int32_t* score;
    uint8_t* outl;
    float* Tcw;
    // last frame
    const gf_keypoint* last_kps;
    const uint8_t* last_desc;
    const int32_t* last_nkp;
    const int32_t* last_kp2mp;
    const float* last_pos;
    const float* Tcw_last;
    // the stream maps (map indices of kp2mp)
    const gf_map_point* gmap;
    const uint8_t* gdesc;
    // state
    int32_t* track;  // [B][GF_TR_N]
    int32_t* stats;  // [GF_FE_NSTAT][B]
    gf_rng* rng;
    const int32_t* kf_count;  // [B] keyframes of the stream's graph (-1: no graph; assumed > 5)
    const int32_t* gnmp;      // [B] the stream maps' sizes
    // gates of the TrackLocalMap stages (written for every stream)
    int32_t* nkp_tl;    // [B] nkp when TrackLocalMap runs, else 0
    int32_t* nkp_fi;    // [B] nkp when its FRAME_INFO_MATRIX pass runs, else 0
    int32_t* gate_tl;   // [B]
    int32_t* gate_fi;   // [B]
    float* th_m2;       // [B] 5 within 2 frames of a relocalisation, else 1
    int32_t* nmp_step;  // [B] null with keyframe graphs; else gnmp when TrackLocalMap runs, else 0
    // scratch per stream
    int32_t* grid;        // [B][grid_ints(cap)]
    int32_t* rec;         // [B][cap] rotation-histogram records
    gf_pose_edge* edges;  // [B][cap]
    int32_t* edge_kp;     // [B][cap]
    uint8_t* eoutl;       // [B][cap]
    double* pwork;        // [B][3 cap]
    int32_t* pint;        // [B][4] nedges, inliers, iterations
    // relocalisation (kfdb null: no stream has a database)
    const KfdbDev* kfdb;        // [B] (nkf 0: none)
    int rl_on;                  // the step computes candidates (a vocabulary and some database set)
    const gf_covis_map* covis;  // [B] the streams' keyframe graphs (device)
    gf_reloc_kf* rkf;           // [B][RL_NC]
    const int32_t* rl_gate;     // [B] 1: the stream relocalises this step
    const int32_t* words;       // [B][cap] the frame's BowVector
    const double* values;
    const int32_t* nwords;
    const int32_t* fv_nodes;  // [B][cap] its FeatureVector
    const int32_t* fv_start;  // [B][cap + 1]
    const int32_t* fv_feats;  // [B][cap]
    const int32_t* nfv;
    int ncs;                  // candidate slots per stream in pairs / bow_out (max keyframes over the streams)
    BowPairDev* pairs;        // [B][ncs]
    int32_t* bow_out;         // [B][ncs][cap]
    int32_t* bow_nm;          // [B][ncs]
    int32_t* cands;           // [B][RL_NC]
    int32_t* ncand;           // [B]
    gf_pnp_state* pst;        // [B][RL_NC]
    uint8_t* pbest;           // [B][RL_NC][cap]
    float* p3d;               // [B][cap][3]
    float* p2d;               // [B][cap][2]
    float* psig;              // [B][cap]
    int32_t* pidx;            // [B][cap]
    uint8_t* pinl;            // [B][cap]
    int32_t* pdraws;          // [B][RL_LCAP][8]
    double* prt;              // [B][RL_LCAP][12]
    int32_t* pcnt;            // [B][RL_LCAP]
    double* pwk;              // [B][cap][RL_WORK]
    float* ptcw;              // [B][16]
    int32_t* pflags;          // [B][2] flags, inliers of the last iterate()
};

// The device arrays of a keyframe database (gf_kfdb_create).
const KfdbDev& kfdb_dev(const gf_kfdb* db);
// The checks of gf_kfdb_create on a database's arrays -> its keypoints, BowVector
// entries, FeatureVector nodes and features (GF_ERR_ARG otherwise).
int kfdb_validate(const gf_keyframe_db* db, int& nk, int& nb, int& nn, int& nf);

// ---- a database that grows (kfdbgrow.hip)
// One validated append: the rows' sizes and the delta inverted file of the new
// keyframes (their words merged: u ascending, word u's new keyframes at
// ukf[uoff[u] .. uoff[u + 1]) in index order).
struct KfdbGrowPlan {
    gf_kfdb* db = nullptr;
    const gf_keyframe_db* rows = nullptr;
    int nk = 0, nb = 0, nn = 0, nf = 0;
    std::vector<int32_t> u, uoff, ukf;
};
// Largest per-database counts of a call, for the grids.
struct KfdbGrowShape {
    int work = 0;
};
bool kfdb_growable(const gf_kfdb* db);
int kfdb_max_kf(const gf_kfdb* db);
bool kfdb_bound(const gf_kfdb* db);
// Binds a growable database to its one stream (GF_ERR_ARG when it is bound) and
// releases it; the record as the device holds it now (synchronous).
int kfdb_bind(gf_kfdb* db, KfdbDev* rec);
void kfdb_unbind(gf_kfdb* db);
// gf_kfdb_create's checks on `rows` (offsets from 0) and the database's
// capacities: GF_ERR_ARG / GF_ERR_CAP, the database untouched.
int kfdb_grow_validate(gf_kfdb* db, const gf_keyframe_db* rows, KfdbGrowPlan& P);
size_t kfdb_grow_hdr_bytes(int ndb);
size_t kfdb_grow_bytes(const KfdbGrowPlan& P);
// Packs database `i` of a call into the staging image `pin` (its header at
// slot i, its sections from `at`, which advances) and advances the database's
// host counts. fe_rec: the front end's record of the stream (device) and rkf
// its keyframes' query state, or null.
void kfdb_grow_pack(const KfdbGrowPlan& P, uint8_t* pin, int i, size_t& at, KfdbDev* fe_rec, gf_reloc_kf* rkf,
                    KfdbGrowShape& sh);
int kfdb_grow_launch(gf_ctx* ctx, const uint8_t* stage, int ndb, const KfdbGrowShape& sh, hipStream_t s);
// KeyFrameDatabase::clear for gf_frontend_start_streams: the host's counts of a
// growable database, read, and set (to zero before the start's rows are
// validated against the empty database; to what they were when the call is
// refused). The device's record (kfdb_record) is emptied by the start's first
// kernel, in stream order before the append that follows.
struct KfdbHostCounts {
    int nkf = 0, nk = 0, nb = 0, nn = 0, nf = 0;
};
KfdbHostCounts kfdb_host_counts(const gf_kfdb* db);
void kfdb_set_host_counts(gf_kfdb* db, const KfdbHostCounts& c);
KfdbDev* kfdb_record(gf_kfdb* db);
// KeyFrameDatabase::erase for a map compaction: the keyframes whose kf_remap entry is -1 leave the growable
// database (rows closed up in place, inverted file filtered into the other buffer set, records flipped).
// Synchronises s before and after.
int kfdb_erase(gf_kfdb* db, const int32_t* kf_remap, int nkf0, KfdbDev* fe_rec, hipStream_t s);

// DetectRelocalisationCandidates for the streams that relocalise and their
// SearchByBoW pairs (k_match_bow then runs over A.pairs).
int reloc_candidates(gf_ctx* ctx, const TrackLossArgs& A, hipStream_t s);
// After TrackWithMotionModel: its failure test, TrackPreviousFrame for the
// streams that need it, Relocalisation for the LOST ones; sets GF_TR_OK.
int track_loss(gf_ctx* ctx, const TrackLossArgs& A, hipStream_t s);

}  // namespace gf

struct gf_kfdb {
    int device = 0;  // the context's device (the context may go first)
    gf::KfdbDev dev{};
    std::vector<void*> allocs;
    // gf_kfdb_create_growable: arrays at the capacities, two inverted files
    // written in turn, the record in device memory (d_rec: what the kernels
    // read and flip; dev follows it on the host but for nw, which only the
    // device knows), and the host's counts
    bool growable = false, bound = false;
    gf_ctx* ctx = nullptr;
    int max_kf = 0, max_rows = 0;
    int nk = 0, nb = 0, nn = 0, nf = 0;  // keypoints, BowVector entries, FeatureVector nodes and features
    int side = 0;                        // the inverted file in use
    int32_t *inv_words[2] = {}, *inv_off[2] = {}, *inv_kf[2] = {};
    int32_t *scan = nullptr, *pos = nullptr;  // [max_rows + 1], [max_rows] of the merge
    gf::KfdbDev* d_rec = nullptr;
    uint8_t* stage = nullptr;  // gf_kfdb_append's staging
    size_t stage_bytes = 0;
};
