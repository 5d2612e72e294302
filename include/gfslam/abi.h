/*
 * gfslam C-ABI — the drop-in boundary of the MI355X GF-ORB-SLAM front end.
 *
 * Every entry point is extern "C", takes plain pointers and sizes, returns an
 * int status (GF_OK = 0, negative = error; no exceptions cross the ABI) and
 * replaces one reference C++ operator (file:line cited per function, paths
 * relative to the reference tree Aidenryan/GF_ORB_SLAM). Two families:
 *
 *   host family   (gf_orb_extract, gf_match_project, ...): host buffers in and
 *                 out, synchronous; what a cgo/ctypes/C++ caller binds.
 *   device family (*_dev): device pointers + a hipStream_t passed as void*,
 *                 asynchronous, batched over independent frames; what the
 *                 throughput path (bench.py) and in-process pipelines use.
 *
 * Error behaviour mirrors the reference: empty inputs give empty outputs
 * (ORBextractor.cc:772 returns on an empty image, matchers return 0 matches).
 */
#ifndef GFSLAM_ABI_H
#define GFSLAM_ABI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    GF_OK = 0,
    GF_ERR_ARG = -1,          /* bad argument (null pointer, size mismatch)     */
    GF_ERR_HIP = -2,          /* HIP runtime error (message in gf_last_error)  */
    GF_ERR_CAP = -3,          /* output capacity too small (n_out holds need)  */
    GF_ERR_UNSUPPORTED = -4,  /* option the build does not implement           */
    GF_ERR_NODEV = -5         /* no HIP device                                 */
};

/* cv::KeyPoint memory layout (28 B): pt.x, pt.y, size, angle, response,
 * octave, class_id. */
typedef struct gf_keypoint {
    float x, y, size, angle, response;
    int32_t octave, class_id;
} gf_keypoint;

typedef struct gf_ctx gf_ctx;
typedef struct gf_extractor gf_extractor;

/* ---------------------------------------------------------------- runtime */
int gf_version(void);
const char* gf_last_error(void);
int gf_device_count(int* n);
/* One context per host thread: owns one HIP stream on `hip_device`. */
int gf_ctx_create(int hip_device, gf_ctx** out);
int gf_ctx_destroy(gf_ctx* ctx);
int gf_ctx_stream(gf_ctx* ctx, void** stream);
int gf_ctx_sync(gf_ctx* ctx);
/* Per-kernel timing with HIP events recorded on each launch's own stream
 * (what bench.py reports the roofline from). gf_prof_report returns, for
 * entry idx, the kernel name, summed device time and launch count. */
int gf_prof_enable(gf_ctx* ctx, int on);
int gf_prof_reset(gf_ctx* ctx);
int gf_prof_report(gf_ctx* ctx, int idx, char* name, int name_cap, double* total_ms, int* launches);

/* ------------------------------------------------------- ORB extraction (E1-E8)
 * Replaces ORB_SLAM::ORBextractor (include/ORBextractor.h:57-70,
 * src/ORBextractor.cc:464-998): ctor(nfeatures, scaleFactor, nlevels,
 * scoreType, fastTh) and operator()(image, mask=empty, keypoints, descriptors).
 * The geometry (width x height) is fixed at creation: the pyramid, cell grids
 * and per-level quotas are planned once. score_type: FAST_SCORE (1) or HARRIS_SCORE (0);
 * any other value returns GF_ERR_ARG. max_batch bounds nframes of the
 * batched device call. */
int gf_extractor_create(gf_ctx* ctx, int nfeatures, float scale_factor, int nlevels,
                        int score_type, int fast_th, int width, int height, int max_batch,
                        gf_extractor** out);
int gf_extractor_destroy(gf_extractor* ex);
/* GetLevels()/GetScaleFactor() (ORBextractor.h:66-70) + the per-level
 * feature quotas mnFeaturesPerLevel (ORBextractor.cc:483-494). */
int gf_extractor_info(gf_extractor* ex, int* nlevels, float* scale_factor,
                      int* features_per_level /* [nlevels] or NULL */);
/* Max keypoints one frame can return (sum of level quotas). */
int gf_extractor_capacity(gf_extractor* ex, int* cap);

/* Host family: img is width x height u8 with row stride `stride`; writes up to
 * `cap` keypoints (28 B each) and descriptors (32 B rows). An empty image
 * (width/height 0) returns n_out = 0. */
int gf_orb_extract(gf_extractor* ex, const uint8_t* img, int stride, gf_keypoint* kps,
                   uint8_t* desc, int cap, int* n_out);

/* Device family: nframes images at d_imgs + f*frame_stride (row stride
 * `stride`), outputs at d_kps[f*cap + i], d_desc[(f*cap + i)*32] and
 * d_counts[f]; cap must be >= gf_extractor_capacity. Asynchronous on stream. */
int gf_orb_extract_batch_dev(gf_extractor* ex, int nframes, const uint8_t* d_imgs,
                             size_t frame_stride, int stride, gf_keypoint* d_kps,
                             uint8_t* d_desc, int32_t* d_counts, int cap, void* stream);

/* Pointer-table form of gf_orb_extract_batch_dev: level 0 of frame f is the
 * width x height image at d_img_ptrs[f] (a device array of device pointers,
 * row stride `stride`), so frames can come from anywhere in HBM (a sequence
 * ring, a staging buffer) without a gather copy. */
int gf_orb_extract_ptrs_dev(gf_extractor* ex, int nframes, const uint8_t* const* d_img_ptrs, int stride,
                            gf_keypoint* d_kps, uint8_t* d_desc, int32_t* d_counts, int cap, void* stream);

/* Debug/parity hook: copies one intermediate plane of frame f of the last
 * batch to host. which: 0 = pyramid level (unblurred, ComputePyramid
 * ORBextractor.cc:922-998), 1 = blurred level interior (GaussianBlur :842).
 * out must hold w*h bytes of that level; (w,h) returned. */
int gf_extractor_debug_level(gf_extractor* ex, int frame, int level, int which, uint8_t* out,
                             int* w, int* h);

/* ------------------------------------------------------ matching (E8, M1-M5, M7)
 * Frame view (include/Frame.h:44-150): keypoints mvKeysUn (== mvKeys when
 * k1 == 0, Frame.cc:391-395), descriptors, undistorted image bounds
 * mnMinX..mnMaxY (Frame.cc:470-476), intrinsics, scale pyramid. The 64x48
 * keypoint grid (Frame.cc:100-131) is built on the device per call. */
typedef struct gf_frame_info {
    int32_t min_x, max_x, min_y, max_y;
    float fx, fy, cx, cy;
    int32_t nlevels;
    float scale_factor; /* mvScaleFactors[l] = scale_factor^l (float products) */
} gf_frame_info;

/* MapPoint state used by the tracker (include/MapPoint.h): world position,
 * mean viewing direction, scale-invariance distances mfMinDistance /
 * mfMaxDistance (MapPoint.cc:326-336). Descriptors travel separately (32 B). */
typedef struct gf_map_point {
    float pos[3];
    float normal[3];
    float min_dist, max_dist;
} gf_map_point;

/* Projection state Frame::isInFrustum writes into a MapPoint
 * (Frame.cc:216-222): mTrackProjX/Y, mTrackViewCos, mnTrackScaleLevel,
 * mbTrackInView (in_view = mbTrackInView && !isBad()). */
typedef struct gf_mp_view {
    float u, v, view_cos;
    int32_t level;
    int32_t in_view;
} gf_mp_view;

/* Frame::isInFrustum(pMP, viewingCosLimit), Frame.cc:166-227, for m map
 * points at pose Tcw (row-major 4x4 float). */
int gf_frustum(gf_ctx* ctx, const gf_frame_info* fi, const float* Tcw, const gf_map_point* mps, int m,
               float view_cos_limit, gf_mp_view* views, int* n_in_view);

/* ORBmatcher::SearchByProjection(Frame& F, const vector<MapPoint*>&, th),
 * ORBmatcher.cc:384-465 (M2; with RadiusByViewingCos :696-702,
 * Frame::GetFeaturesInArea Frame.cc:300-365). Map points are processed in
 * list order; a keypoint already claimed (kp2mp[i] >= 0 on entry, or by an
 * earlier map point) is skipped, exactly as F.mvpMapPoints[idx] != NULL.
 * kp2mp/score are in/out (mvpMapPoints / mvpMatchScore, index of the map
 * point in `views`); nmatches = new matches. */
int gf_match_project(gf_ctx* ctx, const gf_frame_info* fi, const gf_keypoint* kps, const uint8_t* desc, int n,
                     const gf_mp_view* views, const uint8_t* mp_desc, int m, float th, float nnratio,
                     int32_t* kp2mp, int32_t* score, int* nmatches);

/* ORBmatcher::SearchByProjection(Frame& Cur, const Frame& Last, th),
 * ORBmatcher.cc:2081-2202, with the rotation-consistency histogram
 * (ComputeThreeMaxima :2338-2379) when check_ori != 0 (M3). Last-frame
 * keypoint i carries map point last_kp2mp[i] (-1: none) at world position
 * last_pos[3i..3i+2] and outlier flag last_outlier[i]. Matches write
 * kp2mp[j] = last_kp2mp[i] and score[j]; rejected rotations reset score to
 * 999 (:2183-2186). */
int gf_match_lastframe(gf_ctx* ctx, const gf_frame_info* fi, const gf_keypoint* kps, const uint8_t* desc, int n,
                       const float* Tcw, const gf_keypoint* last_kps, const uint8_t* last_desc,
                       const int32_t* last_kp2mp, const uint8_t* last_outlier, const float* last_pos, int n_last,
                       float th, int check_ori, int32_t* kp2mp, int32_t* score, int* nmatches);

/* Device family of the three above, batched over nframes independent frames.
 * Per-frame arrays are strided by their capacity (kp_cap keypoints, mp_cap /
 * last_cap queries); counts live on the device (d_n, d_m, d_n_last). Limits:
 * kp_cap <= 4096, mp_cap/last_cap <= 8192. gf_match_lastframe_dev needs
 * d_scratch of nframes*last_cap int32. */
int gf_frustum_dev(gf_ctx* ctx, const gf_frame_info* fi, int nframes, const float* d_Tcw, const gf_map_point* d_mps,
                   const int32_t* d_m, int mp_cap, float view_cos_limit, gf_mp_view* d_views, int32_t* d_nview,
                   void* stream);
int gf_match_project_dev(gf_ctx* ctx, const gf_frame_info* fi, int nframes, const gf_keypoint* d_kps,
                         const uint8_t* d_desc, const int32_t* d_n, int kp_cap, const gf_mp_view* d_views,
                         const uint8_t* d_mp_desc, const int32_t* d_m, int mp_cap, float th, float nnratio,
                         int32_t* d_kp2mp, int32_t* d_score, int32_t* d_nmatches, void* stream);
int gf_match_lastframe_dev(gf_ctx* ctx, const gf_frame_info* fi, int nframes, const gf_keypoint* d_kps,
                           const uint8_t* d_desc, const int32_t* d_n, int kp_cap, const float* d_Tcw,
                           const gf_keypoint* d_last_kps, const uint8_t* d_last_desc, const int32_t* d_last_kp2mp,
                           const uint8_t* d_last_outlier, const float* d_last_pos, const int32_t* d_n_last,
                           int last_cap, float th, int check_ori, int32_t* d_kp2mp, int32_t* d_score,
                           int32_t* d_nmatches, int32_t* d_scratch, void* stream);

/* List forms (device family). Frame::isInFrustum for the map points
 * d_list[f][0 .. d_nlist[f]) only (the visibility pass of
 * SearchAdditionalMatchesInFrame over mLeftMapPoints, Tracking.cc:3105-3126);
 * views of other points are left as they are. And
 * ORBmatcher::SearchByProjection_Budget(F, vpMapPoints, th, time)
 * (ORBmatcher.cc:276-379) = SearchByProjection over the map points of the
 * list in list order (th != 1 scales the window; claims and the ratio test as
 * M2). Lists are strided by mp_cap. */
int gf_frustum_list_dev(gf_ctx* ctx, const gf_frame_info* fi, int nframes, const float* d_Tcw,
                        const gf_map_point* d_mps, int mp_cap, const int32_t* d_list, const int32_t* d_nlist,
                        float view_cos_limit, gf_mp_view* d_views, int32_t* d_nview, void* stream);
int gf_match_project_list_dev(gf_ctx* ctx, const gf_frame_info* fi, int nframes, const gf_keypoint* d_kps,
                              const uint8_t* d_desc, const int32_t* d_n, int kp_cap, const gf_mp_view* d_views,
                              const uint8_t* d_mp_desc, int mp_cap, const int32_t* d_list, const int32_t* d_nlist,
                              float th, float nnratio, int32_t* d_kp2mp, int32_t* d_score, int32_t* d_nmatches,
                              void* stream);

/* ORBmatcher::DescriptorDistance (ORBmatcher.cc:2384-2400) over n pairs of
 * 32-byte rows: dist[i] = popcount(a[i] ^ b[i]). */
int gf_descriptor_distance(gf_ctx* ctx, const uint8_t* a, const uint8_t* b, int n, int32_t* dist);

/* ------------------------------------------------- good-feature selection (G1-G7)
 * f64 throughout, as the reference's Armadillo matrices. */

/* glibc rand() state (TYPE_3 additive feedback, 31 words): the reference draws
 * its lazier-greedy samples with std::rand() % n (Observability.cc:1348,
 * :2895). Callers keep one state per sequence across frames. */
typedef struct gf_rng {
    int32_t state[31];
    int32_t f, r;
} gf_rng;
/* std::srand(seed) */
int gf_rng_seed(gf_rng* rng, uint32_t seed);
/* n successive std::rand() values (host; for checking the device port). */
int gf_rng_next(gf_rng* rng, int32_t* out, int n);

/* Observability camera (PinHoleCamera, include/Util.hpp:136-178) and the
 * visibility margins mBoundX/YInFrame, mBoundDepth (Observability.h:727-728)
 * with Frame::mnMinX..mnMaxY. */
typedef struct gf_obs_camera {
    double fu, fv, cx, cy;
    int32_t nrows, ncols;
    int32_t min_x, max_x, min_y, max_y;
    int32_t bound_x, bound_y;
    float bound_depth;
} gf_obs_camera;

/* One predicted segment of the constant-velocity PWLS motion model
 * (KineStruct, Util.hpp:170-177): state Xv = [twc(3) q_wc(4) v(3) w(3)], the
 * quaternion/angular-rate blocks of F for the full segment and one of 13
 * sub-segments, and the predicted Tcw (float, row-major). */
typedef struct gf_kine {
    double dt, dt_inseg;
    double Xv[13];
    double F_Q[16], F_Omg[12], F_Q_inSeg[16], F_Omg_inSeg[12]; /* row-major */
    float Tcw[16];
} gf_kine;

/* Observability::updatePWLSVec (Observability.h:222-259): Xv from the last
 * frame pose Tcw_prev and the current Twc (float row-major), times in s. */
int gf_obs_update(double t_prev, const float* Tcw_prev, double t_cur, const float* Twc_cur, double* Xv);
/* Observability::predictPWLSVec(dt, nseg) (Observability.h:261-295). */
int gf_obs_predict(const double* Xv, double dt, int nseg, gf_kine* out);

/* Measurement Jacobian + information block per landmark
 * (compute_H_subblock_simplied Observability.h:460-515, reWeightInfoMat
 * :517-596, batchInfoMat_Map / batchInfoMat_Frame Observability.cc:386-644).
 * For each of n landmarks at world position pos[3i..]: H (2x7 row-major,
 * n x 14) and info = H_rw^T H_rw (7x7 row-major, n x 49) at state Xv, where
 * H_rw = H / sigma, sigma^2 = sigma2[i] (frame path: level sigma^2 of the
 * matched keypoint octave) or 1 when sigma2 == NULL (map path). uv = the
 * projected pixel (u_proj, v_proj). valid[i] = 0 when check_viz rejects the
 * landmark (ObsScore = -1). */
int gf_obs_build_info(gf_ctx* ctx, const gf_obs_camera* cam, const double* Xv, const float* pos,
                      const float* sigma2, int n, int check_viz, double* H, double* info, float* uv,
                      uint8_t* valid);

/* Util.hpp:714-731 logDet: 2 log prod diag chol(M), LU log|det| fallback;
 * n 7x7 row-major matrices. */
int gf_logdet(gf_ctx* ctx, const double* M, int n, double* out);

/* Observability::runActiveMapMatching with FRAME_INFO_MATRIX
 * (Observability.cc:1249-1524): lazier-greedy active matching of
 * num_to_match map points into frame F using SearchByProjection_OnePoint
 * (ORBmatcher.h:71-145). Pool = map points with views[i].in_view and
 * updated[i] (updateAtFrameId == frame id), in list order; info/H are their
 * map information blocks and Jacobians (gf_obs_build_info map path), uv their
 * projections. base = mCurrentInfoMat (7x7). level_sigma2 = Frame
 * mvLevelSigma2. Writes claims into kp2mp/score (in/out), the left-over pool
 * (mLeftMapPoints) into left[0..nleft), advances rng; nmatched = matches. */
int gf_obs_active_match(gf_ctx* ctx, const gf_frame_info* fi, const gf_keypoint* kps, const uint8_t* desc, int n,
                        const gf_mp_view* views, const uint8_t* mp_desc, const uint8_t* updated,
                        const double* info, const double* H, const float* uv, int m, const double* base,
                        const float* level_sigma2, int num_to_match, float th, float nnratio, gf_rng* rng,
                        int32_t* kp2mp, int32_t* score, int32_t* left, int* nleft, int* nmatched);

/* Max-volume subset selection over a pool of 7x7 information blocks
 * (Observability.cc): mode 1 = maxVolSelection_BaselineGreedy (:3031-3139),
 * 2 = maxVolSelection_LazierGreedy (:2815-3029), 3 =
 * maxVolAutomatic_LazierGreedy (:3141-3155, deletion when 2k > n).
 * score[i] < 0 excludes block i (obs_score). sample_scale as
 * setSelction_Number computes it (:823). out_idx receives pool indices in
 * selection order (deletion: pool order). rng used by modes 2-3. */
int gf_maxvol_select(gf_ctx* ctx, const double* info, const double* score, int n, int k, double sample_scale,
                     int mode, gf_rng* rng, int32_t* out_idx, int* nout);

/* The greedy stage alone, over a prepared pool (lmkSelectPool,
 * Observability.cc:1046-1160): n blocks info [n][49] with their ObsScore
 * values, k = num_good_inlier; out_idx = pool positions selected (greedy_mtd
 * 3 splits large pools into threadNeeded chunks, run in chunk order on rng).
 * What setSelction_Number runs after MAP_INFO_MATRIX has left points updated
 * this frame (e.g. by FRAME_INFO_MATRIX) with their own blocks and scores. */
int gf_select_pool(gf_ctx* ctx, const double* info, const double* score, int n, int k, int greedy_mtd,
                   int max_threads, gf_rng* rng, int32_t* out_idx, int* nout);

/* Observability::setSelction_Number(num_good_inlier, greedy_mtd, time,
 * mapPoints, mpVec) (Observability.cc:1021-1247; test/test_GoodMap.cpp drives
 * it): MAP_INFO_MATRIX with the visibility check (mKineIdx = 1: Xv is the
 * predicted kinematic[1] state) over the n map points at pos, the visible ones
 * form the pool in list order, then greedy_mtd 1 = BaselineGreedy, 2 =
 * LazierGreedy, 3 = maxVolAutomatic_LazierGreedy with the multi-thread split
 * (threadNeeded = min(round(pool / 1000), max_threads) when pool >= 2000 and
 * pool - 1.2 k > 10; chunks of ceil(pool / T) selecting ceil(k / T * 1.2)
 * each, then one pass over the merged selections). sample_scale 6. The chunks
 * draw from `rng` in chunk order (the reference's threads share std::rand()
 * in race order). out_idx = map indices in selection order (deletion
 * variant: pool order); at most 4096 visible points per greedy call. */
int gf_select_map_points(gf_ctx* ctx, const gf_obs_camera* cam, const double* Xv, const float* pos, int n, int k,
                         int greedy_mtd, int max_threads, gf_rng* rng, int32_t* out_idx, int* nout);

/* Device family of the GF rows, batched over frames (per-frame arrays strided
 * by cap / mp_cap; d_Xv is [F][13], d_base [F][49], d_rng [F]). Pool limit
 * for active matching and max-volume selection: 4096 landmarks.
 * gf_obs_accumulate_dev: d_out[f] = diag*I + sum of d_info rows with d_flag
 * set (mCurrentInfoMat accumulation, Tracking.cc:3161 and :3195-3219).
 * gf_obs_active_match_dev: d_nldet (optional, [F]) = logDet evaluations the
 * reference makes (one per heap push, Observability.cc:1373); frames whose
 * d_m or d_num_to_match is 0 exit before any LDS use. */
int gf_obs_build_info_dev(gf_ctx* ctx, const gf_obs_camera* cam, int nframes, const double* d_Xv, const float* d_pos,
                          const float* d_sigma2, const int32_t* d_n, int cap, int check_viz, double* d_H,
                          double* d_info, float* d_uv, uint8_t* d_valid, void* stream);
int gf_obs_accumulate_dev(gf_ctx* ctx, int nframes, const double* d_info, const uint8_t* d_flag, const int32_t* d_n,
                          int cap, double diag, double* d_out, void* stream);
int gf_obs_active_match_dev(gf_ctx* ctx, const gf_frame_info* fi, int nframes, const gf_keypoint* d_kps,
                            const uint8_t* d_desc, const int32_t* d_n, int kp_cap, const gf_mp_view* d_views,
                            const uint8_t* d_mp_desc, const uint8_t* d_updated, const double* d_info,
                            const double* d_H, const int32_t* d_m, int mp_cap, const double* d_base,
                            const float* level_sigma2, const int32_t* d_num_to_match, float th, float nnratio,
                            gf_rng* d_rng, int32_t* d_kp2mp, int32_t* d_score, int32_t* d_left, int32_t* d_nleft,
                            int32_t* d_nmatched, int32_t* d_nldet, void* stream);
int gf_maxvol_select_dev(gf_ctx* ctx, int npools, const double* d_info, const double* d_score, const int32_t* d_n,
                         int cap, int k, double sample_scale, int mode, gf_rng* d_rng, int32_t* d_out,
                         int32_t* d_nout, void* stream);

/* G1 on the device: Xv[f] = updatePWLSVec(t_prev[f], Tcw_prev[f], t_cur[f],
 * getTwc(Tcw_cur[f])) (Tracking.cc:3168-3169, :797-799, Frame.cc:152-163).
 * Segment 0 of predictPWLSVec keeps this Xv (the in-frame FRAME/MAP builds);
 * d_Xv_next (optional) = kinematic[1].Xv = propagate_PWLS(Xv, float(dt)), the
 * state the next-frame MAP build uses (Tracking.cc:1768, mKineIdx = 1). */
int gf_obs_update_dev(gf_ctx* ctx, int nframes, const double* d_t_prev, const float* d_Tcw_prev,
                      const double* d_t_cur, const float* d_Tcw_cur, double* d_Xv, double* d_Xv_next,
                      void* stream);

/* Map-resident observability state, map-indexed per frame (stride
 * map_stride): H [14], ObsMat [49], u/v_proj [2], updateAtFrameId (int32).
 * gf_obs_frame_info_dev = batchInfoMat_Frame (Observability.cc:386-554):
 *   matched non-outlier keypoints write their map point's H/ObsMat/uv with
 *   the keypoint level sigma^2; updateAtFrameId untouched.
 * gf_obs_map_info_dev = batchInfoMat_Map (Observability.cc:556-644): points
 *   with updateAtFrameId == frame_id are skipped, and with check_viz == 0 so
 *   are points whose view is not in_view (d_views may be NULL only with
 *   check_viz); a valid point is written and stamped frame_id. d_updated
 *   (optional) = (updateAtFrameId == frame_id) for every point afterwards.
 * gf_obs_accumulate_matched_dev: mCurrentInfoMat = diag*I + sum, in keypoint
 *   order, of the ObsMat of matched points stamped frame_id (Tracking.cc:3184,
 *   3195-3213). */
int gf_obs_frame_info_dev(gf_ctx* ctx, const gf_obs_camera* cam, int nframes, const double* d_Xv,
                          const gf_keypoint* d_kps, const int32_t* d_nkps, int kp_stride, const int32_t* d_kp2mp,
                          const uint8_t* d_outlier, const float* d_map_pos, const int32_t* d_nmp, int map_stride,
                          const float* level_sigma2, int nlevels, double* d_H, double* d_info, float* d_uv,
                          void* stream);
int gf_obs_map_info_dev(gf_ctx* ctx, const gf_obs_camera* cam, int nframes, const double* d_Xv, const float* d_map_pos,
                        const int32_t* d_nmp, int map_stride, int check_viz, const gf_mp_view* d_views,
                        int32_t* d_upd_id, int frame_id, double* d_H, double* d_info, float* d_uv,
                        uint8_t* d_updated, void* stream);
int gf_obs_accumulate_matched_dev(gf_ctx* ctx, int nframes, const int32_t* d_kp2mp, const int32_t* d_nkps,
                                  int kp_stride, const double* d_info, const int32_t* d_upd_id, const int32_t* d_nmp,
                                  int map_stride, int frame_id, double diag, double* d_out, void* stream);

/* ------------------------------------------------ pose optimisation (P1-P4)
 * Optimizer::PoseOptimization(Frame*) (src/Optimizer.cc:279-413) on g2o's
 * Levenberg-Marquardt (core/optimization_algorithm_levenberg.cpp:61-189),
 * EdgeSE3ProjectXYZ with a fixed map point (types_six_dof_expmap.cpp:384-428),
 * Huber delta^2 = 5.991 (robust_kernel_impl.cpp:78-88) and the dense LDLT
 * solver (linear_solver_dense.h:65-113). One edge per matched keypoint, in
 * keypoint order; f64 internally, float pose in and out (Converter.cc:38-72).
 * Outlier flags follow the reference: 4 rounds of {10,10,7,5} iterations with
 * chi2 thresholds {9.210,7.378,5.991,5.991}; outliers keep their edge with
 * information 1e-10. ninliers = n - nBad of the last round. */
typedef struct gf_pose_edge {
    float X[3];       /* MapPoint::GetWorldPos() */
    float z[2];       /* mvKeysUn[i].pt */
    float inv_sigma2; /* mvInvLevelSigma2[octave] */
} gf_pose_edge;

/* Host family: one problem of n edges. iterations (may be NULL) = LM
 * iterations run over the 4 rounds. */
int gf_pose_opt(gf_ctx* ctx, const float* Tcw_in, const gf_pose_edge* edges, int n, float fx, float fy, float cx,
                float cy, float* Tcw_out, uint8_t* outlier, int32_t* ninliers, int32_t* iterations);

/* Device family, nprob independent problems (one workgroup each). d_Tcw is
 * nprob x 16 floats, updated in place; problem p owns edges
 * [p*edge_stride, p*edge_stride + d_nedges[p]) and the same outlier slots.
 * d_iterations may be NULL. edge_stride <= 8192. */
int gf_pose_opt_batch_dev(gf_ctx* ctx, int nprob, float* d_Tcw, const gf_pose_edge* d_edges, const int32_t* d_nedges,
                          int edge_stride, float fx, float fy, float cx, float cy, uint8_t* d_outlier,
                          int32_t* d_ninliers, int32_t* d_iterations, void* stream);

/* Device family over Frames: gathers the edges of every keypoint with
 * d_kp2mp >= 0 (X = d_map[kp2mp].pos of that frame's map, z = keypoint,
 * inv_sigma2[octave]), optimises d_Tcw in place and writes mvbOutlier for the
 * matched keypoints (others untouched). inv_sigma2 is a host array of nlevels
 * (<= 16) floats. kp_stride <= 8192. d_nedges (nInitialCorrespondences) and
 * d_iterations may be NULL. */
int gf_pose_opt_frames_dev(gf_ctx* ctx, int nframes, float* d_Tcw, const gf_keypoint* d_kps, const int32_t* d_nkps,
                           int kp_stride, const int32_t* d_kp2mp, const gf_map_point* d_map, int map_stride,
                           const float* inv_sigma2, int nlevels, float fx, float fy, float cx, float cy,
                           uint8_t* d_outlier, int32_t* d_ninliers, int32_t* d_iterations, int32_t* d_nedges,
                           void* stream);

/* --------------------------------------- ORB vocabulary, BoW (D1), SearchByBoW (M6)
 * A DBoW2 ORB vocabulary tree (TemplatedVocabulary<FORB::TDescriptor, FORB>,
 * Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h) as its loaders build it:
 * node 0 is the root; nodes 1..nnodes-1 in file record order with their
 * parent, 32-byte descriptor, weight and leaf flag; a node's children in
 * record order; word ids in record order of the leaves. scoring is DBoW2's
 * ScoringType (0 L1_NORM, 1 L2_NORM, 2 CHI_SQUARE, 3 KL, 4 BHATTACHARYYA,
 * 5 DOT_PRODUCT), weighting its WeightingType (0 TF_IDF, 1 TF, 2 IDF, 3 BINARY). */
typedef struct gf_vocab_arrays {
    int32_t k, L, scoring, weighting, nnodes;
    int32_t* parent;  /* nnodes; parent[0] = -1 */
    uint8_t* desc;    /* nnodes x 32 */
    double* weight;   /* nnodes */
    uint8_t* is_leaf; /* nnodes */
} gf_vocab_arrays;

typedef struct gf_vocab gf_vocab;

/* Host only: parse a vocabulary file — loadFromTextFile (TemplatedVocabulary.h:1352-1432)
 * for a ".txt" path, loadFromBinaryFile (:1469-1510) otherwise. With out->parent
 * == NULL only the header fields and nnodes are filled; call again with buffers
 * of nnodes entries. */
int gf_vocab_read(const char* path, gf_vocab_arrays* out);
/* Host only: TemplatedVocabulary::saveToBinaryFile (TemplatedVocabulary.h:1516-1536;
 * tools/bin_vocabulary.cc converts ORBvoc.txt with it): header {nb_nodes,
 * size_node = 41, k, L, scoring, weighting}, then nodes 1..nnodes-1 as {uint32
 * parent, 32 descriptor bytes, float weight, bool is_leaf}, is_leaf meaning "has
 * no children" as Node::isLeaf. */
int gf_vocab_save_binary(const gf_vocab_arrays* tree, const char* path);
/* Upload a tree (device-resident, shared by every frame of the context). */
int gf_vocab_create(gf_ctx* ctx, const gf_vocab_arrays* tree, gf_vocab** out);
/* gf_vocab_read + gf_vocab_create (main.cc:92-106 picks the loader by suffix). */
int gf_vocab_load(gf_ctx* ctx, const char* path, gf_vocab** out);
int gf_vocab_info(gf_vocab* voc, int* k, int* L, int* nnodes, int* nwords);
/* The vocabulary's ScoringType and WeightingType (BowVector.h:34-53), as
 * created, loaded or received. */
int gf_vocab_scoring(gf_vocab* voc, int* scoring, int* weighting);
int gf_vocab_destroy(gf_vocab* voc);

/* Frame::ComputeBoW (Frame.cc:380-387) = transform(descriptors, mBowVec,
 * mFeatVec, levelsup) (TemplatedVocabulary.h:1141-1208, 1232-1273): the
 * BowVector as words[0..nwords) ascending with values, the FeatureVector as
 * fv_nodes[0..nfv) ascending with the feature indices of node i in
 * fv_feats[fv_start[i] .. fv_start[i+1]). Capacities n (fv_start n + 1).
 * At most 4096 descriptors per frame. */
int gf_bow_transform(gf_vocab* voc, const uint8_t* desc, int n, int levelsup, int32_t* words, double* values,
                     int* nwords, int32_t* fv_nodes, int32_t* fv_start, int32_t* fv_feats, int* nfv);
/* Device family: nframes frames, descriptors and outputs strided by cap. */
int gf_bow_transform_dev(gf_vocab* voc, int nframes, const uint8_t* d_desc, const int32_t* d_n, int cap, int levelsup,
                         int32_t* d_words, double* d_values, int32_t* d_nwords, int32_t* d_fv_nodes,
                         int32_t* d_fv_start, int32_t* d_fv_feats, int32_t* d_nfv, void* stream);

/* One side of ORBmatcher::SearchByBoW: its FeatureVector, descriptors,
 * keypoints (for the angle) and map point per feature (-1 = none or bad). */
typedef struct gf_bow_side {
    const int32_t* fv_nodes;
    const int32_t* fv_start;
    const int32_t* fv_feats;
    int32_t nfv;
    const uint8_t* desc;
    const gf_keypoint* kps;
    const int32_t* mp;
    int32_t n;
} gf_bow_side;

/* mode 0: SearchByBoW(KeyFrame* a, Frame& b, vpMapPointMatches)
 *   (ORBmatcher.cc:724-853): out has b.n entries, out[j] = a's map point
 *   matched to b feature j or -1; a feature needs a map point, best <= TH_LOW.
 * mode 1: SearchByBoW(KeyFrame* a, KeyFrame* b, vpMatches12) (:1289-1424):
 *   out has a.n entries, out[i] = b's map point matched to a feature i; b
 *   features need a map point, best < TH_LOW.
 * Both: best < nnratio * second, rotation consistency (ComputeThreeMaxima
 * :2338-2379) when check_ori. nmatches = the returned count. */
int gf_match_bow(gf_ctx* ctx, int mode, float nnratio, int check_ori, const gf_bow_side* a, const gf_bow_side* b,
                 int32_t* out, int* nmatches);
/* Device family: npairs (a[p], b[p]) pairs whose pointers are device
 * pointers; outs[p] device output of pair p, d_nmatches[p]. The host arrays a,
 * b, outs are copied at the call. At most 4096 features per side. */
int gf_match_bow_dev(gf_ctx* ctx, int mode, float nnratio, int check_ori, int npairs, const gf_bow_side* a,
                     const gf_bow_side* b, int32_t* const* outs, int32_t* d_nmatches, void* stream);

/* ------------------------------------------------ local bundle adjustment (B1)
 * Optimizer::LocalBundleAdjustment(KeyFrame*, bool*) (src/Optimizer.cc:1515-1764)
 * on g2o's Levenberg-Marquardt with the Schur complement over the map points
 * (core/block_solver.hpp:354-486): optimize(5), drop the edges with chi2 >
 * 5.991 or negative depth, optimize(10), flag the outliers again.
 *
 * The caller passes the graph the reference builds (Optimizer.cc:1517-1675)
 * as plain arrays, in the reference's orders:
 *   keyframes in vertex-id order (mnId), kind 0 = local keyframe, 1 = local
 *     keyframe that is fixed (mnId == 0; written back), 2 = fixed camera
 *     (lFixedCameras: a fixed vertex, not written back);
 *   map points in vertex-id order (mnId), their world positions;
 *   edges in insertion order (lLocalMapPoints, then each point's
 *     observations); the edges of one point are contiguous and a point has
 *     at most one edge per keyframe (map<KeyFrame*, size_t>).
 * Results: poses of kinds 0/1 (kind 2 copied through), point positions,
 * per-edge outlier flags (1 = removed after optimize(5), 2 = flagged after
 * optimize(10); the caller erases those observations, Optimizer.cc:1691-1696,
 * 1739-1741) and the iterations of the two optimize() calls (-1 = not run).
 * Limits: at most 32 keyframes of kind 0 per problem, 65536 points. */
typedef struct gf_ba_problem {
    int32_t nkf, npts, nedges;
    const float* kf_Tcw;          /* nkf x 16, row-major KeyFrame::GetPose() */
    const uint8_t* kf_kind;       /* nkf: 0 local, 1 local fixed, 2 fixed camera */
    const float* kf_cam;          /* nkf x 4: fx, fy, cx, cy */
    const float* pt_pos;          /* npts x 3: MapPoint::GetWorldPos() */
    const int32_t* edge_pt;       /* nedges: point index */
    const int32_t* edge_kf;       /* nedges: keyframe index */
    const float* edge_z;          /* nedges x 2: GetKeyPointUn(idx).pt */
    const float* edge_inv_sigma2; /* nedges: GetInvSigma2(octave) */
} gf_ba_problem;

typedef struct gf_ba_result {
    float* kf_Tcw;          /* nkf x 16 */
    float* pt_pos;          /* npts x 3 */
    uint8_t* edge_outlier;  /* nedges */
    int32_t iterations[2];  /* optimize(5), optimize(10) */
} gf_ba_result;

typedef struct gf_ba_plan gf_ba_plan;

/* Host family: one problem, synchronous. */
int gf_local_ba(gf_ctx* ctx, const gf_ba_problem* prob, gf_ba_result* res);

/* Batched device path: gf_ba_plan_create validates and uploads nprob
 * problems and builds their structure (index mapping, per-pose edge lists,
 * Schur panel layout) once; gf_ba_plan_solve runs every problem from its
 * uploaded initial state to the end on `stream` (all problems advance one LM
 * trial per step; the host polls a device done flag every few steps; *steps
 * = steps run); gf_ba_plan_results copies res[0..nprob) out. */
int gf_ba_plan_create(gf_ctx* ctx, int nprob, const gf_ba_problem* probs, gf_ba_plan** out);
int gf_ba_plan_solve(gf_ba_plan* plan, void* stream, int* steps);
int gf_ba_plan_results(gf_ba_plan* plan, gf_ba_result* res);
/* The abortable forms: LocalBundleAdjustment(pKF, &mbAbortBA) with
 * optimizer.setForceStopFlag(pbStopFlag) (Optimizer.cc:1515, 1579-1580;
 * LocalMapping.cc:108). The host polls *stop_flag (written by another thread,
 * as LocalMapping's mbAbortBA is) between LM iterations; once it is set every
 * problem's running optimize() call ends at its next iteration boundary (the
 * iteration in flight completes, as SparseOptimizer::optimize checks
 * terminate() before each iteration), optimize(10) then runs 0 iterations and
 * both outlier checks still run. NULL = never stop. */
int gf_ba_plan_solve_stop(gf_ba_plan* plan, void* stream, const volatile uint8_t* stop_flag, int* steps);
int gf_local_ba_stop(gf_ctx* ctx, const gf_ba_problem* prob, gf_ba_result* res, const volatile uint8_t* stop_flag);
int gf_ba_plan_destroy(gf_ba_plan* plan);

/* Optimizer::BundleAdjustment(vpKFs, vpMP, nIterations, pbStopFlag)
 * (src/Optimizer.cc:36-142; GlobalBundleAdjustemnt :28-33 calls it on the
 * whole map) on the same graph arrays: one optimize(niterations), no outlier
 * pass and no edge removal. The solver's schedule (the iteration caps of the
 * two optimize() calls, whether the outlier passes run) is a property of the
 * plan: gf_ba_plan_create builds the local form's {5, 10} with the passes,
 * gf_ba_plan_create_iters {niterations} without them; the solve and results
 * entries above serve both. Results: edge_outlier all zero, iterations =
 * {run, -1}; a graph without an edge has nothing to optimise (initialize-
 * Optimization fails): {-1, -1}, inputs returned. All three kf_kind values
 * are accepted (BundleAdjustment itself makes 0 and, for mnId == 0, 1).
 * niterations in [0, 64], else GF_ERR_ARG; the limits of the local form hold
 * (GF_ERR_UNSUPPORTED beyond them). stop_flag as in gf_local_ba_stop: raised,
 * optimize() ends at its next iteration boundary. The host loop gives up
 * with an error after 10 * niterations + 1 steps (an iteration takes at most
 * 10 LM trials, one step each). */
int gf_ba_plan_create_iters(gf_ctx* ctx, int nprob, const gf_ba_problem* probs, int niterations, gf_ba_plan** out);
int gf_bundle_adjustment(gf_ctx* ctx, const gf_ba_problem* prob, int niterations, gf_ba_result* res,
                         const volatile uint8_t* stop_flag);
/* Device pointers into the plan's output arrays for problem p (Optimizer.cc:
 * 125-140, the recovered poses and points): kf_Tcw nkf x 16 and pt_pos npts x
 * 3 floats, the values gf_ba_plan_results copies out, and iterations, the two
 * counts of gf_ba_result. Valid after a solve for work enqueued on the same
 * stream, until the next solve or the plan's destruction; any output pointer
 * may be NULL. */
int gf_ba_plan_results_dev(gf_ba_plan* plan, int p, const float** kf_Tcw, const float** pt_pos,
                           const int32_t** iterations);

/* ------------------------------------------------ keypoint undistortion
 * Frame::UndistortKeyPoints (Frame.cc:389-423): cv::undistortPoints with
 * K = {fx, fy, cx, cy} and dist = {k1, k2, p1, p2, k3} (k3 = 0 for the 4-term
 * model); keypoints are copied unchanged when k1 == 0. Only x/y change. */
int gf_undistort_keypoints(gf_ctx* ctx, const float K[4], const float dist[5], const gf_keypoint* kps, int n,
                           gf_keypoint* out);
/* Batched: d_in/d_out are [nframes][cap], d_n[nframes] keypoints each. */
int gf_undistort_keypoints_dev(gf_ctx* ctx, int nframes, const float K[4], const float dist[5],
                               const gf_keypoint* d_in, const int32_t* d_n, int cap, gf_keypoint* d_out, void* stream);

/* ------------------------------------------ local-mapping matchers (§8f rank 3)
 * MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:197-262) for nmp
 * map points at once: point p's observation descriptors (non-bad keyframes,
 * observation-map order) are rows offsets[p] .. offsets[p+1]-1 of desc
 * (offsets has nmp + 1 entries, offsets[0] = 0). best[p] = the row (relative
 * to offsets[p]) with the least median Hamming distance to the others, -1 for
 * a point without observations; out_desc (optional, nmp x 32, in/out)
 * receives that row (mDescriptor), untouched for an empty point. */
int gf_distinctive_descriptors(gf_ctx* ctx, int nmp, const uint8_t* desc, const int32_t* offsets, int32_t* best,
                               uint8_t* out_desc);
/* Device family: total = offsets[nmp] (host value: sizes the row grid). */
int gf_distinctive_descriptors_dev(gf_ctx* ctx, int nmp, const uint8_t* d_desc, const int32_t* d_offsets,
                                   int32_t* d_best, uint8_t* d_out_desc, int total, void* stream);

/* ORBmatcher::Fuse(KeyFrame* pKF, vector<MapPoint*>& vpMapPoints, th)
 * (src/ORBmatcher.cc:1590-1707). The keyframe: bounds/intrinsics/pyramid in
 * fi, pose Tcw (row-major 4x4), camera centre Ow (KeyFrame::GetCameraCenter),
 * undistorted keypoints, descriptors, kf_mp[k] = id of the map point at slot k
 * (-1 none) and kf_mp_bad[k] its isBad() (optional). The candidates:
 * gf_map_point (mfMin/MaxDistance are the invariance distances), descriptors,
 * mp_skip[i] (optional) = NULL / isBad() / IsInKeyFrame(pKF), mp_ids[i]
 * (optional, default i) the id reported as a Replace() target. Result per
 * candidate in list order:
 *   kp      keypoint fused with (bestDist <= TH_LOW) or -1;
 *   action  GF_FUSE_ADD      pMP->AddObservation(pKF, kp), pKF->AddMapPoint;
 *           GF_FUSE_REPLACE  pMP->Replace(target): target is the slot's
 *                            occupant, or the earlier candidate that took the
 *                            empty slot in this call;
 *           GF_FUSE_KEEP     the occupant isBad(): nothing changes;
 *   nfused = number of candidates with kp >= 0 (the reference's nFused). */
enum { GF_FUSE_NONE = 0, GF_FUSE_ADD = 1, GF_FUSE_REPLACE = 2, GF_FUSE_KEEP = 3 };
typedef struct gf_fuse_result {
    int32_t kp, action, target;
} gf_fuse_result;
int gf_fuse(gf_ctx* ctx, const gf_frame_info* fi, const float* Tcw, const float* Ow, const gf_keypoint* kps,
            const uint8_t* desc, int n, const int32_t* kf_mp, const uint8_t* kf_mp_bad, const gf_map_point* mps,
            const uint8_t* mp_desc, const uint8_t* mp_skip, const int32_t* mp_ids, int m, float th,
            gf_fuse_result* res, int* nfused);
/* Device family: nprob independent (keyframe, candidate list) problems that
 * share fi; every pointer in a problem is a device pointer (the array itself
 * is host memory, copied at the call). At most 4096 keypoints per keyframe. */
typedef struct gf_fuse_problem {
    float Tcw[16];
    float Ow[3];
    const gf_keypoint* kps;
    const uint8_t* desc;
    int32_t n;
    const int32_t* kf_mp;
    const uint8_t* kf_mp_bad;
    const gf_map_point* mps;
    const uint8_t* mp_desc;
    const uint8_t* mp_skip;
    const int32_t* mp_ids;
    int32_t m;
    float th;
    gf_fuse_result* res;
    int32_t* nfused;
} gf_fuse_problem;
int gf_fuse_dev(gf_ctx* ctx, const gf_frame_info* fi, int nprob, const gf_fuse_problem* probs, void* stream);

/* The search half of ORBmatcher::Fuse(pKF, vpMapPoints, th)
 * (src/ORBmatcher.cc:1607-1687) up to the choice of bestIdx, the searches
 * LocalMapping::SearchInNeighbors (src/LocalMapping.cc:436-468) runs: candidates
 * are map point ids into the whole-map arrays mps / mp_desc / mp_bad (nmp rows),
 * no gathered copy. Tcw (row-major 4x4) and Ow (KeyFrame::GetCameraCenter) come
 * from the caller as for gf_fuse. points[i] = -1 is a NULL slot (:1611);
 * skip[i] (optional) is the caller's IsInKeyFrame(pKF) read from the
 * observation map (:1614). Result per candidate in list order: kp = bestIdx and
 * dist = bestDist when bestDist <= TH_LOW (:1690), else {-1, -1}; a candidate
 * with id < 0 or >= nmp, with mp_bad set or with skip set gets {-1, -1}.
 * KeyFrame::GetFeaturesInArea order decides ties. What :1690-1703 does with kp
 * depends on the live map (MapPoint::Replace moves observations and turns
 * candidates bad) and is the caller's. Host arrays, one keyframe. */
typedef struct gf_fuse_search_result {
    int32_t kp, dist;
} gf_fuse_search_result;
int gf_fuse_search(gf_ctx* ctx, const gf_frame_info* fi, const float* Tcw, const float* Ow, const gf_keypoint* kps,
                   const uint8_t* desc, int n, const gf_map_point* mps, const uint8_t* mp_desc, const uint8_t* mp_bad,
                   int nmp, const int32_t* points, const uint8_t* skip, int npoints, float th,
                   gf_fuse_search_result* res);
/* Device family: nprob (keyframe, candidate-id list) searches in one launch,
 * enqueued on stream without synchronising. The problem array is host memory,
 * copied at the call; every pointer in it, and d_mps / d_mp_desc / d_mp_bad
 * (nmp rows, shared by all problems, d_mp_bad optional), is a device pointer.
 * A long candidate list is spread over several workgroups, so one keyframe
 * against the union of its neighbours' points (:468) fills the machine. At most
 * 4096 keypoints per keyframe; res entries past npoints are never written. */
typedef struct gf_fuse_search_problem {
    float Tcw[16];
    float Ow[3];
    float th;
    const gf_keypoint* kps;
    const uint8_t* desc;
    int32_t n;
    const int32_t* points;
    const uint8_t* skip;
    int32_t npoints;
    gf_fuse_search_result* res;
} gf_fuse_search_problem;
int gf_fuse_search_dev(gf_ctx* ctx, const gf_frame_info* fi, int nprob, const gf_fuse_search_problem* probs,
                       const gf_map_point* d_mps, const uint8_t* d_mp_desc, const uint8_t* d_mp_bad, int nmp,
                       void* stream);
/* Candidates per workgroup of gf_fuse_search_dev on this context, for
 * measurements (scripts/neighbors_bench.py); the default, 256, is the measured
 * choice. A value outside [64, 65536] is an error and changes nothing. The
 * results do not depend on it. */
int gf_fuse_search_set_chunk(gf_ctx* ctx, int chunk);

/* MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:285-324) for npts points.
 * pos[npts][3]; the observing keyframes of point p are obs_kf[offsets[p] ..
 * offsets[p + 1]) in observation-map order (the order of the float sum at
 * :302-309); kf_Ow[nkf][3] the camera centres; ref_kf[p] = mpRefKF and
 * ref_level[p] = the octave of observations[pRefKF] in it (:313), computed by
 * the caller; the pyramid comes from fi. cv::norm is a double sum cast to
 * float and Mat / scalar one float factor (float)(1 / scalar). normal, min_dist
 * and max_dist are in / out: a point with an empty row or ref_kf < 0, where
 * the reference divides by zero, is left untouched. Host arrays. */
int gf_update_normal_and_depth(gf_ctx* ctx, const gf_frame_info* fi, int npts, const float* pos, const int32_t* offsets,
                               const int32_t* obs_kf, const float* kf_Ow, int nkf, const int32_t* ref_kf,
                               const int32_t* ref_level, float* normal, float* min_dist, float* max_dist);
/* Device family: device pointers, enqueued on stream without synchronising. */
int gf_update_normal_and_depth_dev(gf_ctx* ctx, const gf_frame_info* fi, int npts, const float* d_pos,
                                   const int32_t* d_offsets, const int32_t* d_obs_kf, const float* d_kf_Ow, int nkf,
                                   const int32_t* d_ref_kf, const int32_t* d_ref_level, float* d_normal,
                                   float* d_min_dist, float* d_max_dist, void* stream);

/* The counting of LocalMapping::KeyFrameCulling (src/LocalMapping.cc:562-616)
 * for ncand candidate keyframes cand[c] in one launch. The tables are flat:
 * kf_off[nkf + 1] prefix sums of the keyframes' keypoint counts (nkp =
 * kf_off[nkf]); octave[nkp] = GetKeyPointUn(i).octave and slots[nkp] =
 * mvpMapPoints of every keyframe, keyframe-major; mp_bad[nmp]; the observation
 * maps as CSR rows obs_gkp[obs_off[p] .. obs_off[p + 1]) of global keypoint
 * indices kf_off[kf'] + idx', point-major in observation-map order, -1 = an
 * erased observation, which is skipped. For every slot i of candidate K whose
 * point p has 0 <= p < nmp and !mp_bad[p]: nmps++ (:585); when the row has
 * more than 3 live entries (:586), those outside [kf_off[K], kf_off[K + 1])
 * (:594) with octave[g] <= octave[kf_off[K] + i] + 1 (:597) are counted, and
 * the slot is redundant when they reach 3 (:604). A point in two slots counts
 * per slot, a point that does not list K counts every observer, and no observer
 * is tested for isBad(), as in the reference. counts[c] = {nmps, nredundant};
 * flags (optional, nkp bytes) gets 0 = NULL or bad, 1 = counted, 2 = redundant
 * inside the candidates' slot ranges and is not written elsewhere. The
 * decision nredundant > 0.9 * nmps (:613) is a double comparison and the
 * caller's. Host arrays, synchronous; at most 4096 keypoints per keyframe. */
int gf_keyframe_culling_counts(gf_ctx* ctx, int nkf, const int32_t* kf_off, const uint8_t* octave, const int32_t* slots,
                               int nmp, const uint8_t* mp_bad, const int32_t* obs_off, const int32_t* obs_gkp,
                               int ncand, const int32_t* cand, int32_t* counts, uint8_t* flags);
/* Device family (src/LocalMapping.cc:562-616): device pointers, the totals nkp
 * and nobs given by the caller, enqueued on stream without synchronising. An
 * entry of d_obs_gkp outside [0, nkp) is skipped like -1, a candidate outside
 * [0, nkf) gets {0, 0}. */
int gf_keyframe_culling_counts_dev(gf_ctx* ctx, int nkf, int nkp, const int32_t* d_kf_off, const uint8_t* d_octave,
                                   const int32_t* d_slots, int nmp, const uint8_t* d_mp_bad, const int32_t* d_obs_off,
                                   const int32_t* d_obs_gkp, int nobs, int ncand, const int32_t* d_cand,
                                   int32_t* d_counts, uint8_t* d_flags, void* stream);

/* The counting and ordering of KeyFrame::UpdateConnections (src/KeyFrame.cc:
 * 332-403) for nq query keyframes query[i] in one launch, over the flat tables
 * of gf_keyframe_culling_counts (kf_off, slots, mp_bad, obs_off / obs_gkp; the
 * octaves are not read). Every output has nq rows of nkf entries.
 *   weights[i][k] = KFcounter[k] (:341-361): for every slot of the query in
 *     slot order whose point p has 0 <= p < nmp and !mp_bad[p], every entry of
 *     p's row whose keyframe is not the query adds one to that keyframe. A point
 *     in two slots counts twice, a point whose row does not list the query
 *     counts every observer, entries equal to -1 or outside [0, nkp) are
 *     skipped, and no observer is tested for isBad(), as in the reference.
 *     0 = not in the counter.
 *   n_ordered[i], ordered_kf[i][0 .. n), ordered_w[i][0 .. n) =
 *     mvpOrderedConnectedKeyFrames / mvOrderedWeights (:369-403): the keyframes
 *     with weights >= 15 by (weight, index) descending, the higher index first
 *     among equal weights (the sort of (int, KeyFrame*) pairs, reversed); when
 *     none reaches 15 the single heaviest, the lowest index among equals (the
 *     strict > of :378); n = 0 exactly when the counter is empty (the return
 *     of :365). The rows are filled up with -1 / 0 past n.
 * A query outside [0, nkf) gets a zero row and n = 0; a query may repeat. The
 * graph updates of :376-418 are the caller's. Host arrays, synchronous;
 * GF_ERR_ARG for kf_off / obs_off that do not start at 0 or decrease,
 * GF_ERR_CAP above 4096 keypoints in a keyframe; nkf is bounded by memory
 * only. */
int gf_update_connections(gf_ctx* ctx, int nkf, const int32_t* kf_off, const int32_t* slots, int nmp,
                          const uint8_t* mp_bad, const int32_t* obs_off, const int32_t* obs_gkp, int nq,
                          const int32_t* query, int32_t* weights, int32_t* n_ordered, int32_t* ordered_kf,
                          int32_t* ordered_w);
/* Device family (src/KeyFrame.cc:332-403): device pointers, the totals nkp and
 * nobs given by the caller, enqueued on stream without synchronising; every
 * entry of the four outputs is written, so they need no clearing. The tables
 * are not read on the host: a row outside [0, nobs) is clamped, a keyframe is
 * walked up to 4096 slots. */
int gf_update_connections_dev(gf_ctx* ctx, int nkf, int nkp, const int32_t* d_kf_off, const int32_t* d_slots, int nmp,
                              const uint8_t* d_mp_bad, const int32_t* d_obs_off, const int32_t* d_obs_gkp, int nobs,
                              int nq, const int32_t* d_query, int32_t* d_weights, int32_t* d_n_ordered,
                              int32_t* d_ordered_kf, int32_t* d_ordered_w, void* stream);

/* Resident map tables: the flat tables of gf_keyframe_culling_counts kept on
 * the device and updated in place by a journal of the map's own writes. The
 * observation table is a slack CSR: obs_off[p] .. obs_off[p + 1] is the
 * capacity of row p; inside it sit the live entries in ascending order of the
 * global keypoint index kf_off[kf] + idx (= observation-map order), then -1 up
 * to the capacity. The three consumers above skip -1, so they read such a
 * table as it is.
 *
 * gf_map_tables_apply applies one journal:
 *   slot_g[nslot], slot_v[nslot]: slots[slot_g[i]] = slot_v[i], what
 *     KeyFrame::AddMapPoint, ReplaceMapPointMatch (a point id) and
 *     EraseMapPointMatch (-1) write (src/KeyFrame.cc:210-236);
 *   bad_p[nbad]: mp_bad[bad_p[i]] = 1 (mbBad of MapPoint::SetBadFlag,
 *     src/MapPoint.cc:117-131, and Replace, :136-170);
 *   the observation ops, stable-sorted by point: row_ids[nrows] the touched
 *     points, each once; row_op_off[nrows + 1] the ranges into ops[nops][3] =
 *     (kind, kf, idx), applied to the row serially in journal order:
 *       GF_MT_OBS_SET   mObservations[kf] = idx (MapPoint::AddObservation,
 *         MapPoint.cc:77-81): an entry inside [kf_off[kf], kf_off[kf + 1]) is
 *         overwritten with kf_off[kf] + idx, otherwise the entry is inserted
 *         at its ascending place (after the entries below kf_off[kf]);
 *       GF_MT_OBS_ERASE mObservations.erase(kf) (EraseObservation, :83-103):
 *         the entry inside the keyframe's range goes, nothing when absent;
 *       GF_MT_OBS_CLEAR mObservations.clear() (SetBadFlag, Replace).
 *     The row is then written back as its live entries followed by -1 up to
 *     the capacity; every entry of a touched row is written.
 * Targets must be unique (the caller keeps the last write per slot).
 * status[0] counts the rows left byte for byte untouched because their final
 * length exceeds their capacity or a length on the way exceeds GF_MT_ROW
 * entries (the length on the way may exceed the capacity); status[1] counts the
 * ops skipped because their p, g, kf, idx or kind is out of range (a row id
 * outside [0, nmp) skips all its ops). An entry >= 0 is live. Host arrays,
 * synchronous, slots / mp_bad / obs_gkp updated in place; GF_ERR_ARG for
 * kf_off / obs_off / row_op_off that do not start at 0, decrease or disagree
 * with the lengths, row_ids that do not strictly increase and repeated slot
 * targets. */
enum { GF_MT_OBS_SET = 0, GF_MT_OBS_ERASE = 1, GF_MT_OBS_CLEAR = 2 };
#define GF_MT_ROW 1024
int gf_map_tables_apply(gf_ctx* ctx, int nkf, const int32_t* kf_off, int32_t* slots, int nmp, uint8_t* mp_bad,
                        const int32_t* obs_off, int32_t* obs_gkp, int nslot, const int32_t* slot_g,
                        const int32_t* slot_v, int nbad, const int32_t* bad_p, int nrows, const int32_t* row_ids,
                        const int32_t* row_op_off, int nops, const int32_t* ops, int32_t* status);
/* Device family (MapPoint.cc:77-81, :83-103, :117-131, :136-170; KeyFrame::
 * AddMapPoint / EraseMapPointMatch / ReplaceMapPointMatch): device pointers,
 * the totals nkp and nobs given by the caller, enqueued on stream without
 * synchronising. d_status[2] is cleared on the stream first. Nothing is read on
 * the host: a row outside [0, nobs) is clamped, an op range outside [0, nops)
 * too; repeated targets or row ids race (each write stays inside the tables). */
int gf_map_tables_apply_dev(gf_ctx* ctx, int nkf, int nkp, const int32_t* d_kf_off, int32_t* d_slots, int nmp,
                            uint8_t* d_mp_bad, const int32_t* d_obs_off, int32_t* d_obs_gkp, int nobs, int nslot,
                            const int32_t* d_slot_g, const int32_t* d_slot_v, int nbad, const int32_t* d_bad_p,
                            int nrows, const int32_t* d_row_ids, const int32_t* d_row_op_off, int nops,
                            const int32_t* d_ops, int32_t* d_status, void* stream);

/* The regrow of a slack CSR: every row's live entries (>= 0), compacted and in
 * order, are copied from old_gkp[old_off[p] .. old_off[p + 1]) to
 * new_gkp[new_off[p] ..] and the rest of the new capacity is filled with -1, so
 * every entry of the new table is written. Entries equal to -1 anywhere in an
 * old row are legal (the point updates of a cull leave them). A row whose new
 * capacity is below its live count is written as all -1 and counted in
 * status[0]. The observation maps themselves do not change: this stands for no
 * line of the reference, it makes room for the MapPoint::AddObservation
 * (MapPoint.cc:77-81) entries of the journal that follows. Host arrays,
 * synchronous; the two tables must not overlap; GF_ERR_ARG for offsets that do
 * not start at 0 or decrease. */
int gf_map_tables_move(gf_ctx* ctx, int nmp, const int32_t* old_off, const int32_t* old_gkp, const int32_t* new_off,
                       int32_t* new_gkp, int32_t* status);
/* Device family: device pointers, the totals nobs_old and nobs_new given by the
 * caller, enqueued on stream without synchronising; d_status[1] is cleared on
 * the stream first. Rows are clamped to the tables they lie in. */
int gf_map_tables_move_dev(gf_ctx* ctx, int nmp, const int32_t* d_old_off, const int32_t* d_old_gkp, int nobs_old,
                           const int32_t* d_new_off, int32_t* d_new_gkp, int nobs_new, int32_t* d_status,
                           void* stream);

/* The graph assembly of Optimizer::LocalBundleAdjustment (src/Optimizer.cc:
 * 1517-1675) over flat tables of the whole map: the five tables of
 * gf_keyframe_culling_counts (kf_off, octave, slots, mp_bad, obs_off /
 * obs_gkp, -1 = an erased observation) plus kf_bad[nkf], kp_xy[nkp x 2] =
 * GetKeyPointUn(i).pt keyframe-major like octave, inv_sigma2[nlevels] =
 * GetInvSigma2(level), kf_Tcw[nkf x 16], mp_pos[nmp x 3], one camera cam =
 * {fx, fy, cx, cy}, and kf0 = the index of the keyframe with mnId 0 (-1: not
 * in the map). Keyframe indices are in mnId order. */
typedef struct gf_lba_tables {
    int32_t nkf, nkp, nmp, nobs, nlevels, kf0;
    const int32_t* kf_off;   /* nkf + 1 */
    const uint8_t* octave;   /* nkp */
    const int32_t* slots;    /* nkp */
    const uint8_t* kf_bad;   /* nkf */
    const float* kp_xy;      /* nkp x 2 */
    const float* kf_Tcw;     /* nkf x 16 */
    const uint8_t* mp_bad;   /* nmp */
    const float* mp_pos;     /* nmp x 3 */
    const int32_t* obs_off;  /* nmp + 1 */
    const int32_t* obs_gkp;  /* nobs */
    const float* inv_sigma2; /* nlevels */
    float cam[4];
} gf_lba_tables;

/* The assembled gf_ba_problem and what the write-back needs. Every buffer is
 * sized by its safe bound (nkf keyframes, nmp points, nobs edges of the
 * tables); counts = {nkf, npts, nedges} of the problem. prob_kf / prob_pt:
 * the map index of every problem keyframe / point; edge_gkp: the global
 * keypoint index kf_off[kf] + idx of every edge. */
typedef struct gf_lba_graph_out {
    int32_t* counts;        /* 3 */
    int32_t* prob_kf;       /* nkf */
    uint8_t* kf_kind;       /* nkf */
    float* kf_Tcw;          /* nkf x 16 */
    float* kf_cam;          /* nkf x 4 */
    int32_t* prob_pt;       /* nmp */
    float* pt_pos;          /* nmp x 3 */
    int32_t* edge_pt;       /* nobs */
    int32_t* edge_kf;       /* nobs */
    float* edge_z;          /* nobs x 2 */
    float* edge_inv_sigma2; /* nobs */
    int32_t* edge_gkp;      /* nobs */
} gf_lba_graph_out;

/* Optimizer.cc:1517-1675 on host arrays, synchronous. local[0] is the current
 * keyframe, local[1..nlocal) its GetVectorCovisibleKeyFrames() in list order
 * with the bad ones left out (:1523-1530). The problem, in the orders
 * gf_ba_problem demands:
 *   keyframes in index order: the local list (kind 0, or 1 for kf0) united
 *     with the fixed cameras (kind 2): the observers of a local point that are
 *     neither local nor bad (:1552-1566);
 *   points in id order: every point with 0 <= p < nmp and !mp_bad[p] found in
 *     a slot of a local keyframe (:1534-1548);
 *   edges: the points in lLocalMapPoints order (first occurrence when the
 *     local keyframes are walked in list order and their slots in index
 *     order), each point's row in row order, -1 entries and observers with
 *     kf_bad skipped (:1644).
 * GF_ERR_ARG, nothing written, for: kf_off / obs_off that do not start at 0,
 * decrease or do not end at nkp / nobs, a keyframe above 4096 keypoints, an
 * octave >= nlevels, nlevels outside [1, 16], an observation entry outside
 * [-1, nkp), kf0 outside [-1, nkf), an empty local list, a local index
 * outside [0, nkf), a repeat, or more than 32 local keyframes of kind 0 (the
 * solver's limit). */
int gf_lba_graph(gf_ctx* ctx, const gf_lba_tables* tables, int nlocal, const int32_t* local,
                 const gf_lba_graph_out* out);
/* Device family (Optimizer.cc:1517-1675): the pointers of d_tables and d_out
 * are device pointers (the two structs and local are host memory, read at the
 * call), enqueued on stream without synchronising; the entry clears its own
 * workspace. kf_Tcw, kp_xy and the float outputs are read and written as
 * 16- and 8-byte vectors: device allocations as they come (hipMalloc, a
 * tensor's storage) are aligned enough. The local list is checked as above; the tables are not read on
 * the host: a slot outside [0, nmp), a row outside [0, nobs) and an entry
 * outside [0, nkp) are skipped, a keyframe is walked up to 4096 slots, an
 * octave is clamped to nlevels - 1. */
int gf_lba_graph_dev(gf_ctx* ctx, const gf_lba_tables* d_tables, int nlocal, const int32_t* local,
                     const gf_lba_graph_out* d_out, void* stream);

/* ORBmatcher::SearchForTriangulation(pKF1, pKF2, F12, ...) (src/ORBmatcher.cc:
 * 1426-1588): keypoints of a (pKF1) and b (pKF2) without a map point
 * (mp < 0) that share a FeatureVector node; best distance <= TH_LOW, the
 * candidates within 2x the best walked in (distance, index) order, the first
 * passing CheckDistEpipolarLine (:705-722: squared distance to the epipolar
 * line x1' F12 < 3.84 sigma2_b[octave]) matches; rotation consistency when
 * check_ori. F12 row-major 3x3; sigma2_b = pKF2's mvLevelSigma2 (nlevels <= 16).
 * out[i] (a.n entries) = the b keypoint matched to a keypoint i or -1
 * (vMatches12; vMatchedPairs are its non-negative entries in order). */
int gf_search_for_triangulation(gf_ctx* ctx, int check_ori, const gf_bow_side* a, const gf_bow_side* b,
                                const float* F12, const float* sigma2_b, int nlevels, int32_t* out, int* nmatches);
/* Device family: npairs independent (a[p], b[p]) keyframe pairs (device
 * pointers; LocalMapping::CreateNewMapPoints pairs the new keyframe with each
 * covisible neighbour), F12 host array of npairs x 9, one sigma2 table,
 * outs[p] device output of pair p, d_nmatches[p]. One workgroup per pair. */
int gf_search_for_triangulation_dev(gf_ctx* ctx, int check_ori, int npairs, const gf_bow_side* a,
                                    const gf_bow_side* b, const float* F12, const float* sigma2_b, int nlevels,
                                    int32_t* const* outs, int32_t* d_nmatches, void* stream);

/* ------------------------------------------------ CreateNewMapPoints
 * LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:243-409) with
 * ComputeF12 (:490-507) and KeyFrame::ComputeSceneMedianDepth
 * (src/KeyFrame.cc:659-689): the new keyframe `cur` against its covisible
 * neighbours, in the given order. Per neighbour: the baseline test
 * (|Ow2 - Ow1| / median scene depth of the neighbour < 0.01 skips it), F12,
 * SearchForTriangulation of (cur, neighbour), and per match the linear
 * triangulation (4x4 CV_32F SVD) with the parallax, depth, reprojection
 * (5.991 sigma2) and scale-consistency tests. An accepted match becomes a
 * new map point: its id goes into cur's slot table at idx1 and into the
 * neighbour's at idx2, so the search against the next neighbour skips that
 * keypoint (ORBmatcher.cc:1466-1469) — the neighbours are a chain, not
 * independent pairs.
 *
 * A keyframe: Tcw (row-major 4x4), its gf_bow_side (side.mp is ignored) and
 * its writable slot table mp[side.n] (mvpMapPoints: map point id or -1). The
 * slot tables of cur and of all neighbours are distinct arrays. Both share
 * fi (one camera, one scale pyramid). mp_pos[nmp][3]: world positions of the
 * existing points, for the median depth (every slot id in 0..nmp-1 counts,
 * bad points included: the reference only tests the pointer).
 * New points get the ids nmp + 0, 1, 2, ... in creation order: neighbour by
 * neighbour, inside one neighbour by ascending idx1 (vMatchedIndices order).
 * At most 4096 keypoints per keyframe and 20 neighbours. */
enum { GF_NEWPTS_MAX_NEIGH = 20 };
enum { GF_NP_OK = 0, GF_NP_BASELINE = 1, GF_NP_NODEPTH = 2 }; /* per-neighbour status */
/* where a match left the per-match body (:307-407); -1 = keypoint not matched */
enum {
    GF_NP_EXIT_PARALLAX = 0, /* cosParallaxRays < 0 or > 0.9998 (:322)  */
    GF_NP_EXIT_W0 = 1,       /* x3D(3) == 0 (:337)                      */
    GF_NP_EXIT_Z1 = 2,       /* z1 <= 0 (:346)                          */
    GF_NP_EXIT_Z2 = 3,       /* z2 <= 0 (:350)                          */
    GF_NP_EXIT_REPROJ1 = 4,  /* (:362)                                  */
    GF_NP_EXIT_REPROJ2 = 5,  /* (:374)                                  */
    GF_NP_EXIT_DIST0 = 6,    /* dist1 == 0 or dist2 == 0 (:384)         */
    GF_NP_EXIT_SCALE = 7,    /* (:389)                                  */
    GF_NP_EXIT_ACCEPTED = 8
};
typedef struct gf_newpoints_kf {
    float Tcw[16];
    gf_bow_side side;
    int32_t* mp;
} gf_newpoints_kf;
typedef struct gf_newpoints_neigh {
    int32_t status;     /* GF_NP_BASELINE: skipped at :280; GF_NP_NODEPTH: the neighbour
                           has no map point (undefined in the reference), skipped */
    float F12[9];       /* zeros when skipped */
    float median_depth; /* 0 when GF_NP_NODEPTH */
    int32_t nmatches;   /* vMatchedIndices.size() */
    int32_t naccepted;
} gf_newpoints_neigh;
typedef struct gf_newpoint {
    int32_t neighbour, idx1, idx2;
    float pos[3];
} gf_newpoint;
/* Device family: every pointer inside cur / neigh[i] is a device pointer (the
 * structs are host memory, copied at the call); d_mp_pos, d_report[nneigh],
 * d_points[cap], d_exits[nneigh][cur->side.n] and d_total[1] are device
 * memory. Everything is enqueued on `stream` without a host synchronisation:
 * one set-up launch, then the matcher and the triangulation launch per
 * neighbour. d_total = number of points created; records beyond cap are
 * dropped (the slot tables still receive their ids). Entries of d_points past
 * min(total, cap) are not written. nneigh = 0 writes d_total = 0 only. */
int gf_create_new_map_points_dev(gf_ctx* ctx, const gf_frame_info* fi, const gf_newpoints_kf* cur, int nneigh,
                                 const gf_newpoints_kf* neigh, const float* d_mp_pos, int nmp, int check_ori,
                                 int cap, gf_newpoints_neigh* d_report, gf_newpoint* d_points, int32_t* d_exits,
                                 int32_t* d_total, void* stream);
/* Host family: host arrays everywhere, the slot tables updated in place, one
 * synchronisation at the end. GF_ERR_CAP when total > cap (total holds the
 * need; the slot tables are not written back). */
int gf_create_new_map_points(gf_ctx* ctx, const gf_frame_info* fi, const gf_newpoints_kf* cur, int nneigh,
                             const gf_newpoints_kf* neigh, const float* mp_pos, int nmp, int check_ori, int cap,
                             gf_newpoints_neigh* report, gf_newpoint* points, int32_t* exits, int* total);

/* ----------------------------------------- local-map assembly
 * Tracking::UpdateReference (Tracking.cc:3689-3706) =
 * UpdateReferenceKeyFrames (:3768-3852) + UpdateReferencePoints (:3708-3766),
 * for a batch of frames tracking against one map:
 *   - every map point of the frame (mvpMapPoints, keypoint order) that is
 *     not bad votes once for each keyframe observing it; bad ones are set to
 *     -1 in the frame (:3778-3793);
 *   - local keyframes = the voted keyframes that are not bad, in
 *     std::map<KeyFrame*,int> order, i.e. ascending KeyFrame* — which is the
 *     order keyframes are passed in here (Map::GetAllKeyFrames iterates its
 *     std::set<KeyFrame*> that way); the reference keyframe is the first one
 *     with the most votes (:3798-3817);
 *   - while the list holds <= 80, each of the keyframes found so far adds the
 *     first of its best 10 covisible keyframes (GetBestCovisibilityKeyFrames(10))
 *     that is neither bad nor in the list (:3820-3848);
 *   - local map points = the map points of the local keyframes
 *     (GetMapPointMatches, slot order), first occurrence only, not bad
 *     (:3737-3763; GOOD_FEATURE_MAP_BOUND is off in the reference build).
 * The keyframe / map-point "mnTrackReferenceForFrame" marks are the
 * call's own: every call starts from unmarked keyframes and points. */
typedef struct gf_covis_map {
    int32_t nkf, nmp;           /* keyframes (<= 8192), map points            */
    const uint8_t* kf_bad;      /* [nkf] KeyFrame::isBad, ascending KeyFrame* */
    const int32_t* kf_mp_off;   /* [nkf+1] CSR of KeyFrame::mvpMapPoints      */
    const int32_t* kf_mp;       /*   map point index per slot, -1 = NULL      */
    const int32_t* kf_cov_off;  /* [nkf+1] CSR of mvpOrderedConnectedKeyFrames */
    const int32_t* kf_cov;      /*   keyframe indices (the first 10 are used) */
    const uint8_t* mp_bad;      /* [nmp] MapPoint::isBad                      */
    const int32_t* mp_obs_off;  /* [nmp+1] CSR of MapPoint::mObservations     */
    const int32_t* mp_obs;      /*   observing keyframe indices               */
} gf_covis_map;
/* One frame, host arrays (the map is uploaded per call). frame_mps[nkp] is
 * updated in place. Outputs up to the caps; the counts are the full sizes
 * (GF_ERR_CAP when a cap is exceeded). ref_kf = pKFmax index or -1. */
int gf_update_reference(gf_ctx* ctx, const gf_covis_map* map, int32_t* frame_mps, int nkp, int32_t* local_kfs,
                        int* n_local_kfs, int kf_cap, int32_t* local_mps, int* n_local_mps, int mp_cap,
                        int32_t* ref_kf);
/* B frames against one map whose arrays are device pointers (the struct is
 * host memory). d_frame_mps [B][stride] with d_nkps[B]; outputs
 * [B][kf_cap] / [B][mp_cap], counts [B], d_ref_kf [B]. */
int gf_update_reference_dev(gf_ctx* ctx, const gf_covis_map* d_map, int nframes, int32_t* d_frame_mps,
                            const int32_t* d_nkps, int stride, int32_t* d_local_kfs, int32_t* d_n_local_kfs,
                            int kf_cap, int32_t* d_local_mps, int32_t* d_n_local_mps, int mp_cap,
                            int32_t* d_ref_kf, void* stream);

/* ------------------------------------------------ relocalisation PnP
 * ORB_SLAM::PnPsolver (src/PnPsolver.cc, include/PnPsolver.h): EPnP
 * (Lepetit et al.) on random minimal sets inside RANSAC, then a refinement
 * over the best inlier set; Tracking::Relocalization drives it
 * (Tracking.cc:3916-3942: SetRansacParameters(0.99,10,300,4,0.5,5.991), then
 * iterate(5) per candidate keyframe). A problem is the solver's correspondence
 * list in PnPsolver order (ctor :50-72): p3d (n x 3 world points), p2d (n x 2
 * undistorted keypoints), sigma2 (level sigma^2 of each keypoint octave). The
 * keypoint-index mapping (mvKeyPointIndices) stays with the caller. */
typedef struct gf_pnp_params { /* SetRansacParameters arguments (:93) */
    double probability;
    int32_t min_inliers;
    int32_t max_iterations;
    int32_t min_set; /* 1..8 (the reference uses 4) */
    float epsilon;
    float th2;
} gf_pnp_params;
typedef struct gf_pnp_state { /* one solver across iterate() calls */
    int32_t n;              /* N correspondences */
    int32_t min_inliers;    /* mRansacMinInliers after the adjustment (:106-111) */
    int32_t max_iterations; /* mRansacMaxIts after the adjustment (:116-124) */
    int32_t min_set;        /* mRansacMinSet */
    float epsilon;          /* mRansacEpsilon after the adjustment (:113-114) */
    float th2;              /* mvMaxError[i] = sigma2[i] * th2 (:126-128) */
    int32_t iterations;     /* mnIterations */
    int32_t best_inliers;   /* mnBestInliers */
    float best_Tcw[16];     /* mBestTcw, row-major */
} gf_pnp_state;
#define GF_PNP_FOUND 1   /* iterate returned a pose (refined or best)      */
#define GF_PNP_NOMORE 2  /* bNoMore                                        */
#define GF_PNP_REFINED 4 /* the pose came from Refine() (:198-208)         */
#define GF_PNP_TRUNCATED 8 /* device path: max_iterations cut the state's loop short */
/* PnPsolver::SetRansacParameters (host scalar set-up; resets the iteration
 * count and the best hypothesis as a fresh solver has them). */
int gf_pnp_init(int n, const gf_pnp_params* params, gf_pnp_state* state);
/* PnPsolver::iterate(nIterations, bNoMore, vbInliers, nInliers) (:137-230)
 * for one solver; rng is the process-wide std::rand() state the minimal sets
 * are drawn from (DUtils::Random::RandomInt, :165), advanced by min_set draws
 * per iteration run. best_mask (n bytes, mvbBestInliers) persists across calls
 * with the state. Outputs: Tcw (row-major, valid when flags & FOUND), inliers
 * (n bytes), ninliers, flags. */
int gf_pnp_iterate(gf_ctx* ctx, const float* p3d, const float* p2d, const float* sigma2, const float K[4],
                   gf_pnp_state* state, uint8_t* best_mask, int n_iterations, gf_rng* rng, float Tcw[16],
                   uint8_t* inliers, int32_t* ninliers, int32_t* flags);
/* Device batch: nprob independent solvers, problem b's correspondences at
 * [b][cap] of d_p3d/d_p2d/d_sigma2/d_best_mask/d_inliers, its size in
 * d_state[b].n; each problem draws from its own d_rng[b]. d_Tcw is [nprob][16].
 * max_iterations bounds every problem's loop count (the params value it was
 * initialised with); a problem whose loop it cuts short gets GF_PNP_TRUNCATED.
 * States are clamped on the device (min_set to 1..8, n to cap). */
int gf_pnp_iterate_dev(gf_ctx* ctx, int nprob, const float* d_p3d, const float* d_p2d, const float* d_sigma2,
                       int cap, const float K[4], gf_pnp_state* d_state, uint8_t* d_best_mask, int n_iterations,
                       int max_iterations, gf_rng* d_rng, float* d_Tcw, uint8_t* d_inliers, int32_t* d_ninliers,
                       int32_t* d_flags, void* stream);

/* ------------------------------------------------ loop-closure Sim3 solver
 * ORB_SLAM::Sim3Solver (src/Sim3Solver.cc, include/Sim3Solver.h): Horn's
 * closed-form absolute orientation on random three-point sets inside RANSAC;
 * LoopClosing::ComputeSim3 drives it (LoopClosing.cc:261-352:
 * SetRansacParameters(0.99,20,300), then iterate(5) per candidate keyframe,
 * round robin). A problem is the solver's correspondence list after the
 * constructor's filtering (:62-103), in that order: X1, X2 (n x 3, the matched
 * map points in camera 1 / camera 2 coordinates), sigma2_1, sigma2_2 (level
 * sigma^2 of the two keypoints), K1, K2 = (fx, fy, cx, cy). The keypoint-index
 * mapping (mvnIndices1) stays with the caller. */
typedef struct gf_sim3_params { /* SetRansacParameters arguments (:114) */
    double probability;
    int32_t min_inliers;
    int32_t max_iterations;
} gf_sim3_params;
typedef struct gf_sim3_state { /* one solver across iterate() calls */
    int32_t n;              /* N correspondences */
    int32_t min_inliers;    /* mRansacMinInliers */
    int32_t max_iterations; /* mRansacMaxIts after the adjustment (:125-135) */
    int32_t iterations;     /* mnIterations */
    int32_t best_inliers;   /* mnBestInliers */
    float best_scale;       /* mBestScale */
    float best_R[9];        /* mBestRotation, row-major */
    float best_t[3];        /* mBestTranslation */
    float best_T12[16];     /* mBestT12, row-major */
} gf_sim3_state;
#define GF_SIM3_FOUND 1     /* iterate returned a Sim3                         */
#define GF_SIM3_NOMORE 2    /* bNoMore                                         */
#define GF_SIM3_TRUNCATED 8 /* device path: max_iterations cut the call's loop short */
/* Sim3Solver::SetRansacParameters (host scalar set-up) into a fresh state:
 * iteration count 0, no best hypothesis. Where the reference converts a NaN or
 * out-of-range iteration estimate to int, max_iterations is taken. */
int gf_sim3_init(int n, const gf_sim3_params* params, gf_sim3_state* state);
/* Sim3Solver::iterate(nIterations, bNoMore, vbInliers, nInliers) (:140-207)
 * for one solver; rng is the process-wide std::rand() state the minimal sets
 * are drawn from (DUtils::Random::RandomInt, :168), advanced by three draws
 * per iteration run. best_mask (n bytes, mvbBestInliers) persists across calls
 * with the state; the best hypothesis is replaced on >=, so it can hold the
 * NaN transform of a degenerate set. Outputs: T12 (row-major, valid when
 * flags & FOUND, else zeros), inliers (n bytes, correspondence order),
 * ninliers, flags. */
int gf_sim3_iterate(gf_ctx* ctx, const float* X1, const float* X2, const float* sigma2_1, const float* sigma2_2,
                    const float K1[4], const float K2[4], gf_sim3_state* state, uint8_t* best_mask, int n_iterations,
                    gf_rng* rng, float T12[16], uint8_t* inliers, int32_t* ninliers, int32_t* flags);
/* Device batch: nprob independent solvers, problem b's correspondences at
 * [b][cap] of d_X1, d_X2, d_sigma2_1, d_sigma2_2, d_best_mask, d_inliers, its size in
 * d_state[b].n; each problem draws from its own d_rng[b]. d_T12 is [nprob][16].
 * max_iterations bounds the iterations of this call; a problem whose loop it
 * cuts short before a Sim3 is found gets GF_SIM3_TRUNCATED. States are clamped
 * on the device (n to cap). Asynchronous on `stream`. */
int gf_sim3_iterate_dev(gf_ctx* ctx, int nprob, const float* d_X1, const float* d_X2, const float* d_sigma2_1,
                        const float* d_sigma2_2, int cap, const float K1[4], const float K2[4],
                        gf_sim3_state* d_state, uint8_t* d_best_mask, int n_iterations, int max_iterations,
                        gf_rng* d_rng, float* d_T12, uint8_t* d_inliers, int32_t* d_ninliers, int32_t* d_flags,
                        void* stream);
/* ORBmatcher::SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th)
 * (ORBmatcher.cc:1841-2079) for one keyframe pair, host arrays: KF1's
 * unmatched map points are projected into KF2 with (sR21, t21), KF2's into KF1
 * with (sR12, t12); a pair of keypoints that chose each other becomes a match.
 * Both passes use fi's intrinsics, image bounds and scale factors (the
 * reference takes KF1's, :1844-1847). Per keyframe: Tcw (row-major 4x4), kps
 * (undistorted), desc (n x 32), n <= 4096, kf_mp (slot -> index into
 * mps/mp_desc/mp_bad, or -1: GetMapPointMatches). matches12 (n1, in and out)
 * holds map point indices of KF2's points, -1 = NULL; entries that come in set
 * are left as they are. GetIndexInKeyFrame(pKF2) of an incoming match is read
 * as the slot of kf_mp2 that holds it: a map point occurs at most once per
 * keyframe. KeyFrame::GetFeaturesInArea order decides ties (cell column outer,
 * row inner, keypoint index ascending in a cell). nfound: matches added. */
int gf_search_by_sim3(gf_ctx* ctx, const gf_frame_info* fi, const float* Tcw1, const gf_keypoint* kps1,
                      const uint8_t* desc1, int n1, const int32_t* kf_mp1, const float* Tcw2, const gf_keypoint* kps2,
                      const uint8_t* desc2, int n2, const int32_t* kf_mp2, const gf_map_point* mps,
                      const uint8_t* mp_desc, const uint8_t* mp_bad, int nmp, int32_t* matches12, float s12,
                      const float R12[9], const float t12[3], float th, int* nfound);
/* Optimizer::OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, th2)
 * (src/Optimizer.cc:2019-2215) for one keyframe pair, host arrays. A problem
 * is the routine's edge list after its own filtering (:2072-2111), in that
 * order, n pairs: X1 / X2 (n x 3) the matched map points in camera 1 / camera
 * 2 coordinates (Rcw*Xw + tcw in float), z1 / z2 (n x 2) the undistorted
 * keypoints of KF1 / KF2, w1 the information of EdgeSim3ProjectXYZ =
 * KF1's invSigma2[octave1], w2 the information of EdgeInverseSim3ProjectXYZ =
 * KF2's sigma2[octave2]: the reference calls GetSigma2, not GetInvSigma2, at
 * :2140, and that is kept. K1, K2 = (fx, fy, cx, cy). deltaHuber = sqrt(th2)
 * is taken in float (:2068). S12 (in and out) is the g2o::Sim3 estimate in the
 * order of its operator[]: qx qy qz qw tx ty tz s, in double; the quaternion
 * is Quaterniond(Matrix3d) of the solver's rotation and is not normalised by
 * any g2o::Sim3 operation. The Jacobians are BaseBinaryEdge's central
 * differences (core/base_binary_edge.hpp:147-196), the LM is the reference's
 * modified OptimizationAlgorithmLevenberg::solve
 * (core/optimization_algorithm_levenberg.cpp:61-164), the linear solve a 7x7
 * Eigen::LDLT. optimize(5); pairs with chi2(e12) > th2 || chi2(e21) > th2 are
 * dropped; with fewer than 10 left the routine returns 0 and S12 stays as it
 * came in; else optimize(nBad > 0 ? 10 : 5) and the same test again. The chi2
 * tested are those of the last LM trial evaluated (no computeError() before
 * chi2()), the rejected estimate's when that trial was popped. Outputs: inlier
 * (n bytes: 1 = vpMatches1 entry kept, 0 = cleared), nin (the return value),
 * stats (4 ints or NULL: iterations of the two rounds, LM trials of the two). */
int gf_optimize_sim3(gf_ctx* ctx, int n, const float* X1, const float* X2, const float* z1, const float* z2,
                     const float* w1, const float* w2, const float K1[4], const float K2[4], float th2, double S12[8],
                     uint8_t* inlier, int32_t* nin, int32_t* stats);
/* Device batch of Optimizer::OptimizeSim3 (src/Optimizer.cc:2019-2215), ragged:
 * problem p's pairs are rows [d_offsets[p], d_offsets[p + 1]) of the pair
 * arrays and of d_inlier; d_K is [nprob][8] (K1 then K2), d_th2 [nprob],
 * d_S12 [nprob][8] in and out, d_nin [nprob], d_stats [nprob][4] or NULL. One
 * wave per problem. Asynchronous on `stream`. Preconditions, as for the other
 * _dev entries: the buffers and `stream` belong to ctx's device, which is the
 * caller's current one; d_offsets is non-decreasing with d_offsets[0] >= 0 and
 * d_offsets[nprob] within the pair arrays. The offsets live on the device and
 * are not read back: a decreasing step is run as an empty problem, nothing
 * else is checked. */
int gf_optimize_sim3_dev(gf_ctx* ctx, int nprob, const float* d_X1, const float* d_X2, const float* d_z1,
                         const float* d_z2, const float* d_w1, const float* d_w2, const int32_t* d_offsets,
                         const float* d_K, const float* d_th2, double* d_S12, uint8_t* d_inlier, int32_t* d_nin,
                         int32_t* d_stats, void* stream);
/* ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th)
 * (src/ORBmatcher.cc:855-977), the search LoopClosing::ComputeSim3 runs over
 * the loop map points once a candidate is accepted (LoopClosing.cc:385), host
 * arrays. Scw is the row-major 4x4 similarity (sR | t), decomposed as at
 * :866-871. kps / desc (n <= 4096) are the keyframe's undistorted keypoints
 * and descriptors; points (npoints map point ids into mps / mp_desc / mp_bad)
 * is vpPoints in list order; matched (n, in and out) is vpMatched as map point
 * ids, -1 = NULL. Points named in matched at entry are skipped (the set is
 * built once, :874). vpMatched[bestIdx] is written inside the candidate loop,
 * so a keypoint taken by an earlier candidate is gone for the later ones: the
 * result equals the serial list-order result. KeyFrame::GetFeaturesInArea
 * order decides ties. nmatches: matches added. */
int gf_search_kf_sim3_projection(gf_ctx* ctx, const gf_frame_info* fi, const float Scw[16], const gf_keypoint* kps,
                                 const uint8_t* desc, int n, const gf_map_point* mps, const uint8_t* mp_desc,
                                 const uint8_t* mp_bad, int nmp, const int32_t* points, int npoints, int32_t* matched,
                                 int th, int* nmatches);
/* ORBmatcher::Fuse(KeyFrame* pKF, cv::Mat Scw, vpPoints, th)
 * (src/ORBmatcher.cc:1710-1839) up to the choice of bestIdx (:1816), the
 * search LoopClosing::SearchAndFuse (src/LoopClosing.cc:572-585) runs for every
 * keyframe of CorrectedSim3. Host arrays, one keyframe, shaped like
 * gf_search_kf_sim3_projection: Scw is decomposed as at :1719-1723, points are
 * map point ids in list order, kf_mp[k] is the id at slot k or -1. A candidate
 * that isBad() or is a non-bad point of the slot table (spAlreadyFound, :1726,
 * :1739) is skipped. Result per candidate: kp = the keypoint with
 * bestDist <= TH_LOW after the exits of :1739-1816, else -1; dist = its
 * distance, else -1. KeyFrame::GetFeaturesInArea order decides ties. What
 * :1819-1833 does with kp depends on the live map (the occupant of the slot
 * may have been replaced by an earlier candidate) and is the caller's. */
typedef struct gf_fuse_sim3_result {
    int32_t kp, dist;
} gf_fuse_sim3_result;
int gf_fuse_sim3(gf_ctx* ctx, const gf_frame_info* fi, const float Scw[16], const gf_keypoint* kps, const uint8_t* desc,
                 int n, const int32_t* kf_mp, const gf_map_point* mps, const uint8_t* mp_desc, const uint8_t* mp_bad,
                 int nmp, const int32_t* points, int npoints, float th, gf_fuse_sim3_result* res);
/* Device family: the nprob (keyframe, candidate list) searches of one
 * SearchAndFuse in one launch. The problem array is host memory, copied at the
 * call; every pointer in it, and d_mps / d_mp_desc / d_mp_bad (nmp rows, shared
 * by all problems, d_mp_bad optional), is a device pointer. A long candidate
 * list is spread over several workgroups. Ids outside [0, nmp) give kp = -1. */
typedef struct gf_fuse_sim3_problem {
    float Scw[16];
    const gf_keypoint* kps;
    const uint8_t* desc;
    int32_t n;
    const int32_t* kf_mp;
    const int32_t* points;
    int32_t npoints;
    float th;
    gf_fuse_sim3_result* res;
} gf_fuse_sim3_problem;
int gf_fuse_sim3_dev(gf_ctx* ctx, const gf_frame_info* fi, int nprob, const gf_fuse_sim3_problem* probs,
                     const gf_map_point* d_mps, const uint8_t* d_mp_desc, const uint8_t* d_mp_bad, int nmp,
                     void* stream);

/* ------------------------------------------------ essential graph (loop correction)
 * Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:1768-2017), the 7-DoF
 * pose graph LoopClosing::CorrectLoop runs over every keyframe of the map
 * (LoopClosing.cc:556), and the point correction of CorrectLoop itself
 * (LoopClosing.cc:462-491). One problem is one map; every index is a position
 * in the keyframe list (Map::GetAllKeyFrames(), no bad keyframe), whose mnId
 * are kf_id, strictly increasing (culled ids are absent).
 *   covisibility: CSR rows in mvpOrderedConnectedKeyFrames order with their
 *     weights; GetCovisiblesByWeight(100) is a row's prefix with weight >= 100,
 *     GetWeight a lookup in the row (absent: 0);
 *   le_*: GetLoopEdges() as CSR; lc_*: the LoopConnections map, keys lc_key
 *     (nlc of them) with CSR rows lc_start / lc_nbr;
 *   corr_idx / corrected / noncorrected: the keys of CorrectedSim3 /
 *     NonCorrectedSim3 (the same key set) and their g2o::Sim3 as
 *     qx qy qz qw tx ty tz s in double;
 *   points: GetWorldPos(), isBad(), the reference keyframe (pt_ref, -1 leaves
 *     the point as it is) and pt_corrected_ref (>= 0 where mnCorrectedByKF ==
 *     pCurKF->mnId: mnCorrectedReference, used instead of pt_ref).
 * The edge set is :1832-1957 with the reference's std::set / std::map
 * iterations (pointer order) run in keyframe-id order (assumption A24); the
 * linear solve is a tile Cholesky in place of CHOLMOD (A25). The Levenberg
 * schedule is optimization_algorithm_levenberg.cpp:61-164 with
 * setUserLambdaInit(1e-16) and optimize(20); Jacobians are BaseBinaryEdge's
 * central differences (base_binary_edge.hpp:147-196). Poses are written back
 * as [R | t/s] (:1965-1983), points as correctedSwr.map(Srw.map(p))
 * (:1986-2016); MapPoint::UpdateNormalAndDepth is the caller's.
 * Limits: 2 <= nkf <= GF_ESSGRAPH_MAX_KF; the factor's tile envelope must fit
 * GF_ESSGRAPH_MAX_TILES 64x64 f64 tiles (GF_ERR_CAP otherwise). */
#define GF_ESSGRAPH_MAX_KF 4096
#define GF_ESSGRAPH_MAX_TILES 65536 /* 2 GiB of factor */
#define GF_ESSGRAPH_TRACE 200
typedef struct gf_essgraph_problem {
    int32_t nkf, npts, ncorr, nlc;
    int32_t loop_kf, cur_kf;          /* pLoopKF (the fixed vertex), pCurKF */
    const int32_t* kf_id;             /* nkf */
    const float* kf_Tcw;              /* nkf x 16, row-major GetPose() */
    const int32_t* parent;            /* nkf, -1 = none */
    const int32_t* cov_start;         /* nkf + 1 */
    const int32_t* cov_nbr;
    const int32_t* cov_weight;
    const int32_t* le_start;          /* nkf + 1 */
    const int32_t* le_nbr;
    const int32_t* lc_key;            /* nlc */
    const int32_t* lc_start;          /* nlc + 1 */
    const int32_t* lc_nbr;
    const int32_t* corr_idx;          /* ncorr */
    const double* corrected;          /* ncorr x 8 */
    const double* noncorrected;       /* ncorr x 8 */
    const float* pt_pos;              /* npts x 3 */
    const uint8_t* pt_bad;            /* npts */
    const int32_t* pt_ref;            /* npts */
    const int32_t* pt_corrected_ref;  /* npts */
} gf_essgraph_problem;

/* stop: 0 = optimize(20) ran out, 1 = rho == 0, 2 = 10 trials failed, 3 = the
 * _nBad >= 3 rule (optimization_algorithm_levenberg.cpp:151-161). */
typedef struct gf_essgraph_stats {
    int32_t iterations, trials, stop, ntrace;
    double chi2_initial, chi2_final;
} gf_essgraph_stats;

typedef struct gf_essgraph_result {
    float* kf_Tcw;             /* nkf x 16 */
    float* pt_pos;             /* npts x 3 */
    gf_essgraph_stats stats;
    double* trace_lambda;      /* GF_ESSGRAPH_TRACE or NULL: lambda of each trial */
    double* trace_chi2;        /* GF_ESSGRAPH_TRACE or NULL: tempChi */
    uint8_t* trace_accepted;   /* GF_ESSGRAPH_TRACE or NULL */
} gf_essgraph_result;

typedef struct gf_essgraph_plan gf_essgraph_plan;

/* Validates nprob maps (a ragged batch), builds each edge set, Hessian index
 * (rank by id among the free keyframes, as initializeOptimization gives), the
 * gather lists of the 7x7 blocks and the tile envelope on the host, and
 * uploads them. nkf < 2, an unsorted kf_id, an index out of range or nkf above
 * the cap: GF_ERR_ARG, checked before any device work. */
int gf_essgraph_plan_create(gf_ctx* ctx, int nprob, const gf_essgraph_problem* probs, gf_essgraph_plan** out);
/* The edge rows (i, j, kind) of problem p in insertion order (Optimizer.cc:
 * 1832-1957): vertex 0 = i, vertex 1 = j, kind 0 loop connection, 1 spanning
 * tree, 2 past loop edge, 3 covisibility. rows NULL: only *nedges. */
int gf_essgraph_plan_edges(gf_essgraph_plan* plan, int p, int32_t* rows, int cap, int* nedges);
/* optimize(20) of every problem from its uploaded state (:1959-1962) and the
 * write-back (:1964-2016), on `stream`; the host reads three scalars back per
 * Levenberg trial. Solving twice gives identical bytes. */
int gf_essgraph_plan_solve(gf_essgraph_plan* plan, void* stream);
int gf_essgraph_plan_results(gf_essgraph_plan* plan, gf_essgraph_result* res);
int gf_essgraph_plan_destroy(gf_essgraph_plan* plan);
/* Optimizer::OptimizeEssentialGraph (Optimizer.cc:1768-2017) of one map. */
int gf_optimize_essential_graph(gf_ctx* ctx, const gf_essgraph_problem* prob, gf_essgraph_result* res);
/* The point loop of LoopClosing::CorrectLoop (LoopClosing.cc:462-491): point m
 * with sel[m] = c >= 0 becomes to[c].inverse().map(from[c].map(pos[m])) in
 * double, stored as float; bad points and sel < 0 are copied through. from /
 * to: nsim x 8 g2o::Sim3 (NonCorrectedSim3 / CorrectedSim3 rows). */
int gf_correct_loop_points(gf_ctx* ctx, int npts, const float* pos, const uint8_t* bad, const int32_t* sel, int nsim,
                           const double* from, const double* to, float* pos_out);

/* ------------------------------------------------ loop detection (LoopClosing::DetectLoop)
 * gf_loopdb: the keyframe database of loop closing (KeyFrameDatabase.cc:32-196)
 * as BowVectors resident on the device in CSR form (words int32 ascending,
 * values double). A keyframe is a slot: gf_loopdb_insert stores its BowVector
 * (0 to 4096 words) without listing it -- keyframe 0 never enters the file
 * (LoopClosing.cc:98-103) yet is scored for minScore (:132-146) -- and
 * returns the slot, numbered from 0 in insert order. Storage grows by doubling;
 * no query uploads the database. Each slot carries an add sequence number, -1
 * while the keyframe is not in the inverted file:
 *   gf_loopdb_add    KeyFrameDatabase::add (:39-45): the next sequence number;
 *                    adding a listed slot is GF_ERR_ARG.
 *   gf_loopdb_erase  KeyFrameDatabase::erase (:47-66): back to -1; a later add
 *                    puts the keyframe at the back of its words' lists.
 *   gf_loopdb_clear  KeyFrameDatabase::clear (:68-72): every slot unlisted, the
 *                    sequence restarts; the stored vectors and slots remain.
 * The calls of one database run on its context's stream. gf_loopdb_insert_dev
 * takes frame `frame` of the arrays gf_bow_transform_dev writes (d_words /
 * d_values strided by cap, d_nwords per frame) on `stream` without a host
 * synchronisation; the slot reserves cap entries. It orders the two streams
 * itself with an event in both directions: its copies wait for the work the
 * context's stream already holds, and the context's later work waits for
 * them. Its input stays on the device, so it is not validated as
 * gf_loopdb_insert's is: the words must ascend, be >= 0 and < INT_MAX, and
 * d_nwords[frame] is clamped to [0, cap].
 * gf_bow_score: TemplatedVocabulary::score = L1Scoring::score
 *   (TemplatedVocabulary.h:1213-1217, ScoringObject.cpp:23-68) of two
 *   BowVectors, host only, in double: the common words' terms fabs(vi - wi) -
 *   fabs(vi) - fabs(wi) added in ascending word order, then -score / 2.0.
 *   scoring = the vocabulary's ScoringType; other than L1_NORM (0):
 *   GF_ERR_UNSUPPORTED.
 * gf_loopdb_scores: that score on the device, query_slot's vector against each
 *   of slots[0..n) (listed or not), cast to float as LoopClosing.cc:142 does.
 * gf_detect_loop_candidates: KeyFrameDatabase::DetectLoopCandidates(pKF,
 *   minScore) (:75-196) for the keyframe in query_slot. connected = the slots
 *   of pKF->GetConnectedKeyFrames(); cov_off ([nslots + 1]) / cov =
 *   mvpOrderedConnectedKeyFrames per slot as gf_reloc_candidates takes them,
 *   of which GetBestCovisibilityKeyFrames(10) reads the first ten.
 *   words_out[nslots] = mnLoopWords (0 for slots that are unlisted, connected
 *   or share no word), score_out[nslots] = mLoopScore, valid where words_out >
 *   *min_common (= minCommonWords; 0 when nothing shares a word). cands (room
 *   for nslots) / ncand = the returned vector, in the reference's order. */
typedef struct gf_loopdb gf_loopdb;
int gf_loopdb_create(gf_ctx* ctx, gf_loopdb** out);
int gf_loopdb_destroy(gf_loopdb* db);
int gf_loopdb_size(gf_loopdb* db, int* nslots, int* nlisted);
int gf_loopdb_clear(gf_loopdb* db);
int gf_loopdb_insert(gf_loopdb* db, const int32_t* words, const double* values, int n, int* slot);
int gf_loopdb_insert_dev(gf_loopdb* db, const int32_t* d_words, const double* d_values, const int32_t* d_nwords,
                         int cap, int frame, void* stream, int* slot);
int gf_loopdb_add(gf_loopdb* db, int slot);
int gf_loopdb_erase(gf_loopdb* db, int slot);
int gf_bow_score(int scoring, const int32_t* w1, const double* v1, int n1, const int32_t* w2, const double* v2, int n2,
                 double* score);
int gf_loopdb_scores(gf_loopdb* db, int query_slot, const int32_t* slots, int n, float* out);
int gf_detect_loop_candidates(gf_loopdb* db, int query_slot, const int32_t* connected, int nconn,
                              const int32_t* cov_off, const int32_t* cov, float min_score, int32_t* words_out,
                              float* score_out, int* min_common, int32_t* cands, int* ncand);

/* ------------------------------------------------ monocular initialisation
 * ORB_SLAM::Initializer (src/Initializer.cc, include/Initializer.h):
 * Initializer(ReferenceFrame, sigma, iterations) + Initialize(CurrentFrame,
 * vMatches12, R21, t21, vP3D, vbTriangulated) (:44-132), called by
 * Tracking::MonocularInitialization with sigma 1.0 and 200 iterations; the
 * reference passes minTriangulated = THRES_INIT_MPT_NUM / 2 = 50. Frame 1 is
 * the reference frame (mvKeys1 = its undistorted keypoints), frame 2 the
 * current one; matches12[i] (n1 entries) is the frame-2 keypoint matched to
 * keypoint i of frame 1 or -1. The 8-point sets are drawn from rng (the
 * process-wide std::rand() state, DUtils::Random::RandomInt), which advances
 * by 8 * iterations draws. Outputs p3d (n1 x 3) and triangulated (n1) are
 * vP3D / vbTriangulated when ok, zeros otherwise. */
typedef struct gf_init_result {
    int32_t ok;         /* Initialize() returned true: R21, t21, p3d, triangulated valid      */
    int32_t model;      /* 0 homography (RH > 0.40), 1 fundamental, -1 neither search scored  */
    int32_t nmatches;   /* N = entries of matches12 >= 0                                       */
    int32_t iter_H;     /* RANSAC iteration of the kept H (first strict best), -1 none         */
    int32_t iter_F;     /* same for F                                                          */
    int32_t ninliers_H; /* vbMatchesInliersH count                                             */
    int32_t ninliers_F; /* vbMatchesInliersF count                                             */
    int32_t best;       /* motion hypothesis with the most nGood (0..7 H, 0..3 F), -1 none     */
    int32_t ngood[8];   /* CheckRT nGood of each motion hypothesis                             */
    float SH, SF, RH;   /* scores and ratio (RH = 0 when both scores are 0)                    */
    float parallax;     /* parallax (degrees) of hypothesis `best`                             */
    float H21[9], F21[9]; /* kept models, row-major (zeros when none)                          */
    float R21[9], t21[3]; /* accepted motion, row-major                                        */
} gf_init_result;
/* Host family: uploads, runs the device path, downloads. GF_ERR_ARG when a
 * match index is >= n2 or fewer than 8 matches exist (nothing runs then). */
int gf_initialize(gf_ctx* ctx, const float K[9], float sigma, int iterations, int min_triangulated,
                  const gf_keypoint* kps1, int n1, const gf_keypoint* kps2, int n2, const int32_t* matches12,
                  gf_rng* rng, gf_init_result* result, float* p3d, uint8_t* triangulated);
/* Device family: all buffers in device memory; the caller guarantees the
 * match indices are < n2. With fewer than 8 matches the result reports
 * model -1 and nmatches, and rng is left as it was. */
int gf_initialize_dev(gf_ctx* ctx, const float K[9], float sigma, int iterations, int min_triangulated,
                      const gf_keypoint* d_kps1, int n1, const gf_keypoint* d_kps2, int n2,
                      const int32_t* d_matches12, gf_rng* d_rng, gf_init_result* d_result, float* d_p3d,
                      uint8_t* d_triangulated, void* stream);
/* Device batch: nprob independent initialisations in one launch set (e.g. every
 * sequence of a multi-sequence tracker at start-up). Problem p's reference /
 * current keypoints at [p][cap1] / [p][cap2] with d_n1[p] / d_n2[p] valid
 * (clamped to the caps), matches12 [p][cap1], rng [p], result [p], p3d
 * [p][cap1][3], triangulated [p][cap1]. Same per-problem results as
 * gf_initialize_dev. */
int gf_initialize_batch_dev(gf_ctx* ctx, int nprob, const float K[9], float sigma, int iterations,
                            int min_triangulated, const gf_keypoint* d_kps1, int cap1, const int32_t* d_n1,
                            const gf_keypoint* d_kps2, int cap2, const int32_t* d_n2, const int32_t* d_matches12,
                            gf_rng* d_rng, gf_init_result* d_result, float* d_p3d, uint8_t* d_triangulated,
                            void* stream);

/* ------------------------------------------------ the initial map
 * Tracking::CreateInitialMap (src/Tracking.cc:1199-1322) behind the filter of
 * Tracking::Initialize (:1126-1133), as two batched device stages around the
 * bundle adjustment (gf_ba_plan_create_iters with 20 iterations, :1263). The
 * inputs are laid out as gf_initialize_batch_dev lays them out, [P][cap...]
 * with per-problem counts (clamped to the caps); a frame holds at most 4096
 * keypoints. Descriptors are 32 bytes a row and 4-byte aligned. KFcur's pose
 * is [R21 | t21] as the initialiser returned them (the motion-prior rescale of
 * :1139 belongs to Tracking::Initialize's bookkeeping and is not applied). */
enum {
    GF_IM_OK = 0,
    GF_IM_NOT_INITIALIZED = 1, /* the initialiser's record says ok == 0: no map, nothing to reset */
    GF_IM_RESET_DEPTH = 2,     /* medianDepth < 0: the reference calls Reset() (:1269) */
    GF_IM_RESET_FEW = 3        /* TrackedMapPoints() < THRES_INIT_MPT_NUM, or no point at all */
};

typedef struct gf_initmap_in { /* device pointers */
    const gf_keypoint* kps1;     /* [P][cap1] KFini's undistorted keypoints            */
    const uint8_t* desc1;        /* [P][cap1][32]                                      */
    const int32_t* n1;           /* [P]                                                */
    const gf_keypoint* kps2;     /* [P][cap2] KFcur's                                  */
    const uint8_t* desc2;        /* [P][cap2][32]                                      */
    const int32_t* n2;           /* [P]                                                */
    const int32_t* matches12;    /* [P][cap1] mvIniMatches before the filter           */
    const gf_init_result* init;  /* [P] the initialiser's records                      */
    const float* p3d;            /* [P][cap1][3] mvIniP3D                              */
    const uint8_t* triangulated; /* [P][cap1] vbTriangulated                           */
    int32_t cap1, cap2;
} gf_initmap_in;

/* What gf_initial_map_points_dev writes (device pointers). The last nine
 * arrays are problem p's gf_ba_problem in the orders that struct demands:
 * nkf = 2, npts = npts[p], nedges = 2 npts[p]. */
typedef struct gf_initmap_points {
    int32_t* status;        /* [P] GF_IM_OK or GF_IM_NOT_INITIALIZED                         */
    int32_t* npts;          /* [P]                                                           */
    int32_t* pt_kp;         /* [P][cap1][2] the observations: keypoint in KFini, in KFcur    */
    gf_map_point* mps;      /* [P][cap1]                                                     */
    uint8_t* mp_desc;       /* [P][cap1][32]                                                 */
    int32_t* slots1;        /* [P][cap1] KFini's mvpMapPoints, -1 = NULL                     */
    int32_t* slots2;        /* [P][cap2] KFcur's                                             */
    float* kf_Tcw;          /* [P][2][16] KFini identity, KFcur [R21 | t21]                  */
    uint8_t* kf_kind;       /* [P][2] 1 (fixed, mnId 0), 0                                   */
    float* kf_cam;          /* [P][2][4]                                                     */
    float* pt_pos;          /* [P][cap1][3]                                                  */
    int32_t* edge_pt;       /* [P][2 cap1] edge 2j and 2j + 1: point j                       */
    int32_t* edge_kf;       /* [P][2 cap1] 0 (KFini), 1 (KFcur)                              */
    float* edge_z;          /* [P][2 cap1][2] the undistorted keypoint position              */
    float* edge_inv_sigma2; /* [P][2 cap1] GetInvSigma2(octave)                              */
} gf_initmap_points;

/* Stage 1 (:1126-1133, :1206-1249). A problem whose record says ok == 0 gets
 * zero points, empty slot tables and GF_IM_NOT_INITIALIZED. Otherwise the
 * matches with matches12[i] >= 0 && triangulated[i] (and matches12[i] <
 * n2[p]: the reference would index outside the frame) become the map points
 * 0..n-1 in increasing i. Per point: the keypoint pair; the position p3d[i];
 * the descriptor, ComputeDistinctiveDescriptors over two observations =
 * KFini's row (both medians are 0, the first observation wins); normal and
 * min / max distance by UpdateNormalAndDepth with mpRefKF = pKFcur (level =
 * the octave of the KFcur keypoint), KFini at identity and KFcur at [R21 |
 * t21], in the arithmetic of gf_update_normal_and_depth. Slot tables: when
 * two matches name the same KFcur keypoint the later i owns the slot, as
 * AddMapPoint overwrites; both points keep their observation. */
int gf_initial_map_points_dev(gf_ctx* ctx, const gf_frame_info* fi, int nprob, const gf_initmap_in* in,
                              const gf_initmap_points* out, void* stream);

typedef struct gf_initmap_report {
    int32_t status;        /* GF_IM_*                                                     */
    int32_t npts;          /* map points                                                  */
    int32_t tracked;       /* pKFcur->TrackedMapPoints(): its non-NULL slots               */
    int32_t ba_iterations; /* iterations of optimize(20), -1 = not run                    */
    float median_depth;    /* pKFini->ComputeSceneMedianDepth(2) before the scaling       */
    float Tcw[32];         /* KFini, KFcur: final poses, row-major 4x4 each               */
} gf_initmap_report;

/* Stage 2 (Optimizer.cc:125-140, Tracking.cc:1268-1299) from the solver's
 * output, read in place: d_ba_kf_Tcw[p] / d_ba_pt_pos[p] are device pointers
 * to problem p's optimised poses (2 x 16) and points (npts x 3), e.g. those
 * of gf_ba_plan_results_dev, d_ba_iterations[p] a device pointer to its
 * iteration count (the table may be NULL); the three tables themselves are
 * device arrays of nprob pointers. Every point gets
 * UpdateNormalAndDepth with the optimised pose and positions; the median
 * depth is the element (n - 1) / 2 of KFini's sorted depths z = (float)
 * (Rcw.row(2) . x + zcw), by an exact selection; status GF_IM_RESET_DEPTH
 * when it is < 0, else GF_IM_RESET_FEW when tracked < thres_init_mpt_num
 * (THRES_INIT_MPT_NUM, 100 in the reference) or when there is no point at all
 * (the reference indexes an empty vector there). On GF_IM_OK KFcur's
 * translation and every point position are multiplied by invMedianDepth =
 * 1.0f / median in float. The normals and the min / max distances are NOT
 * recomputed after the scaling: they stay those of the unscaled result, as
 * in the reference. On a reset status poses and points are the unscaled
 * solver output. A GF_IM_NOT_INITIALIZED problem passes through (its BA
 * pointers are not read). d_mps: [P][cap1] rows out. */
int gf_initial_map_finish_dev(gf_ctx* ctx, const gf_frame_info* fi, int nprob, const gf_initmap_in* in,
                              const gf_initmap_points* pts, const float* const* d_ba_kf_Tcw,
                              const float* const* d_ba_pt_pos, const int32_t* const* d_ba_iterations,
                              int thres_init_mpt_num,
                              gf_initmap_report* d_report, gf_map_point* d_mps, void* stream);

/* ------------------------------------------------ the matches of the initialiser
 * ORBmatcher::SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12,
 * windowSize) (src/ORBmatcher.cc:1172-1287) over Frame::GetFeaturesInArea
 * (src/Frame.cc:300-365) and the grid of Frame.cc:100-131, :367-377, as
 * Tracking::Initialize calls it (src/Tracking.cc:1007-1008: ORBmatcher(0.9,
 * true), window SRH_WINDOW_SIZE_INIT = 100). Frame 1 is the initial frame,
 * frame 2 the current one; keypoints are the undistorted ones, octaves >= 0.
 * Only the level-0 keypoints of both frames take part. prev_matched [n1][2]
 * is vbPrevMatched: the window of query i is centred on prev_matched[i], and
 * at the end every surviving match writes its frame-2 position there; other
 * entries keep their value. matches12 [n1]: the frame-2 keypoint of query i
 * or -1; nmatches: the reference's return value. Accept: best distance <= 50
 * (TH_LOW) and best < (float)second * nnratio, first candidate in walk order
 * on ties; a later accept of the same frame-2 keypoint steals it; with
 * check_ori the rotation histogram counts every accept, also of queries robbed
 * later (ComputeThreeMaxima, :2338-2379).
 * flags: GF_SI_DIRECT makes every query walk its window inside the ordered
 * pass with the distances computed in place, instead of reading the candidate
 * list that a parallel pass stored; a query with more than 64 level-0
 * candidates in its window does that in either mode. Same results. */
enum { GF_SI_DIRECT = 1 };
/* Host family: uploads, runs the device path, downloads. */
int gf_search_for_initialization(gf_ctx* ctx, const gf_frame_info* fi, const gf_keypoint* kps1, const uint8_t* desc1,
                                 int n1, const gf_keypoint* kps2, const uint8_t* desc2, int n2, int window,
                                 float nnratio, int check_ori, int flags, float* prev_matched, int32_t* matches12,
                                 int* nmatches);
/* Device batch, laid out as gf_initialize_batch_dev lays its problems out:
 * problem p's frames at [p][cap1] / [p][cap2] (descriptor rows 32 bytes,
 * 16-byte aligned), d_n1[p] / d_n2[p] valid (clamped to the caps, 1 <= cap <=
 * 4096), d_prev_matched [P][cap1][2] in / out, d_matches12 [P][cap1] (-1 past
 * n1), d_nmatches [P]. Asynchronous on stream; the grid and the candidate
 * lists (256 bytes per frame-1 row) live in the context's scratch. */
int gf_search_for_initialization_batch_dev(gf_ctx* ctx, const gf_frame_info* fi, int nprob, const gf_keypoint* d_kps1,
                                           const uint8_t* d_desc1, int cap1, const int32_t* d_n1,
                                           const gf_keypoint* d_kps2, const uint8_t* d_desc2, int cap2,
                                           const int32_t* d_n2, int window, float nnratio, int check_ori, int flags,
                                           float* d_prev_matched, int32_t* d_matches12, int32_t* d_nmatches,
                                           void* stream);
/* The gate of Tracking::Initialize (src/Tracking.cc:999-1017) per problem,
 * after the matcher has run on every problem of the batch. thres is
 * THRES_INIT_MPT_NUM (100 in the reference).
 *   GF_SI_FEW_KEYPOINTS  d_n2[p] <= thres: the reference returns before the
 *     matcher, so d_matches12[p] becomes all -1 (:1001), d_prev_matched[p] is
 *     restored from d_prev_before[p] (the caller's copy from before the
 *     matcher) and d_nmatches[p] = 0; the tracker goes to NOT_INITIALIZED;
 *   GF_SI_FEW_MATCHES    d_nmatches[p] < thres: d_matches12 and
 *     d_prev_matched stay as the matcher left them; NOT_INITIALIZED;
 *   GF_SI_OK             the initialiser runs.
 * d_init_matches12 [P][cap1] is what the initialiser is to see: a copy of
 * d_matches12 on GF_SI_OK, all -1 otherwise, so that gf_initialize_batch_dev
 * reports ok == 0 for that problem and leaves its rand() state untouched, as
 * the reference does not call Initializer::Initialize there. */
enum { GF_SI_OK = 0, GF_SI_FEW_KEYPOINTS = 1, GF_SI_FEW_MATCHES = 2 };
int gf_tracking_initialize_gate_dev(gf_ctx* ctx, int nprob, const int32_t* d_n2, int cap1, int thres,
                                    const float* d_prev_before, float* d_prev_matched, int32_t* d_matches12,
                                    int32_t* d_nmatches, int32_t* d_status, int32_t* d_init_matches12, void* stream);

/* ------------------------------------------------ tracking glue (device)
 * Per-frame bookkeeping of Tracking between the stages above, so a front-end
 * step stays on the device. One workgroup per frame.
 * gf_motion_predict_dev: Tcw = velocity * Tcw_last (Tracking.cc:1511).
 * gf_discard_outliers_dev: kp2mp = -1, outlier = 0 for flagged matches
 *   (Tracking.cc:1550-1563); nmatches = remaining, num_to_match = budget -
 *   nmatches (Tracking.cc:3228). Either output may be NULL.
 * gf_matched_gather_dev: keypoint-ordered compaction of the matched points:
 *   pos (map position), sigma2 (level sigma^2 of the octave), idx (keypoint),
 *   n per frame; the FRAME_INFO_MATRIX input (Observability.cc:386-520).
 * gf_views_exclude_matched_dev: views[kp2mp].in_view = 0, i.e.
 *   mbTrackInView = false for points already matched (Tracking.cc:3205). */
int gf_motion_predict_dev(gf_ctx* ctx, int nframes, const float* d_velocity, const float* d_Tcw_last, float* d_Tcw,
                          void* stream);
int gf_discard_outliers_dev(gf_ctx* ctx, int nframes, int32_t* d_kp2mp, uint8_t* d_outlier, const int32_t* d_nkps,
                            int kp_stride, int budget, int32_t* d_nmatches, int32_t* d_num_to_match, void* stream);
int gf_matched_gather_dev(gf_ctx* ctx, int nframes, const gf_keypoint* d_kps, const int32_t* d_nkps, int kp_stride,
                          const int32_t* d_kp2mp, const gf_map_point* d_map, int map_stride,
                          const float* level_sigma2, int nlevels, float* d_pos, float* d_sigma2, int32_t* d_idx,
                          int32_t* d_n, void* stream);
int gf_views_exclude_matched_dev(gf_ctx* ctx, int nframes, const int32_t* d_kp2mp, const int32_t* d_nkps,
                                 int kp_stride, gf_mp_view* d_views, const int32_t* d_nmp, int mp_stride,
                                 void* stream);

/* ------------------------------------------------ batched tracking front end
 * Tracking::GrabImage in the WORKING state (Tracking.cc:461-917) for B
 * independent sequences ("streams"), every frame of every stream on the
 * device, no host round trip inside a step:
 *   Frame (ORB extraction, E1-E8)
 *   TrackWithMotionModel (Tracking.cc:1506-1642): Tcw = V * Tlast, M3
 *     SearchByProjection(Cur, Last, 15), PoseOptimization, discard outliers
 *   TrackLocalMap (:2732-2844) with SearchReferencePointsInFrustum
 *     (:3149-3410): updatePWLSVec, FRAME_INFO_MATRIX, mCurrentInfoMat; then
 *     num_to_match <= 0: mLeftMapPoints = in-view (stale mbTrackInView)
 *       local points, mbNeedVizCheck;
 *     else isInFrustum; nToMatch < 400: SearchByProjection(F, local, 1);
 *       else MAP_INFO_MATRIX + runActiveMapMatching (leftovers = unmatched
 *       pool); PoseOptimization (outliers kept, :2776)
 *   motion model update V = Tcw * LastTwc (:729-738), updatePWLSVec +
 *     predictPWLSVec(dt, 2), RunMapPointsSelection's MAP_INFO_MATRIX at
 *     kinematic[1] (:1717-1779), SearchAdditionalMatchesInFrame
 *     (:3097-3145: isInFrustum when mbNeedVizCheck, SearchByProjection_Budget
 *     th 0.8), outliers set NULL, mLastFrame = Frame(mCurrentFrame) (:901-910).
 * The local map (UpdateReference, :3689-3852) is the map set with
 * gf_frontend_set_map, in that order. Keyframe insertion
 * (NeedNewKeyFrame / CreateNewKeyFrame, :896-897) is a stage of the step once
 * gf_frontend_set_keyframes switched it on; local mapping takes the keyframes
 * from its outbox (gf_frontend_take_keyframes) and runs outside the path. The
 * tracking state machine of GrabImage
 * (:602-644, 652-716, 854-911) runs per stream (GF_FE_TRACK):
 *   WORKING with a velocity and >= 2 frames since a relocalisation:
 *     TrackWithMotionModel; it fails on < 20 matches (:1559) or < 10 after
 *     the outlier discard (:1641), and TrackPreviousFrame (:1325-1404) runs;
 *   WORKING otherwise: TrackPreviousFrame (WindowSearch 200 from the upper
 *     half of the pyramid, then 100 at any level, PoseOptimization,
 *     SearchByProjection(Last, Cur, 15 or 50), PoseOptimization);
 *   LOST: Relocalisation (:3854-4031) against the stream's keyframe
 *     database (gf_frontend_set_kfdb; none: the frame stays LOST):
 *     ComputeBoW, DetectRelocalisationCandidates, SearchByBoW(0.75) per
 *     candidate (>= 15), P4P RANSAC iterate(5) rounds over the candidates
 *     (0.99, 10, 300, 4, 0.5, 5.991) with PoseOptimization and the
 *     SearchByProjection(F, KF, found, 10 / 3, 100 / 64) refinements, until
 *     one pose keeps >= 50 inliers.
 *   A frame whose initial estimate succeeded runs TrackLocalMap (the
 *   SearchByProjection window is 5 and FRAME_INFO_MATRIX is skipped for two
 *   frames after a relocalisation, :3162, :3318-3320); it fails on < 25
 *   inliers within mMaxFrames of a relocalisation or < 15 (:2819-2824). A
 *   failed frame sets LOST, clears the velocity and skips the post-publish
 *   block: mLastFrame stays the last tracked frame.
 * Assumed of the map: >= 6 keyframes (KeyFramesInMap() >= 4 for the motion
 * model, > 5 for WindowSearch's octave floor; the keyframe graph's count when
 * one is set) and frames past the initial TIME_INIT_TRACKING window.
 * updateAtFrameId stamps are stored relative to the current frame
 * (the frame being tracked is 1, the next 2; every step shifts them by -1),
 * so a step has no per-frame host argument and can be replayed as a HIP
 * graph. Time budgets follow gf_set_budgets of the context (+inf = parity). */
typedef struct gf_frontend_params {
    int32_t width, height;
    float fx, fy, cx, cy;       /* Camera.fx/fy/cx/cy                             */
    int32_t nfeatures;          /* ORBextractor.nFeatures */
    float scale_factor;         /* ORBextractor.scaleFactor */
    int32_t nlevels;            /* ORBextractor.nLevels */
    int32_t fast_th;            /* ORBextractor.fastTh */
    int32_t batch;              /* streams B */
    int32_t map_cap;            /* local-map capacity per stream (<= 4096) */
    int32_t gf_budget;          /* num_good_inlier_predef (main.cc GF budget) */
    int32_t gf;                 /* 1 GOOD_FEATURE_MAP_MATCHING, 0 ORB-SLAM baseline matching */
    double dt;                  /* frame period 1 / Camera.fps (timestamps t_k = t_0 + k dt) */
    float dist[5];              /* Camera.k1 k2 p1 p2 [k3] (mDistCoef). k1 != 0: every
                                   frame's keypoints are undistorted after extraction
                                   (Frame::UndistortKeyPoints, Frame.cc:389-423) and the
                                   image bounds mnMinX..mnMaxY come from the undistorted
                                   corners and edge midpoints (Frame.cc:425-493); they
                                   set the projection bounds, the keypoint grid and the
                                   observability margins (Tracking.cc:876-877).
                                   k1 == 0: keypoints as extracted, bounds = the image. */
    int32_t max_frames;         /* mMaxFrames = 18 * Camera.fps / 30 (Tracking.cc:153), the
                                   window of TrackLocalMap's stricter inlier rule after a
                                   relocalisation; 0: derived from dt */
    int32_t harris_score;       /* 1: ORBextractor.nScoreType = HARRIS_SCORE (0; Tracking.cc:186),
                                   0: FAST_SCORE (1, the settings' default) */
} gf_frontend_params;
typedef struct gf_frontend gf_frontend;

// Extraction gate for several front ends sharing one GPU: before its
// extraction kernels a step waits for `wait_event` (a hipEvent_t; NULL: no
// wait), after them it records `done_event` (NULL: none). Chaining front end
// g's done event into front end g+1's wait event serialises the
// bandwidth-bound extraction stages while each front end's tracking kernels
// overlap the next one's extraction. Events stay owned by the caller.
// A gated front end cannot be captured as a graph (gf_frontend_capture
// refuses), nor can a captured one be gated.
int gf_frontend_set_gate(gf_frontend* fe, void* wait_event, void* done_event);
// The extraction stage after which the gate's done event is recorded: 0
// resize, 1 blur + FAST map, 2 cells, 3 select, 4 describe (the default, the
// whole extraction). An earlier stage lets the next front end's extraction
// start sooner (overlapping this one's later stages).
int gf_frontend_set_gate_stage(gf_frontend* fe, int stage);
// Tracking stream: the step's kernels after extraction run on a stream of
// their own created with HIP stream priority `priority` (clamped to the
// device's range; lower = more urgent), forked from and joined back into the
// context's stream each step, so results and ordering are unchanged. With
// several front ends on one GPU a high priority lets one front end's
// latency-bound tracking kernels take compute units ahead of another's
// extraction kernels. Once per front end; not with gf_frontend_capture. The
// tracking kernels use the context's scratch slots, so the front end must be
// the only one on its context (GF_ERR_ARG otherwise, and gf_frontend_create
// then refuses a second front end on that context).
int gf_frontend_set_track_priority(gf_frontend* fe, int priority);
// A hipEvent_t (timing disabled) on the context's device, for the gate.
int gf_event_create(gf_ctx* ctx, void** event_out);
int gf_event_destroy(void* event);

/* Per-stream state and outputs, readable / writable as whole-batch arrays. */
enum {
    GF_FE_KPS = 0,      /* [B][cap] gf_keypoint  mCurrentFrame.mvKeysUn      */
    GF_FE_DESC,         /* [B][cap][32] u8       mDescriptors               */
    GF_FE_NKP,          /* [B] i32               N                          */
    GF_FE_TCW,          /* [B][16] f32           mTcw                       */
    GF_FE_KP2MP,        /* [B][cap] i32          mvpMapPoints (map index)   */
    GF_FE_SCORE,        /* [B][cap] i32          mvpMatchScore              */
    GF_FE_OUTLIER,      /* [B][cap] u8           mvbOutlier                 */
    GF_FE_LAST_KPS,     /* mLastFrame: as the four above                    */
    GF_FE_LAST_DESC,
    GF_FE_LAST_NKP,
    GF_FE_LAST_KP2MP,
    GF_FE_LAST_OUTLIER, /* [B][cap] u8                                      */
    GF_FE_LAST_POS,     /* [B][cap][3] f32 world position of each last MP  */
    GF_FE_TCW_LAST,     /* [B][16] f32 mLastFrame.mTcw                      */
    GF_FE_VELOCITY,     /* [B][16] f32 mVelocity                            */
    GF_FE_T_PREV,       /* [B] f64 mLastFrame.mTimeStamp                    */
    GF_FE_T_CUR,        /* [B] f64 mCurrentFrame.mTimeStamp                 */
    GF_FE_MAP,          /* [B][M] gf_map_point                              */
    GF_FE_MAP_DESC,     /* [B][M][32] u8                                    */
    GF_FE_NMP,          /* [B] i32                                          */
    GF_FE_VIEWS,        /* [B][M] gf_mp_view (mbTrackInView & projection)   */
    GF_FE_XV,           /* [B][13] f64 kinematic[0].Xv                      */
    GF_FE_XV_NEXT,      /* [B][13] f64 kinematic[1].Xv                      */
    GF_FE_BASE,         /* [B][49] f64 mCurrentInfoMat                      */
    GF_FE_MP_H,         /* [B][M][14] f64 MapPoint::H_meas                  */
    GF_FE_MP_INFO,      /* [B][M][49] f64 MapPoint::ObsMat                  */
    GF_FE_MP_UV,        /* [B][M][2] f32 u_proj, v_proj                     */
    GF_FE_MP_UPD,       /* [B][M] i32 updateAtFrameId (relative stamps)     */
    GF_FE_RNG,          /* [B] gf_rng std::rand() state per stream          */
    GF_FE_LEFT,         /* [B][M] i32 mLeftMapPoints of the last step       */
    GF_FE_STATS,        /* [GF_FE_NSTAT][B] i32, see GF_ST_*                */
    GF_FE_HIST,         /* [B][8] i32 running counters since the last write:
                           [0..4] steps per GF_ST_BRANCH value, [5] steps in
                           which a time cap fired, [6] logDet evaluations,
                           [7] local-map search matches                      */
    GF_FE_CLOCK,        /* [B][GF_CK_WORDS(M, budget)] i64 budget clock record
                           of the last step (see gf_set_budgets)             */
    GF_FE_TRACK,        /* [B][GF_TR_N] i32 tracking state, see GF_TR_*     */
    GF_FE_RELOC,        /* [B][64] gf_reloc_kf: keyframes' relocalisation-query
                           state (mnRelocQuery / mnRelocWords / mRelocScore) */
    GF_FE_NFIELDS
};
enum {
    GF_TR_STATE = 0,    /* mState after the step: 0 WORKING, 1 LOST, 2 NOT_INITIALIZED
                           (parked: the step extracts the stream's frame and
                           tracks nothing; see gf_frontend_set_lifecycle)    */
    GF_TR_VEL,          /* 1: mVelocity holds a motion, 0: empty              */
    GF_TR_SINCE,        /* mnId - mnLastRelocFrameId (saturates at 1 << 30)  */
    GF_TR_PATH,         /* initial estimate of the last step: 0 TrackWithMotionModel,
                           1 TrackPreviousFrame after it failed, 2 TrackPreviousFrame,
                           3 Relocalisation, 4 none (the stream is parked)   */
    GF_TR_QUERY,        /* mnId of the last frame (the keyframe database's query id) */
    GF_TR_OK,           /* bOK of the last step's initial estimate           */
    GF_TR_FORCE,        /* mbForceRelocalisation: 1 while a request of
                           gf_frontend_force_relocalisation is pending, else 0 */
    GF_TR_FORCE_KF,     /* mpLastKeyFrame of a pending request (graph keyframe
                           index), else 0                                     */
    GF_TR_N = 8
};
/* KeyFrame::mnRelocQuery / mnRelocWords / mRelocScore of one keyframe of a
 * stream's database (KeyFrame.h:163-165; the reference leaves mRelocScore
 * uninitialised, here it starts at 0). */
typedef struct gf_reloc_kf {
    uint32_t query;
    int32_t words;
    float score;
} gf_reloc_kf;
enum {
    GF_ST_M3 = 0,       /* SearchByProjection(Cur, Last) matches            */
    GF_ST_FOUND,        /* nMatchesFound after the outlier discard          */
    GF_ST_TO_MATCH,     /* num_to_match = budget - nMatchesFound            */
    GF_ST_BRANCH,       /* 1 leftovers only, 2 SearchByProjection, 3 active matching, 4 nToMatch = 0 */
    GF_ST_IN_VIEW,      /* nToMatch                                         */
    GF_ST_LOCAL,        /* matches of the local-map search (M2 or active)   */
    GF_ST_INL1,         /* inliers of the first PoseOptimization            */
    GF_ST_INL2,         /* mnMatchesInliers                                 */
    GF_ST_EXTRA,        /* SearchAdditionalMatchesInFrame matches           */
    GF_ST_NLEFT,        /* mLeftMapPoints size                              */
    GF_ST_ITER1, GF_ST_ITER2, GF_ST_EDGES1, GF_ST_EDGES2,
    GF_ST_FLAGS,        /* 1: M3 < 20 (TrackPreviousFrame fall-back), 2: < 10 after PoseOptimization,
                           4: mnMatchesInliers < 15 (LOST), 8: a time budget cut a loop,
                           16: timeCost_rest <= 0 (RunMapPointsSelection and
                           SearchByProjection_Budget return at once),
                           32: isInFrustum cap, 64: MAP_INFO cap (active branch),
                           128: runActiveMapMatching cap, 256: MAP_INFO cap of
                           RunMapPointsSelection, 512: visibility cap of
                           SearchAdditionalMatchesInFrame, 1024: SearchByProjection_Budget cap,
                           2048: TrackPreviousFrame ran, 4096: Relocalisation ran,
                           8192: the initial estimate failed (no TrackLocalMap),
                           16384: TrackLocalMap failed, 32768: relocalised,
                           65536: the relocalisation of this step was a forced
                           one (gf_frontend_force_relocalisation)            */
    GF_ST_FRAMES,       /* frames tracked                                   */
    GF_ST_LDETS,        /* logDet evaluations of runActiveMapMatching (heap
                           pushes, Observability.cc:1373): SURVEY §8d E_ld  */
    GF_ST_NLOCAL,       /* mvpLocalMapPoints size (keyframe graphs only)    */
    GF_ST_NCUT,         /* local points the isInFrustum cap moved to mLeftMapPoints */
    GF_ST_CAND_LAST,    /* SearchByProjection(Cur, Last): area candidates (GetFeaturesInArea
                           sizes; SURVEY §8d B_match's C)                   */
    GF_ST_CAND_PROJ,    /* the same for SearchByProjection(F, local) and
                           SearchByProjection_Budget together              */
    GF_ST_TPF,          /* TrackPreviousFrame's final nmatches (lmk_num_initTrack) */
    GF_ST_NCAND,        /* relocalisation candidates (DetectRelocalisationCandidates) */
    GF_ST_RELOC,        /* relocalisation: nGood of the last pose it optimised */
    GF_ST_RANSAC,       /* relocalisation: PnPsolver::iterate calls           */
    GF_FE_NSTAT
};
int gf_frontend_create(gf_ctx* ctx, const gf_frontend_params* params, gf_frontend** out);
int gf_frontend_destroy(gf_frontend* fe);
/* Keypoint capacity per frame (sum of the extractor's level quotas). */
int gf_frontend_capacity(gf_frontend* fe, int* cap);
/* Frame source: stream b's frame at step k is the image at d_bases[b] +
 * ((phase[b] + k) mod period) * frame_stride (device memory, row stride =
 * width). d_bases / phase are host arrays of B entries (copied). */
int gf_frontend_set_source(gf_frontend* fe, const uint8_t* const* d_bases, const int32_t* phase, int period,
                           size_t frame_stride);
/* The local map of one stream (host arrays; m <= map_cap), in
 * mvpLocalMapPoints order. Resets that stream's observability state. */
int gf_frontend_set_map(gf_frontend* fe, int stream, const gf_map_point* mps, const uint8_t* desc, int m);
int gf_frontend_set_rng(gf_frontend* fe, int stream, uint32_t seed);
/* ----------------------------------------- keyframe database (relocalisation)
 * The keyframes of a stream's map as Relocalisation reads them: per keyframe
 * its undistorted keypoints and descriptors (mvKeysUn, mDescriptors; slot i of
 * the keyframe graph's kf_mp is keypoint i), its BowVector (words ascending,
 * values) and FeatureVector (nodes ascending; node g's keypoints are
 * fv_feats[fv_start[g] .. fv_start[g + 1]), offsets absolute over all
 * keyframes, fv_start has fv_off[nkf] + 1 entries), all from
 * KeyFrame::ComputeBoW with the front end's vocabulary (levelsup 4). The
 * inverted file (KeyFrameDatabase::add, KeyFrameDatabase.cc:39-45) is built
 * from the BowVectors, keyframes in index order (= insertion order).
 * gf_kfdb_create uploads a database once (device resident; several streams
 * over one scene share it); gf_frontend_set_kfdb attaches it to a stream,
 * whose keyframe graph (gf_frontend_set_covis, same nkf and slot counts)
 * supplies the map points, isBad flags and covisibility. */
typedef struct gf_keyframe_db {
    int32_t nkf;
    const int32_t* kp_off;      /* [nkf + 1] keypoint offsets                 */
    const gf_keypoint* kps;     /* [kp_off[nkf]]                              */
    const uint8_t* desc;        /* [kp_off[nkf]][32]                          */
    const int32_t* bow_off;     /* [nkf + 1]                                  */
    const int32_t* bow_words;   /* [bow_off[nkf]]                             */
    const double* bow_values;   /* [bow_off[nkf]]                             */
    const int32_t* fv_off;      /* [nkf + 1] FeatureVector nodes per keyframe */
    const int32_t* fv_nodes;    /* [fv_off[nkf]]                              */
    const int32_t* fv_start;    /* [fv_off[nkf] + 1]                          */
    const int32_t* fv_feats;    /* [fv_start[fv_off[nkf]]] keyframe-local keypoint indices */
} gf_keyframe_db;
typedef struct gf_kfdb gf_kfdb;
int gf_kfdb_create(gf_ctx* ctx, const gf_keyframe_db* db, gf_kfdb** out);
int gf_kfdb_destroy(gf_kfdb* db);
/* A database that grows with the map (KeyFrameDatabase::add for the keyframes
 * LocalMapping hands on): the same input as gf_kfdb_create (offsets from 0),
 * with every device array allocated for max_kf keyframes (<= 64) and max_rows
 * keypoints in total. A keyframe has at most one BowVector word, one
 * FeatureVector node and one inverted-file entry per keypoint, so max_rows
 * bounds those arrays too. The inverted file is kept current on the device. A
 * database from gf_kfdb_create stays fixed and can be shared between streams;
 * a growable one belongs to one stream of one front end (attaching it while it
 * is attached elsewhere: GF_ERR_ARG; gf_frontend_set_kfdb(fe, stream, NULL)
 * releases it). `ctx` outlives the database's appends. */
int gf_kfdb_create_growable(gf_ctx* ctx, const gf_keyframe_db* db, int max_kf, int max_rows, gf_kfdb** out);
/* Host family, synchronous: rows->nkf keyframes (rows' own offsets from 0)
 * become the keyframes nkf .. nkf + rows->nkf - 1; several in one call give
 * what appending them one at a time gives. gf_kfdb_create's validation on the
 * host before anything is enqueued (GF_ERR_ARG: words or nodes not ascending,
 * a feature index out of range, more words / nodes / features than
 * keypoints); GF_ERR_CAP above max_kf or max_rows; GF_ERR_ARG on a fixed
 * database and on one attached to a front end (there the keyframes arrive
 * with gf_frontend_update_maps_kfdb). A refused call leaves the database
 * untouched. */
int gf_kfdb_append(gf_kfdb* db, const gf_keyframe_db* rows);
/* A database (fixed or growable) and its inverted file read back, packed:
 * counts[6] = keyframes, keypoints, BowVector entries, FeatureVector nodes,
 * FeatureVector features, inverted-file words (always written). out NULL
 * returns the counts only. Otherwise the arrays of `out` are caller buffers
 * that are written (the struct is the input one, hence its const), inv_words
 * [words], inv_off [words + 1] and inv_kf [BowVector entries] receive the
 * inverted file, and caps[6] holds the buffers' capacities in the order of
 * counts (offset arrays hold one more); a cap too small: GF_ERR_CAP, nothing
 * copied. Synchronises the device. What a test compares and what a caller
 * checkpoints: the output is gf_kfdb_create_growable's input. */
int gf_kfdb_read(gf_kfdb* db, int32_t counts[6], gf_keyframe_db* out, int32_t* inv_words, int32_t* inv_off,
                 int32_t* inv_kf, const int32_t caps[6]);
/* NULL detaches (Relocalisation then finds no candidate). The stream's
 * keyframes' query state (GF_FE_RELOC) is reset. With a growable database
 * attached, the candidate scratch of the step is laid out for its max_kf, so a
 * captured graph stays valid while the database grows. */
int gf_frontend_set_kfdb(gf_frontend* fe, int stream, gf_kfdb* db);
/* The vocabulary of Frame::ComputeBoW for relocalisation (mpORBVocabulary);
 * the caller keeps it alive while the front end steps. */
int gf_frontend_set_vocab(gf_frontend* fe, gf_vocab* voc);
/* The track-loss matchers of the step, one problem per call (host arrays,
 * synchronous; at most 4096 keypoints a frame and map points):
 * gf_window_search: ORBmatcher::WindowSearch(F1, F2, window,
 *   vpMapPointMatches2, min_level, max_level) (ORBmatcher.cc:979-1086) with
 *   ORBmatcher(nnratio, check_ori); F1 = keypoints / descriptors / map point
 *   per keypoint (-1 NULL) of the last frame, F2 the current frame; out (n2)
 *   = vpMapPointMatches2; max_level = INT_MAX for none.
 * gf_search_frames: ORBmatcher::SearchByProjection(F1, F2, window,
 *   vpMapPointMatches2) (:1089-1168): F1's map points (world positions pos1)
 *   projected with Tcw2; kp2mp / score (n2) are F2.mvpMapPoints /
 *   mvpMatchScore, in and out.
 * gf_search_kf_projection: ORBmatcher::SearchByProjection(F, pKF,
 *   sAlreadyFound, th, ORBdist) (:2204-2336): the keyframe's slots (kf_mp,
 *   its keypoints for the angle) against the frame at Tcw; found = a byte per
 *   map point (sAlreadyFound); kp2mp / score in and out.
 * gf_reloc_candidates: KeyFrameDatabase::DetectRelocalisationCandidates
 *   (KeyFrameDatabase.cc:198-308) for a frame's BowVector against db's
 *   keyframes (kf_bad optional; cov_off / cov = mvpOrderedConnectedKeyFrames);
 *   query = the frame's mnId (!= 0); state (db->nkf entries) persists across
 *   queries as the keyframes' fields do. */
int gf_window_search(gf_ctx* ctx, const gf_frame_info* fi, const gf_keypoint* kps2, const uint8_t* desc2, int n2,
                     const gf_keypoint* kps1, const uint8_t* desc1, const int32_t* mp1, int n1, int window,
                     int min_level, int max_level, float nnratio, int check_ori, int32_t* out, int* nmatches);
int gf_search_frames(gf_ctx* ctx, const gf_frame_info* fi, const gf_keypoint* kps2, const uint8_t* desc2, int n2,
                     const float* Tcw2, const gf_keypoint* kps1, const uint8_t* desc1, const int32_t* mp1,
                     const float* pos1, int n1, int window, float nnratio, int32_t* kp2mp, int32_t* score,
                     int* nmatches);
int gf_search_kf_projection(gf_ctx* ctx, const gf_frame_info* fi, const gf_keypoint* kps, const uint8_t* desc, int n,
                            const float* Tcw, const gf_keypoint* kf_kps, const int32_t* kf_mp, int nslots,
                            const gf_map_point* mps, const uint8_t* mp_desc, int nmp, const uint8_t* found, float th,
                            int orb_dist, int check_ori, int32_t* kp2mp, int32_t* score, int* nmatches);
int gf_reloc_candidates(gf_ctx* ctx, const int32_t* words, const double* values, int nwords, const gf_keyframe_db* db,
                        const uint8_t* kf_bad, const int32_t* cov_off, const int32_t* cov, uint32_t query,
                        gf_reloc_kf* state, int32_t* cands, int* ncand);
/* The keyframe graph of one stream's map (host arrays, gf_covis_map over the
 * map set with gf_frontend_set_map: g->nmp must equal its size; at most 64
 * keyframes, 64 x keypoint-capacity slots and observations). Once any stream
 * has a graph, every step first runs Tracking::UpdateReference
 * (Tracking.cc:2745, 3689-3852) on the frame's matches after
 * TrackWithMotionModel and tracks the rest of the frame against the local map
 * it returns (local keyframes' points, mvpLocalMapPoints order), so the local
 * map follows the camera; every stream then needs a graph. The map fields
 * (GF_FE_MAP, VIEWS, MP_*) keep indexing the stream's map, and GF_FE_LEFT /
 * GF_FE_KP2MP map indices. The bootstrap matches the whole map. */
int gf_frontend_set_covis(gf_frontend* fe, int stream, const gf_covis_map* graph);
/* Start of tracking: the current source frame of every stream is taken at the
 * given pose (Tcw [B][16]) and matched to its local map
 * (isInFrustum + SearchByProjection(F, local, 1) with nnratio 0.8); it becomes
 * mLastFrame with timestamp t0, V [B][16] the motion model, and the step
 * counter advances by one. */
int gf_frontend_bootstrap(gf_frontend* fe, const float* Tcw, const float* V, double t0);
/* Same with the B bootstrap frames from host memory ([B][height][width] u8),
 * for callers without a device frame source (then step with
 * gf_frontend_step_host). */
int gf_frontend_bootstrap_host(gf_frontend* fe, const uint8_t* imgs, const float* Tcw, const float* V, double t0);
/* One frame per stream from the source (asynchronous on the context stream). */
int gf_frontend_step(gf_frontend* fe);
/* gf_frontend_step in two calls: the extraction gate and Frame construction
 * (ORB extraction, undistortion; the Frame(...) of Tracking.cc:521), then tracking (Track()). Lets a caller stepping several
 * gated front ends from one thread enqueue every front end's extraction before
 * any tracking. Each call fails with GF_ERR_ARG out of order; gf_frontend_step
 * fails while an extracted frame awaits tracking. Not for captured front ends. */
int gf_frontend_step_extract(gf_frontend* fe);
int gf_frontend_step_track(gf_frontend* fe);
/* Same with the B frames taken from host memory ([B][height][width] u8):
 * the PCIe copy is part of the step. */
int gf_frontend_step_host(gf_frontend* fe, const uint8_t* imgs);
/* Capture gf_frontend_step as one HIP graph; later steps replay it (and
 * capture again when gf_set_budgets changed the budgets). While the graph
 * exists the context's scratch buffers are pinned: a call on the same context
 * that would need a larger one fails with GF_ERR_ARG instead of freeing
 * memory the graph uses. */
int gf_frontend_capture(gf_frontend* fe);
int gf_frontend_sync(gf_frontend* fe);
/* Copy a whole-batch field (synchronises; bytes must equal the field size). */
int gf_frontend_read(gf_frontend* fe, int field, void* host, size_t bytes);
int gf_frontend_write(gf_frontend* fe, int field, const void* host, size_t bytes);
/* Size and device pointer of a field. */
int gf_frontend_field(gf_frontend* fe, int field, size_t* bytes, void** d_ptr);

/* ------------------------------------------------------------ map feedback
 * What LocalMapping wrote into the map since the tracker last looked, for one
 * stream, in the front end's own indices (map index, graph keyframe index;
 * this call only appends, so every index the front end holds stays valid;
 * gf_frontend_compact_maps is what renumbers). In the
 * reference Tracking reads these through MapPoint* / KeyFrame* (Tracking.cc:
 * 3689-3852): here they are applied to the stream's map and keyframe graph in
 * place, on the context's stream behind the last step. Host arrays; an array
 * whose count is 0 may be NULL.
 *   new_mp / new_mp_desc / new_mp_bad [n_new_mp]: Map::AddMapPoint; they take
 *     the indices nmp .. nmp + n_new_mp - 1 with the per-point state of a
 *     fresh point (GF_FE_MP_UPD -1000, GF_FE_VIEWS 0). new_mp_bad NULL: none.
 *   set_mp_idx / set_mp / set_mp_desc [n_set_mp]: SetWorldPos,
 *     UpdateNormalAndDepth and ComputeDistinctiveDescriptors of existing points
 *     (distinct indices < nmp); GF_FE_MP_H / MP_INFO / MP_UV / MP_UPD / VIEWS of
 *     the point stay as they are.
 *   bad_mp [n_bad_mp]: MapPoint::SetBadFlag / Replace: mp_bad = 1 (indices <
 *     nmp + n_new_mp). A bad point never returns; its state rows stay.
 *   new_kf_off [n_new_kf + 1] / new_kf_mp / new_kf_bad [n_new_kf]:
 *     Map::AddKeyFrame; slot rows as a CSR starting at 0, appended at the tail
 *     of kf_mp (existing rows do not move). new_kf_bad NULL: none.
 *   bad_kf [n_bad_kf]: KeyFrame::SetBadFlag (indices < nkf + n_new_kf).
 *   slot_kf / slot_idx / slot_val [n_slot]: AddMapPoint / ReplaceMapPointMatch /
 *     EraseMapPointMatch on existing keyframes (kf < nkf), value -1 = NULL, at
 *     most one write per slot.
 *   obs_mp [n_obs_rows] / obs_off [n_obs_rows + 1] / obs_kf: the whole new
 *     observation row (observing keyframe indices, ascending) of every touched
 *     point, old or appended (distinct points); an untouched point keeps its row
 *     and an appended point without a row has none.
 *   kf_cov_off [nkf + n_new_kf + 1] / kf_cov: mvpOrderedConnectedKeyFrames of
 *     every keyframe, when has_cov != 0; otherwise the lists stay and appended
 *     keyframes get empty ones. */
typedef struct gf_map_delta {
    int32_t stream;
    int32_t n_new_mp;
    const gf_map_point* new_mp;
    const uint8_t* new_mp_desc;
    const uint8_t* new_mp_bad;
    int32_t n_set_mp;
    const int32_t* set_mp_idx;
    const gf_map_point* set_mp;
    const uint8_t* set_mp_desc;
    int32_t n_bad_mp;
    const int32_t* bad_mp;
    int32_t n_new_kf;
    const int32_t* new_kf_off;
    const int32_t* new_kf_mp;
    const uint8_t* new_kf_bad;
    int32_t n_bad_kf;
    const int32_t* bad_kf;
    int32_t n_slot;
    const int32_t* slot_kf;
    const int32_t* slot_idx;
    const int32_t* slot_val;
    int32_t n_obs_rows;
    const int32_t* obs_mp;
    const int32_t* obs_off;
    const int32_t* obs_kf;
    int32_t has_cov;
    const int32_t* kf_cov_off;
    const int32_t* kf_cov;
} gf_map_delta;
/* Apply ndelta deltas (any number of streams, each named at most once; every
 * stream needs a keyframe graph) in one upload and one set of launches, with
 * no host synchronisation on success. Legal after gf_frontend_capture: no
 * buffer moves, and the step reads every count it needs from device memory.
 * Everything is validated on the host first: GF_ERR_ARG for an index out of
 * range, a row that is not ascending, a duplicate stream / point / slot;
 * GF_ERR_CAP above 64 keyframes, map_cap points, 64 x keypoint-capacity slots
 * or observations, or nkf^2 covisibility entries (the capacities do not grow:
 * gf_frontend_compact_maps makes room in a map that reaches them);
 * GF_ERR_UNSUPPORTED for an appended keyframe on a stream whose keyframe
 * database cannot follow it (gf_frontend_set_kfdb: the database and the graph
 * must agree in keyframes): a fixed database, or a growable one without the
 * keyframe's rows (gf_frontend_update_maps_kfdb). A failing delta leaves every
 * stream of the call untouched.
 * After the call the map's cached copies are current: the float3 positions,
 * GF_FE_LAST_POS of the last frame's points, the graph's mp_bad. A stream not
 * named and every row not addressed are byte-identical before and after. */
int gf_frontend_update_maps(gf_frontend* fe, int ndelta, const gf_map_delta* deltas);
/* The same call with the appended keyframes' database rows: kf_rows[i] is NULL
 * or the rows of deltas[i]'s appended keyframes (nkf == n_new_kf, offsets from
 * 0, keyframe k with as many keypoints as its new_kf_off row has slots), which
 * join the stream's growable database (gf_kfdb_create_growable) in the same
 * launches: KeyFrameDatabase::add. kf_rows NULL is gf_frontend_update_maps.
 * On a stream with a database an appended keyframe needs a growable database
 * and its rows (GF_ERR_UNSUPPORTED otherwise); rows on a stream without a
 * database or with n_new_kf == 0, rows that differ from the slot counts and
 * what gf_kfdb_append refuses: GF_ERR_ARG; above the database's max_kf or
 * max_rows: GF_ERR_CAP. As for every failure of this call, no stream, graph
 * or database of the call is touched. On success there is no host
 * synchronisation and the call is legal after gf_frontend_capture: the step
 * reads the stream's database record from device memory, and the last kernel
 * flips it to the merged inverted file. Existing keyframes' GF_FE_RELOC rows
 * are untouched; an appended keyframe's row is zero (a keyframe no query has
 * touched). Staging for the rows is allocated by the first call of a size. */
int gf_frontend_update_maps_kfdb(gf_frontend* fe, int ndelta, const gf_map_delta* deltas,
                                 const gf_keyframe_db* const* kf_rows);
/* ------------------------------------------- stream start, park and reset
 * A stream whose GF_TR_STATE is 2 (NOT_INITIALIZED) is parked: the step
 * extracts its frame as for every stream, but the frame is not tracked, not
 * relocalised and creates no keyframe. Its carried state (map, graph, database
 * record, GF_FE_RELOC row, last frame, velocity, GF_FE_RNG, per-point state,
 * Xv / Xv_next / base, the GF_KF_* words) stays byte-identical however many
 * steps pass; only the per-step outputs change: the current frame's keypoints,
 * descriptors, count and match arrays, GF_FE_TCW (zeros, a fresh Frame's empty
 * mTcw), GF_FE_T_CUR, the stats, GF_TR_QUERY, GF_TR_SINCE, GF_TR_PATH = 4 and
 * GF_TR_OK = 0. The extraction of a parked stream still runs.
 *
 * gf_frontend_set_lifecycle(fe, on), before gf_frontend_capture like the other
 * set calls; off is the default. When on, the step applies the reset rule of
 * Tracking::GrabImage (Tracking.cc:718-726): a stream whose verdict is LOST and
 * whose map holds at most 5 keyframes (the count the step reads for the < 4
 * test of :602; a stream without a keyframe graph, count -1, never resets) goes
 * to state 2 instead of 1. Nothing else is written: the map stays where it is
 * (parking stands for mpKeyFrameDB->clear() / mpMap->clear() until the host
 * reacts), so the host mirrors stay true, and the next gf_frontend_start_streams
 * overwrites everything. Switching it on also allocates what the first
 * gf_frontend_set_covis and gf_frontend_set_kfdb would allocate and gives every
 * stream that has no map and no graph an empty graph (0 keyframes, 0 points) in
 * state 2, so that a front end can begin empty and be captured. An empty
 * growable database attaches to such a graph with gf_frontend_set_kfdb. It
 * also allocates the staging of gf_frontend_start_streams and of the map
 * update, so that no start on this front end allocates or synchronises;
 * without it the first start (as the first gf_frontend_update_maps) allocates
 * its staging and synchronises once.
 * Which streams it parks is decided at the call: those with neither a map nor
 * a graph at that moment. A parked stream leaves state 2 only through
 * gf_frontend_start_streams or a write of GF_TR_STATE (GF_FE_TRACK):
 * gf_frontend_set_map / gf_frontend_set_covis on a parked stream leave it
 * parked. gf_frontend_bootstrap is the start of every stream at once and
 * overrides parking: it sets every stream WORKING, a parked one included.
 * gf_frontend_lifecycle_read: GF_TR_STATE of every stream ([B] i32), after a
 * synchronisation. */
int gf_frontend_set_lifecycle(gf_frontend* fe, int on);
int gf_frontend_lifecycle_read(gf_frontend* fe, int32_t* state);
/* One stream's beginning (Tracking::CreateInitialMap, Tracking.cc:1302-1321):
 *   map: the whole new map as a delta read against an empty map (appended
 *     points, appended keyframes with their slot rows, observation rows, the
 *     covisibility lists; n_set_mp, n_bad_mp, n_bad_kf and n_slot must be 0);
 *     map.stream names the stream.
 *   the frame that becomes mLastFrame (:1308): n_last <= the keypoint capacity
 *     undistorted keypoints, descriptors and kp2mp (indices of the new map, -1
 *     NULL; no outliers), its pose, timestamp and mnId, and since_reloc =
 *     mnId - mnLastRelocFrameId.
 *   ref_kf: mpReferenceKF = pKFcur (:1315) as an index of the new graph (-1
 *     only for a map without keyframes). */
typedef struct gf_stream_start {
    gf_map_delta map;
    int32_t n_last;
    const gf_keypoint* last_kps;
    const uint8_t* last_desc;   /* [n_last][32] */
    const int32_t* last_kp2mp;
    float Tcw[16];
    double timestamp;
    int32_t frame_id, since_reloc;
    int32_t ref_kf;
} gf_stream_start;
/* Start n streams (each named at most once; every one needs a keyframe graph,
 * possibly the empty one of gf_frontend_set_lifecycle) in one upload and one
 * set of launches on the context's stream behind the last step, with no host
 * synchronisation on success (the staging is allocated by
 * gf_frontend_set_lifecycle, else by the first call, which then synchronises
 * once); legal after gf_frontend_capture. kf_rows is NULL
 * or per request NULL / the database rows of the map's keyframes, as in
 * gf_frontend_update_maps_kfdb. On success a named stream holds
 *   the map alone: counts, points, descriptors, cached positions, mp_bad, slot
 *     rows, observation rows and covisibility are those of the delta, the
 *     per-point state of rows [0, nmp) that of fresh points (GF_FE_MP_UPD
 *     -1000, GF_FE_VIEWS 0; MP_H / MP_INFO / MP_UV as gf_frontend_set_map
 *     leaves them); rows past the new counts keep their bytes;
 *   the last frame: GF_FE_LAST_* from the request (LAST_OUTLIER 0), LAST_POS
 *     gathered from the new map on the device, TCW_LAST and T_PREV from the
 *     request, T_CUR = T_PREV; KP2MP (-1) and OUTLIER (0) of the current frame
 *     cleared; GF_FE_LEFT empty (GF_ST_NLEFT 0);
 *   the tracking words: STATE 0, VEL 0 (mVelocity is empty after the
 *     initialiser, so the next step takes TrackPreviousFrame), SINCE =
 *     since_reloc, QUERY = frame_id, PATH 2, OK 1;
 *   the keyframe words (when the stage is allocated): SINCE 0 (:1309), PENDING
 *     0 (an untaken keyframe of the old map is dropped, as RequestReset empties
 *     mlNewKeyFrames), ABORT 0, DECISION 0, REF and the persistent
 *     reference-keyframe word = ref_kf; the other words stay;
 *   Xv, Xv_next and base as gf_frontend_create leaves them (zeros); GF_FE_RNG
 *     and GF_FE_VELOCITY untouched;
 *   the database: a growable one is emptied (KeyFrameDatabase::clear) and then
 *     holds exactly the given rows, inverted file rebuilt on the device; the
 *     stream's GF_FE_RELOC rows are zero and no relocalisation candidate
 *     survives. A fixed database: GF_ERR_UNSUPPORTED. Rows without a database:
 *     GF_ERR_ARG.
 * Validation on the host first, as gf_frontend_update_maps_kfdb against an
 * empty map (ranges, ascending rows, duplicates, GF_ERR_CAP above 64
 * keyframes, map_cap points, the slot / observation / covisibility capacities,
 * the database's max_kf and max_rows), plus GF_ERR_ARG for a non-empty set_*,
 * bad_* or slot_* array, kp2mp or ref_kf out of range, and GF_ERR_CAP for
 * n_last above the keypoint capacity. A failing request leaves every stream,
 * graph and database of the call untouched; a stream not named is
 * byte-identical before and after; n == 0 launches nothing. */
int gf_frontend_start_streams(gf_frontend* fe, int n, const gf_stream_start* reqs,
                              const gf_keyframe_db* const* kf_rows);
/* ------------------------------------------------------ ForceRelocalisation
 * Tracking::ForceRelocalisation (Tracking.cc:4035-4045), what
 * LoopClosing::CorrectLoop calls after it has moved the map (LoopClosing.cc:
 * 554): the next step of each named stream takes the relocalisation branch
 * although the stream is WORKING (Tracking.cc:584, 622-628), and Relocalisation
 * does not ask the keyframe database: its candidates are the local window
 * around the last keyframe, mpLastKeyFrame->GetBestCovisibilityKeyFrames(9)
 * followed by mpLastKeyFrame (:3866-3879).
 * The request writes, per named stream, GF_TR_FORCE = 1, GF_TR_FORCE_KF =
 * last_kf[i] and GF_TR_SINCE = 0 (:4044, mnLastRelocFrameId = mCurrentFrame.
 * mnId): one upload and one small kernel on the context's stream behind the
 * last step, with no host synchronisation (the first call allocates its
 * staging and synchronises once); legal after gf_frontend_capture. last_kf
 * NULL or last_kf[i] == -1: the newest keyframe of the stream's graph that is
 * not bad (the device reads kf_bad; the newest one when all are bad).
 * The next step of such a stream: GF_TR_PATH 3 whatever GF_TR_STATE is, except
 * that a parked stream (state 2) stays on path 4 and keeps the request pending,
 * byte for byte. The candidate list is the first min(9, row length) entries of
 * FORCE_KF's covisibility row in the row's order, then FORCE_KF; GF_ST_NCAND is
 * its length, GF_ST_FLAGS gains 65536, both words go back to 0 before the list
 * is used (the reference clears the flag first, :3864: a forced relocalisation
 * that fails leaves a LOST stream that asks the database from the next frame
 * on), and the keyframes' query state (GF_FE_RELOC) is not touched. A candidate
 * the stream's database does not hold (index >= its keyframe count) has no
 * SearchByBoW matches and is discarded by nmatches < 15; bad keyframes are
 * discarded as in every relocalisation. gf_frontend_start_streams clears a
 * pending request; map compaction pins and renumbers FORCE_KF as it does the
 * reference keyframe.
 * Decided on the host, nothing written: GF_ERR_ARG for a stream out of range or
 * named twice, a stream without a keyframe graph (an empty one included) and
 * last_kf outside [-1, keyframes of the graph); without a vocabulary or without
 * a database on the stream, the status the step's relocalisation is refused
 * with (GF_ERR_ARG). n == 0 launches nothing. */
int gf_frontend_force_relocalisation(gf_frontend* fe, int n, const int32_t* streams, const int32_t* last_kf);
/* The relocalisation candidates every stream used in the last step: cands
 * [B][64] (entries past ncand[b] are whatever an earlier step left) and
 * ncand[B]; 0 for a stream that did not relocalise. Synchronises. */
int gf_frontend_reloc_candidates_read(gf_frontend* fe, int32_t* cands, int32_t* ncand);
/* The keyframe graph the front end holds for a stream. counts[5] = nkf, nmp,
 * slots, covisibility entries, observations (always written); the arrays of
 * `out` are caller buffers with caps[3] = slot, covisibility and observation
 * capacity, and room for 64 + 1 keyframe entries and map_cap + 1 point entries.
 * out NULL returns the counts only; a cap too small: GF_ERR_CAP, nothing
 * copied. Synchronises. */
typedef struct gf_covis_out {
    uint8_t* kf_bad;
    int32_t* kf_mp_off;
    int32_t* kf_mp;
    int32_t* kf_cov_off;
    int32_t* kf_cov;
    uint8_t* mp_bad;
    int32_t* mp_obs_off;
    int32_t* mp_obs;
} gf_covis_out;
int gf_frontend_get_covis(gf_frontend* fe, int stream, int32_t* counts, const gf_covis_out* out, const int32_t* caps);

/* ---------------------------------------------------------- map compaction
 * The inverse of the map feedback: keyframes and points leave a stream's map
 * on the device, in place, and every index the front end holds is renumbered.
 * It stands for Map::EraseMapPoint / Map::EraseKeyFrame (Map.cc) and, for the
 * keyframe's database rows, KeyFrameDatabase::erase (KeyFrameDatabase.cc:
 * 47-60). Used as a window (good keyframes and their points dropped so that a
 * stream runs past the capacities) it stands for nothing: the reference's map
 * is unbounded.
 * The stream's map becomes the restriction of its map to the kept keyframes
 * and points. Kept items keep their relative order (keyframe order is
 * KeyFrame* order for UpdateReference). Every per-point row moves with its
 * point, byte for byte: GF_FE_MAP, MAP_DESC, VIEWS, MP_H, MP_INFO, MP_UV,
 * MP_UPD, the graph's mp_bad and the internal copies (float3 positions, packed
 * ObsMat triangles). kf_bad and GF_FE_RELOC rows move with their keyframe.
 * Slot rows of dropped keyframes disappear, kept rows close up, slot values
 * are renumbered (a slot that named a dropped point becomes -1). Observation
 * rows are filtered to the kept keyframes and renumbered (they stay
 * ascending), covisibility lists are filtered in order and renumbered. Rows
 * past the new counts keep whatever bytes they held.
 * Pins: a point the next step can still read through frame state is kept even
 * when listed: the points of GF_FE_KP2MP[0..nkp), GF_FE_LAST_KP2MP[0..last_nkp)
 * and the slots of a pending outbox keyframe (GF_KF_PENDING); so are the
 * keyframe the persistent reference-keyframe word names and the GF_TR_FORCE_KF
 * of a pending forced relocalisation. The device decides
 * (a mark pass before the scan) and reports: n_kept_* count the listed items
 * that stayed, and the remap tables say where everything went. A pinned point
 * whose keyframes are all gone keeps an empty observation row. Those holders
 * are renumbered; GF_FE_LEFT[0..nleft) and GF_KF_REF, outputs of the last
 * step, are renumbered with a dropped entry turned into -1.
 * Everything is validated on the host first: GF_ERR_ARG for an index out of
 * range, a duplicate, a stream named twice or a stream without a keyframe
 * graph; GF_ERR_UNSUPPORTED for a non-empty drop_kf on a stream with a fixed
 * (shareable) keyframe database attached (a points-only request is fine
 * there). On a stream with a growable database (gf_kfdb_create_growable) a
 * dropped keyframe's database rows go with it (keypoints, descriptors,
 * BowVector, FeatureVector, offsets rebased), the inverted file is filtered
 * and renumbered into the database's other buffer set and the record the step
 * reads is flipped: KeyFrameDatabase::erase. A failing request leaves every stream of the call untouched;
 * an empty request is a no-op with identity remaps. A stream not named is
 * byte-identical before and after.
 * The call runs behind the last step on the context's stream and is legal
 * after gf_frontend_capture: no buffer moves, and the step reads every count
 * from device memory. It synchronises once at the end (the result is
 * device-decided) and brings the host mirrors up to date, so that
 * gf_frontend_update_maps works against the compacted map with no read-back
 * of its own. */
typedef struct gf_map_compact {   /* one stream */
    int32_t stream;
    int32_t n_drop_kf;
    const int32_t* drop_kf;       /* graph keyframe indices, distinct */
    int32_t n_drop_mp;
    const int32_t* drop_mp;       /* map indices, distinct            */
} gf_map_compact;
typedef struct gf_map_remap {     /* caller buffers, one per request  */
    int32_t nkf, nmp;             /* after the call                   */
    int32_t* kf_remap;            /* [old nkf] new index, -1 dropped (room for 64)       */
    int32_t* mp_remap;            /* [old nmp] new index, -1 dropped (room for map_cap)  */
    int32_t n_kept_kf, n_kept_mp; /* requested drops that were pinned */
} gf_map_remap;
int gf_frontend_compact_maps(gf_frontend* fe, int n, const gf_map_compact* reqs, gf_map_remap* out);

/* ------------------------------------- NeedNewKeyFrame / CreateNewKeyFrame
 * `if(NeedNewKeyFrame()) CreateNewKeyFrame();` (Tracking.cc:896-897), the
 * only way a frame becomes a keyframe: a stage of the step between the
 * hand-back of the local map and the NULLing of the outlier matches
 * (:899-907), so the keyframe carries the outliers and bundle adjustment
 * decides about them (:899-902). Off until gf_frontend_set_keyframes.
 * Per-stream state, [B][GF_KF_N] i32 (not a GF_FE_* field; read and written
 * with gf_frontend_keyframe_state_read / _write):                          */
enum {
    GF_KF_SINCE = 0,    /* mnId - mnLastKeyFrameId: + 1 every step for every stream
                           (saturates at 1 << 30), 0 on creation and when the stage
                           is enabled (Tracking.cc:1309); host-writable              */
    GF_KF_ACCEPT,       /* mbAcceptKeyFrames (LocalMapping.cc:566-576): set by the
                           host, cleared on creation (:70)                           */
    GF_KF_STOP,         /* isStopped() || stopRequested() (:3042); host only         */
    GF_KF_NKF,          /* KeyFramesInMap() (:3046); -1: the keyframe graph's count  */
    GF_KF_ABORT,        /* mbAbortBA: raised on creation (LocalMapping.cc:153) and by
                           InterruptBA (:3071); cleared by the host (LocalMapping.cc:98) */
    GF_KF_DECISION,     /* bits of the last step: 1 evaluated (the frame ended
                           WORKING), 2 refused by the stop test (:3042), 4 refused by
                           the relocalisation test (:3046), 8 c1a, 16 c1b, 32 c2,
                           64 created, 128 InterruptBA, 256 no reference keyframe
                           (verdict false; the reference would dereference NULL,
                           :3050 after :3851). Tests not reached leave their bits 0 */
    GF_KF_REF,          /* mpReferenceKF (keyframe index) the rule read; -1 when
                           not evaluated or none                                     */
    GF_KF_REF_MATCHES,  /* nRefMatches = mpReferenceKF->TrackedMapPoints()
                           (KeyFrame.cc:253-265); 0 when not evaluated / no reference */
    GF_KF_INLIERS,      /* mnMatchesInliers the rule read; 0 when not evaluated      */
    GF_KF_SEQ,          /* keyframes created so far                                  */
    GF_KF_PENDING,      /* 1: the outbox slot holds a keyframe not yet taken         */
    GF_KF_FRAME,        /* its mnFrameId (GF_TR_QUERY of the creating step)          */
    GF_KF_N = 16
};
/* Header of a keyframe in the outbox / of a taken keyframe: `new
 * KeyFrame(mCurrentFrame, ...)` (KeyFrame.cc:30-54) without the rows. */
typedef struct gf_keyframe_hdr {
    int32_t stream, seq;        /* the creating stream, its GF_KF_SEQ after creation */
    int32_t frame_id, n;        /* mnFrameId, N                                      */
    double timestamp;           /* mTimeStamp                                        */
    float Tcw[16];              /* mTcw                                              */
} gf_keyframe_hdr;
/* Tracking::NeedNewKeyFrame (Tracking.cc:3035-3077) alone, host, scalar, in
 * the reference's order and arithmetic (c2's product is a double). since_kf =
 * mnId - mnLastKeyFrameId, since_reloc = mnId - mnLastRelocFrameId, stop =
 * isStopped() || stopRequested(), nkf = KeyFramesInMap(), n_ref_matches =
 * mpReferenceKF->TrackedMapPoints() (< 0: no reference keyframe), accept =
 * AcceptKeyFrames(). *decision (optional) gets the GF_KF_DECISION bits with 1
 * set; *need 1 / 0; InterruptBA is bit 128 (the caller raises mbAbortBA). */
int gf_need_new_keyframe(int since_kf, int since_reloc, int stop, int nkf, int n_ref_matches, int inliers, int accept,
                         int min_frames, int max_frames, int* need, int* decision);
/* The stage on explicit device arrays (the step launches the same kernel, one
 * workgroup per stream): the rule of :3035-3077 with nRefMatches counted from
 * the reference keyframe's slot row, the state words updated as listed at
 * GF_KF_*, and for a stream that creates the snapshot of KeyFrame.cc:30-54
 * into its outbox slot with the effects of CreateNewKeyFrame (:3079-3092) and
 * LocalMapping::InsertKeyFrame (LocalMapping.cc:149-155). A stream that does
 * not create writes nothing into the outbox; no stream writes a row >= N. */
typedef struct gf_newkf_args {
    int32_t B, cap;             /* streams, keypoint rows per stream                 */
    const int32_t* nkp;         /* [B] N                                             */
    const gf_keypoint* kps;     /* [B][cap] mvKeysUn                                 */
    const uint8_t* desc;        /* [B][cap][32] mDescriptors                         */
    const int32_t* kp2mp;       /* [B][cap] mvpMapPoints (map index, -1 NULL)        */
    const float* Tcw;           /* [B][16] mTcw                                      */
    const double* t_cur;        /* [B] mTimeStamp                                    */
    const int32_t* track;       /* [B][GF_TR_N]: GF_TR_SINCE, GF_TR_QUERY are read   */
    const int32_t* inliers;     /* [B] mnMatchesInliers                              */
    const int32_t* working;     /* [B] != 0: the frame ended WORKING (:854)          */
    const int32_t* ref_kf;      /* [B] mpReferenceKF as a keyframe index, -1 none    */
    const int32_t* kf_count;    /* [B] keyframes of the stream's graph               */
    const int32_t* kf_mp_off;   /* [B][off_stride] CSR of KeyFrame::mvpMapPoints     */
    const int32_t* kf_mp;       /* [B][slot_stride] map index per slot, -1 NULL      */
    int64_t off_stride, slot_stride;
    int32_t* state;             /* [B][GF_KF_N]                                      */
    gf_keyframe_hdr* out_hdr;   /* [B]       the outbox                              */
    gf_keypoint* out_kps;       /* [B][cap]                                          */
    uint8_t* out_desc;          /* [B][cap][32]                                      */
    int32_t* out_slots;         /* [B][cap]                                          */
    int32_t min_frames;         /* mMinFrames (0, Tracking.cc:151)                   */
    int32_t max_frames;         /* mMaxFrames (:153)                                 */
} gf_newkf_args;
int gf_need_new_keyframe_dev(gf_ctx* ctx, const gf_newkf_args* args, void* stream);
/* Switch the stage on / off for the following steps: min_frames = mMinFrames
 * (0 in the reference, Tracking.cc:151), max_frames <= 0 = the front end's
 * mMaxFrames. Needs a keyframe graph on every stream (gf_frontend_set_covis)
 * and comes before gf_frontend_capture, like the other set calls. Allocates
 * the state and the outbox on first use and resets the state: SINCE 0 (as
 * after :1309), ACCEPT 1, NKF -1, everything else 0. Off is the default, and
 * with the stage off a step launches exactly what it launched without it. */
int gf_frontend_set_keyframes(gf_frontend* fe, int on, int min_frames, int max_frames);
/* The state words of every stream, [B][GF_KF_N] i32 (synchronises). The write
 * refuses (GF_ERR_ARG, nothing written) a state with ACCEPT and PENDING both
 * set on a stream: mbAcceptKeyFrames comes back only after the keyframe was
 * taken (LocalMapping.cc:116-117), so the device never overwrites an untaken
 * keyframe. */
int gf_frontend_keyframe_state_read(gf_frontend* fe, int32_t* state, size_t bytes);
int gf_frontend_keyframe_state_write(gf_frontend* fe, const int32_t* state, size_t bytes);
/* mlNewKeyFrames' hand-over (LocalMapping.cc:149-155, 168-176): the pending
 * outbox slots packed on the device into one contiguous buffer, downloaded,
 * and their PENDING cleared. Streams ascending; at most max_kf keyframes, the
 * lowest streams first. hdr [max_kf]; keyframe j's rows are
 * [sum of hdr[i].n for i < j, + hdr[j].n) of kps / desc ([rows_cap][32]) /
 * slots (map indices, outliers still in place). *nkf keyframes taken, *nrows
 * their rows. rows_cap too small: GF_ERR_CAP, nothing taken, *nrows = need. */
int gf_frontend_take_keyframes(gf_frontend* fe, int max_kf, int rows_cap, gf_keyframe_hdr* hdr, gf_keypoint* kps,
                               uint8_t* desc, int32_t* slots, int* nkf, int* nrows);
/* The device pointers of the state and the outbox ([B][GF_KF_N], [B],
 * [B][cap], [B][cap][32], [B][cap]) for a caller that stays on the device;
 * any may be NULL. */
int gf_frontend_keyframes_dev(gf_frontend* fe, int32_t** d_state, gf_keyframe_hdr** d_hdr, gf_keypoint** d_kps,
                              uint8_t** d_desc, int32_t** d_slots);

/* Wall-clock budgets of the reference's time-capped loops, in seconds; +inf
 * (the default) is parity mode: no loop is cut and no clock is read.
 *   match_s  = time_total_match (Tracking.cc:3230, 0.015 in the reference).
 *   select_s = the post-publish frame budget 1/(0.5 fps) - 0.002
 *              (Tracking.cc:866, 0.098 at 20 fps); timeCost_rest =
 *              select_s - timeCost_sofar.
 * Every cap is the reference's rule on the device's real-time clock
 * (s_memrealtime, 100 MHz ticks), each timer started where the reference
 * starts it, at the granularity given:
 *   isInFrustum loop (Tracking.cc:3251-3270): timer at the loop start; point i
 *     (skipping points matched this frame) cuts when its elapsed > match/2:
 *     points i.. go to mLeftMapPoints and leave mvpLocalMapPoints. Per point
 *     (a wave's 64 points read the clock once). time_Viz = the last value the
 *     loop compared.
 *   MAP_INFO build (Tracking.cc:3331 -> Observability.cc:564-578), cap
 *     (match - time_Viz)/2 on a timer started after the loop (:3311); per
 *     64-point batch.
 *   runActiveMapMatching (Tracking.cc:3343-3344 -> Observability.cc:1260,
 *     1275-1277, 1366-1370), cap match - time_Mat_Online - time_Viz (<= 0:
 *     the early exit); the clock is read at each round's start and the cut
 *     takes effect at that round's first accepted draw (where the reference
 *     first checks in a round): matches so far stand, no leftovers.
 *   timeCost_sofar from the frame's start (after the extraction gate wait,
 *     so queueing behind other front ends does not count).
 *   RunMapPointsSelection (Tracking.cc:1727-1779): returns when
 *     timeCost_rest <= 0, else MAP_INFO at kinematic[1] capped at
 *     timeCost_rest; per 64-point batch.
 *   SearchAdditionalMatchesInFrame (Tracking.cc:3097-3137): visibility pass
 *     cut at timeCost_rest/2 per list point (mLeftMapPoints erased from
 *     there); SearchByProjection_Budget (ORBmatcher.cc:281-282, 366-371)
 *     returns when timeCost_rest - time_so_far <= 0, else breaks after the
 *     first point that reaches its clock check with elapsed >= that
 *     (per point, elapsed from the matcher's start).
 * The elapsed values every rule compared are written to GF_FE_CLOCK, so a
 * CPU replay can apply the same rules (oracle/chain.cpp) and check the cut
 * positions rather than be told them. */
int gf_set_budgets(gf_ctx* ctx, double match_s, double select_s);

/* GF_FE_CLOCK record of one stream (int64 words, ticks of 10 ns; -1 = not
 * reached). M = map_cap, R = max(gf_budget, 1) (rounds <= num_to_match). */
enum {
    GF_CK_FLAGS = 0,    /* bit 0 match budget on, bit 1 select budget on   */
    GF_CK_MATCH,        /* time_total_match in ticks                        */
    GF_CK_SELECT,       /* select budget in ticks                           */
    GF_CK_VIZ_CUT,      /* isInFrustum: position of the cut (list size when none) */
    GF_CK_VIZ_TIME,     /* time_Viz                                         */
    GF_CK_MAT_ONLINE,   /* time_Mat_Online                                  */
    GF_CK_AM_CUT,       /* round at which the active-matching cap fired, -1 none */
    GF_CK_SOFAR,        /* timeCost_sofar                                   */
    GF_CK_SA_CUT,       /* visibility pass cut position in mLeftMapPoints (size when none) */
    GF_CK_SA_SOFAR,     /* time_so_far before SearchByProjection_Budget     */
    GF_CK_BUDGET_CUT,   /* list position SearchByProjection_Budget broke after, -1 none */
    GF_CK_HEADER = 16
};
#define GF_CK_OFF_VIZ(M, R) (GF_CK_HEADER)                       /* [M] isInFrustum, per list point  */
#define GF_CK_OFF_MI(M, R) (GF_CK_HEADER + (M))                  /* [64] MAP_INFO batches (active)    */
#define GF_CK_OFF_AM(M, R) (GF_CK_HEADER + (M) + 64)             /* [R] active-matching rounds        */
#define GF_CK_OFF_SEL(M, R) (GF_CK_HEADER + (M) + 64 + (R))      /* [64] MAP_INFO batches (kinematic[1]) */
#define GF_CK_OFF_SA(M, R) (GF_CK_HEADER + (M) + 128 + (R))      /* [M] visibility pass, per list point */
#define GF_CK_OFF_BUD(M, R) (GF_CK_HEADER + 2 * (M) + 128 + (R)) /* [M] SearchByProjection_Budget    */
#define GF_CK_WORDS(M, R) (GF_CK_HEADER + 3 * (M) + 128 + (R))
/* Test clock (test-only): every budget check reads base + idx * slope ticks
 * instead of the device clock, idx the check's position at its site (the
 * isInFrustum list point, the MAP_INFO 64-point batch, the active-matching
 * round, the SearchByProjection_Budget point; 0 for a site read once). With
 * it a chosen cap fires at a chosen point, so the budget rules are tested
 * without wall-clock luck; the clock record (GF_FE_CLOCK) holds the values
 * read, as with the device clock. base_slope: [GF_CK_NSITE][2] i64 ticks;
 * NULL restores the device clock. Set before a graph capture. */
enum {
    GF_CK_SITE_VIZ = 0,    /* isInFrustum loop, per list point (Tracking.cc:3262) */
    GF_CK_SITE_MI,         /* MAP_INFO batches of the active branch (Observability.cc:573) */
    GF_CK_SITE_AM_START,   /* time_Mat_Online at runActiveMapMatching's start (Tracking.cc:3311) */
    GF_CK_SITE_AM_ROUND,   /* runActiveMapMatching, per round (Observability.cc:1366) */
    GF_CK_SITE_SOFAR,      /* timeCost_sofar (Tracking.cc:866) */
    GF_CK_SITE_SEL,        /* RunMapPointsSelection's MAP_INFO batches (Tracking.cc:1779) */
    GF_CK_SITE_SA,         /* SearchAdditionalMatchesInFrame's visibility pass, per point (:3107-3119) */
    GF_CK_SITE_SA_SOFAR,   /* time_so_far before SearchByProjection_Budget (:3131) */
    GF_CK_SITE_BUD,        /* SearchByProjection_Budget, per point (ORBmatcher.cc:366) */
    GF_CK_NSITE
};
int gf_frontend_set_test_clock(gf_frontend* fe, const long long* base_slope);

/* Per-frame stage log: Tracking::logCurrentFrame / SaveTimeLog
 * (Tracking.h:254-280, filled at Tracking.cc:528, 605-615, 672, 913,
 * 2808-2814, 3143, 3339). With a log of `steps` entries on, each step
 * records the device real-time clock (s_memrealtime, 100 MHz) at its stage
 * boundaries (one 1-thread launch per boundary on the step's stream) and,
 * per stream, the counts the reference's landmark columns are made of; the
 * last `steps` steps are kept in a ring. The stages are batched: a boundary
 * is where the whole batch crossed it, so a column is the batch's time in
 * that stage, which every stream of the batch shares. Off (steps = 0) by
 * default: the step then launches nothing for it. Not while a captured graph
 * exists (capture again after changing it). */
enum {
    GF_TL_BEGIN = 0,     /* the frame's start, after the extraction gate         */
    GF_TL_EXTRACTED,     /* ORB extraction (+ undistortion) done                 */
    GF_TL_MOTION,        /* TrackWithMotionModel: SearchByProjection(Cur, Last) + PoseOptimization */
    GF_TL_INIT_POSE,     /* + TrackPreviousFrame / Relocalisation, outlier discard */
    GF_TL_REF_UPDATED,   /* TrackLocalMap: UpdateReference                       */
    GF_TL_FRUSTUM,       /* SearchReferencePointsInFrustum: FRAME_INFO, isInFrustum */
    GF_TL_MAT_ONLINE,    /* MAP_INFO_MATRIX (runMatrixBuilding, time_Mat_Online) */
    GF_TL_SELECTED,      /* runActiveMapMatching                                 */
    GF_TL_SEARCHED,      /* SearchByProjection(F, local) (end of SearchReferencePointsInFrustum) */
    GF_TL_OPTIMISED,     /* PoseOptimization + statistics (end of TrackLocalMap)  */
    GF_TL_END,           /* motion update, PWLS prediction, RunMapPointsSelection, SearchAdditionalMatchesInFrame, mLastFrame */
    GF_TL_NSITE = 12
};
typedef struct gf_time_rec {
    double frame_time_stamp; /* mCurrentFrame.mTimeStamp                          */
    int32_t path;            /* GF_TR_PATH of the step                             */
    int32_t branch;          /* GF_ST_BRANCH                                       */
    int32_t found;           /* GF_ST_FOUND: TrackWithMotionModel's nmatches        */
    int32_t tpf;             /* GF_ST_TPF: TrackPreviousFrame's nmatches            */
    int32_t local;           /* GF_ST_LOCAL                                        */
    int32_t inliers;         /* GF_ST_INL2: mnMatchesInliers                       */
    int32_t extra;           /* GF_ST_EXTRA                                        */
    int32_t track_map;       /* 1: TrackLocalMap ran                               */
    int32_t flags;           /* GF_ST_FLAGS                                        */
    int32_t step;            /* the front end's step counter of the record         */
} gf_time_rec;
int gf_frontend_set_time_log(gf_frontend* fe, int steps);
/* The ring in step order, oldest first: stamps [n][GF_TL_NSITE] i64 ticks
 * (0: not reached), recs [n][B]; n (<= steps) returned in *nsteps. */
int gf_frontend_read_time_log(gf_frontend* fe, long long* stamps, gf_time_rec* recs, int* nsteps);

/* ------------------------------------------------ multi-GPU start-up exchange
 * Config 5: one process per GPU, sequences independent,
 * and one exchange step before tracking: an RCCL communicator over xGMI and
 * broadcasts from rank 0 of the shared state. The reference has no
 * distributed layer (one process, main.cc:92-157); the vocabulary it loads
 * once (main.cc:92-106, TemplatedVocabulary.h:1469-1536) and the map it
 * tracks against are what every rank receives. The communicator uses the
 * context's device and stream; calls are synchronous. */
typedef struct gf_dist gf_dist;
/* ncclGetUniqueId on one rank (128 bytes); the caller hands it to the others. */
int gf_dist_unique_id(uint8_t* id);
int gf_dist_init(gf_ctx* ctx, int rank, int world, const uint8_t* id, gf_dist** out);
int gf_dist_destroy(gf_dist* d);
int gf_dist_info(gf_dist* d, int* rank, int* world);
/* Other transports behind the same entry points (gf_dist_bcast / _allreduce /
 * _bcast_vocab / _bcast_map work unchanged on them):
 * - loopback: the ranks are host threads of one process, each with its own
 *   context, meeting in a channel of `world` ranks; a broadcast is a
 *   rendezvous and a device-to-device copy from the root's buffer, an
 *   all-reduce a rank-ordered host reduction. Every rank's call blocks until
 *   all ranks have made the same call (120 s timeout, then GF_ERR_HIP and a
 *   broken channel). One GPU runs the receiving side of config 5 this way.
 * - host-staged: device -> host, fn(user, op, host_buf, bytes, root) does the
 *   collective on host memory (op GF_DIST_OP_BCAST from root; GF_DIST_OP_SUM /
 *   _MAX / _MIN in place over bytes / 8 doubles, root -1) and returns 0,
 *   host -> device. For processes that share a GPU (a gloo group). */
enum { GF_DIST_RCCL = 0, GF_DIST_LOOPBACK = 1, GF_DIST_HOST = 2 };
enum { GF_DIST_OP_BCAST = 0, GF_DIST_OP_SUM = 1, GF_DIST_OP_MAX = 2, GF_DIST_OP_MIN = 3 };
typedef struct gf_dist_channel gf_dist_channel;
typedef int (*gf_dist_host_fn)(void* user, int op, void* host_buf, size_t bytes, int root);
int gf_dist_channel_create(int world, gf_dist_channel** out);
int gf_dist_channel_destroy(gf_dist_channel* ch);
int gf_dist_init_loopback(gf_ctx* ctx, int rank, gf_dist_channel* ch, gf_dist** out);
int gf_dist_init_host(gf_ctx* ctx, int rank, int world, gf_dist_host_fn fn, void* user, gf_dist** out);
/* GF_DIST_RCCL / _LOOPBACK / _HOST */
int gf_dist_transport(gf_dist* d, int* transport);
/* Device buffer broadcast from root. */
int gf_dist_bcast(gf_dist* d, void* d_buf, size_t bytes, int root);
/* In-place all-reduce of n doubles: op 0 sum, 1 max, 2 min. */
int gf_dist_allreduce(gf_dist* d, double* d_buf, size_t n, int op);
/* The vocabulary of root into every rank (*voc == NULL on the others: a
 * vocabulary is created on the communicator's device). */
int gf_dist_bcast_vocab(gf_dist* d, gf_vocab** voc, int root);
/* Every stream's local map (gf_frontend_set_map state) of root's front end
 * into the same-shaped front ends of the other ranks. */
int gf_dist_bcast_map(gf_dist* d, gf_frontend* fe, int root);
/* Host copy of a device vocabulary's node arrays (any may be NULL). */
int gf_vocab_download(gf_vocab* voc, uint8_t* desc, double* weight, int32_t* word, int32_t* cstart);

#ifdef __cplusplus
}
#endif
#endif /* GFSLAM_ABI_H */
