// LocalMapping::CreateNewMapPoints on gfx950 (src/LocalMapping.cc:243-409,
// ComputeF12 :490-507, KeyFrame::ComputeSceneMedianDepth KeyFrame.cc:659-689):
// the new keyframe against its covisible neighbours as a chain of launches
// on one stream, with no host-read value in between.
//   k_np_setup        one workgroup per neighbour, one launch for all: the
//                     scene median depth as the (n-1)/2-th smallest depth by a
//                     4-pass radix select over order-preserving keys in LDS,
//                     the baseline test (:270-281) and F12; it writes F into
//                     the neighbour's matcher pair, or empties the pair when
//                     the neighbour is skipped;
//   k_search_tri      (bow.hip) SearchForTriangulation of (new keyframe,
//                     neighbour i), reading the new keyframe's slot table as
//                     the previous triangulation launch left it;
//   k_np_triangulate  one workgroup: the matches compacted in keypoint order
//                     (vMatchedIndices), one lane per match for the body
//                     (:307-390: rays, the 4x4 float Jacobi SVD in registers,
//                     depth / reprojection / scale tests), the accepted ones
//                     numbered by a workgroup scan, their ids written into
//                     both slot tables and the device counter advanced.
// Arithmetic: float, -ffp-contract=off, correctly rounded div/sqrt; the
// OpenCV readings are docs/ORACLE_ASSUMPTIONS.md A27 (A1 / A17 / A22).
// Parity: bit-exact against tests/helpers/localmap_ref.cpp.
#include <algorithm>
#include <cstring>
#include <vector>

#include "common.h"
#include "cvsvd_core.h"
#include "depthselect.h"

namespace {

using namespace gfcv;

constexpr int NP_MAX = 4096;  // keypoints per keyframe
constexpr int NP_T = 512;     // k_np_triangulate workgroup (256 VGPRs a lane: the SVD does not spill)
constexpr int NP_PER = NP_MAX / NP_T;
constexpr int NP_ST = 256;    // k_np_setup workgroup

struct NpCam {
    float fx, fy, cx, cy;
    float scale_factor;
    int nlevels;
    float sf[16];      // mvScaleFactors
    float sigma2[16];  // mvLevelSigma2
};

struct NpKf {
    float Tcw[16];
    int32_t* mp;
    const gf_keypoint* kps;
    int32_t n;
};

// Ow = -Rcw^T tcw (KeyFrame::SetPose; A1 product, A17 scale)
__device__ void camera_center(const float* T, float* Ow) {
    const float R[9] = {T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10]};
    const float t[3] = {T[3], T[7], T[11]};
    float Rt[9];
    transpose3(R, Rt);
    gemm_f<3, 3, 1>(Rt, t, Ow, -1.0);
}

// ComputeF12 (:490-507)
__device__ void compute_f12(const NpCam& cam, const float* T1, const float* T2, float* F) {
    const float R1[9] = {T1[0], T1[1], T1[2], T1[4], T1[5], T1[6], T1[8], T1[9], T1[10]};
    const float R2[9] = {T2[0], T2[1], T2[2], T2[4], T2[5], T2[6], T2[8], T2[9], T2[10]};
    const float t1[3] = {T1[3], T1[7], T1[11]}, t2[3] = {T2[3], T2[7], T2[11]};
    float R2t[9], R12[9], M[9], t12[3];
    transpose3(R2, R2t);
    gemm_f<3, 3, 3>(R1, R2t, R12);
    gemm_f<3, 3, 3>(R1, R2t, M, -1.0);  // -R1w*R2w.t()
    for (int r = 0; r < 3; r++) t12[r] = ((M[3 * r] * t2[0] + M[3 * r + 1] * t2[1]) + M[3 * r + 2] * t2[2]) + t1[r];
    const float tx[9] = {0.f, -t12[2], t12[1], t12[2], 0.f, -t12[0], -t12[1], t12[0], 0.f};
    const float K[9] = {cam.fx, 0.f, cam.cx, 0.f, cam.fy, cam.cy, 0.f, 0.f, 1.f};
    float Kt[9], Kti[9], Ki[9], A[9], B[9];
    transpose3(K, Kt);
    inv3(Kt, Kti);
    inv3(K, Ki);
    gemm_f<3, 3, 3>(Kti, tx, A);
    gemm_f<3, 3, 3>(A, R12, B);
    gemm_f<3, 3, 3>(B, Ki, F);
}

__global__ __launch_bounds__(NP_ST) void k_np_setup(NpCam cam, NpKf cur, const NpKf* __restrict__ nk,
                                                    gf::TriPairDev* __restrict__ pairs,
                                                    const float* __restrict__ mp_pos, int nmp,
                                                    gf_newpoints_neigh* __restrict__ rep) {
    __shared__ uint32_t keys[NP_MAX];
    __shared__ int hist[256];
    __shared__ uint32_t s_prefix;
    __shared__ int s_rank, s_cnt;
    const int i = blockIdx.x, tid = threadIdx.x;
    const NpKf& K = nk[i];
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    // ComputeSceneMedianDepth(2): z = (float)(Rcw.row(2).dot(x3Dw) + zcw) of every non-NULL slot
    const int n2 = min(K.n, NP_MAX);
    for (int j = tid; j < n2; j += NP_ST) {
        const int m = K.mp[j];
        if (m < 0 || m >= nmp) continue;
        keys[atomicAdd(&s_cnt, 1)] = ord_key(gfsel::scene_depth(K.Tcw, mp_pos + 3 * (size_t)m));
    }
    __syncthreads();
    const int nd = s_cnt;
    // the element std::sort puts at (n-1)/2
    if (nd > 0) gfsel::radix_select<NP_ST>(keys, nd, (nd - 1) / 2, hist, &s_prefix, &s_rank);
    if (tid != 0) return;
    gf_newpoints_neigh R;
    R.status = GF_NP_OK;
    for (int q = 0; q < 9; q++) R.F12[q] = 0.f;
    R.median_depth = 0.f;
    R.nmatches = 0;
    R.naccepted = 0;
    if (nd == 0) {
        R.status = GF_NP_NODEPTH;
    } else {
        float Ow1[3], Ow2[3], vb[3];
        camera_center(cur.Tcw, Ow1);
        camera_center(K.Tcw, Ow2);
        for (int r = 0; r < 3; r++) vb[r] = Ow2[r] - Ow1[r];
        const float baseline = (float)norm3(vb);
        R.median_depth = key_val(s_prefix);
        const float ratio = baseline / R.median_depth;
        if ((double)ratio < 0.01) R.status = GF_NP_BASELINE;
        else compute_f12(cam, cur.Tcw, K.Tcw, R.F12);
    }
    rep[i] = R;
    gf::TriPairDev& P = pairs[i];
    if (R.status == GF_NP_OK) {
        for (int q = 0; q < 9; q++) P.F[q] = R.F12[q];
    } else {  // the matcher launch of a skipped neighbour finds nothing to do
        P.a.n = 0;
        P.a.nfv = 0;
        P.b.nfv = 0;
    }
}

// exclusive scan of one int per lane over the workgroup (NP_T lanes); sw: NP_T/64 + 1 ints
__device__ __forceinline__ int block_scan(int v, int* sw, int& total) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (lane == 63) sw[w] = inc;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int q = 0; q < NP_T / 64; q++) {
            const int t = sw[q];
            sw[q] = run;
            run += t;
        }
        sw[NP_T / 64] = run;
    }
    __syncthreads();
    const int r = sw[w] + inc - v;
    total = sw[NP_T / 64];
    __syncthreads();
    return r;
}

__device__ __forceinline__ double dot3d(const float* a, const float* b) {  // Mat::dot: double accumulation
    double s = 0;
#pragma unroll
    for (int r = 0; r < 3; r++) s += (double)a[r] * (double)b[r];
    return s;
}

// one match of :307-390; x3D is written once the point is triangulated
__device__ int np_match(const NpCam& cam, const float* T1, const float* T2, const float* Ow1, const float* Ow2,
                        const gf_keypoint& kp1, const gf_keypoint& kp2, float* x3D) {
    const float invfx = 1.0f / cam.fx, invfy = 1.0f / cam.fy;
    const float xn1[3] = {(kp1.x - cam.cx) * invfx, (kp1.y - cam.cy) * invfy, 1.f};
    const float xn2[3] = {(kp2.x - cam.cx) * invfx, (kp2.y - cam.cy) * invfy, 1.f};
    float ray1[3], ray2[3];
#pragma unroll
    for (int r = 0; r < 3; r++) {  // Rwc * xn, Rwc = Rcw^T
        ray1[r] = (T1[r] * xn1[0] + T1[4 + r] * xn1[1]) + T1[8 + r] * xn1[2];
        ray2[r] = (T2[r] * xn2[0] + T2[4 + r] * xn2[1]) + T2[8 + r] * xn2[2];
    }
    const float cosPar = (float)(dot3d(ray1, ray2) / (norm3(ray1) * norm3(ray2)));
    if (cosPar < 0 || (double)cosPar > 0.9998) return GF_NP_EXIT_PARALLAX;
    float Am[16];
    auto row = [&](float x, const float* T, int r, float* out) {
#pragma unroll
        for (int c = 0; c < 4; c++)
            out[c] = (float)((double)T[8 + c] * (double)x + (double)T[4 * r + c] * -1.0 + 0.0);
    };
    row(xn1[0], T1, 0, Am);
    row(xn1[1], T1, 1, Am + 4);
    row(xn2[0], T2, 0, Am + 8);
    row(xn2[1], T2, 1, Am + 12);
    float Ta[16], w[4], vt[16];
    svd_f<4, 4, false>(Am, Ta, w, nullptr, vt);
    if (vt[15] == 0) return GF_NP_EXIT_W0;
    scale3(vt + 12, 1.0 / (double)vt[15], x3D);
    const float z1 = (float)(dot3d(T1 + 8, x3D) + (double)T1[11]);
    if (z1 <= 0) return GF_NP_EXIT_Z1;
    const float z2 = (float)(dot3d(T2 + 8, x3D) + (double)T2[11]);
    if (z2 <= 0) return GF_NP_EXIT_Z2;
    const int o1 = min(max(kp1.octave, 0), cam.nlevels - 1), o2 = min(max(kp2.octave, 0), cam.nlevels - 1);
    {
        const float x1 = (float)(dot3d(T1, x3D) + (double)T1[3]);
        const float y1 = (float)(dot3d(T1 + 4, x3D) + (double)T1[7]);
        const float invz1 = (float)(1.0 / (double)z1);
        const float u1 = cam.fx * x1 * invz1 + cam.cx, v1 = cam.fy * y1 * invz1 + cam.cy;
        const float ex = u1 - kp1.x, ey = v1 - kp1.y;
        if ((double)(ex * ex + ey * ey) > 5.991 * (double)cam.sigma2[o1]) return GF_NP_EXIT_REPROJ1;
    }
    {
        const float x2 = (float)(dot3d(T2, x3D) + (double)T2[3]);
        const float y2 = (float)(dot3d(T2 + 4, x3D) + (double)T2[7]);
        const float invz2 = (float)(1.0 / (double)z2);
        const float u2 = cam.fx * x2 * invz2 + cam.cx, v2 = cam.fy * y2 * invz2 + cam.cy;
        const float ex = u2 - kp2.x, ey = v2 - kp2.y;
        if ((double)(ex * ex + ey * ey) > 5.991 * (double)cam.sigma2[o2]) return GF_NP_EXIT_REPROJ2;
    }
    const float n1v[3] = {x3D[0] - Ow1[0], x3D[1] - Ow1[1], x3D[2] - Ow1[2]};
    const float n2v[3] = {x3D[0] - Ow2[0], x3D[1] - Ow2[1], x3D[2] - Ow2[2]};
    const float dist1 = (float)norm3(n1v), dist2 = (float)norm3(n2v);
    if (dist1 == 0 || dist2 == 0) return GF_NP_EXIT_DIST0;
    const float ratioDist = dist1 / dist2;
    const float ratioOctave = cam.sf[o1] / cam.sf[o2];
    const float ratioFactor = 1.5f * cam.scale_factor;
    if (ratioDist * ratioFactor < ratioOctave || ratioDist > ratioOctave * ratioFactor) return GF_NP_EXIT_SCALE;
    return GF_NP_EXIT_ACCEPTED;
}

__global__ __launch_bounds__(NP_T) void k_np_triangulate(NpCam cam, NpKf cur, const NpKf* __restrict__ nk, int i,
                                                         const int32_t* __restrict__ matches, int nmp, int cap,
                                                         gf_newpoints_neigh* __restrict__ rep,
                                                         gf_newpoint* __restrict__ points,
                                                         int32_t* __restrict__ exits, float* __restrict__ tmp,
                                                         int32_t* total) {
    __shared__ uint16_t s_i1[NP_MAX], s_i2[NP_MAX];
    __shared__ int sw[NP_T / 64 + 1];
    const int tid = threadIdx.x;
    const NpKf& K2 = nk[i];
    const int n1 = min(cur.n, NP_MAX);
    int32_t* ex = exits + (size_t)i * cur.n;
    if (rep[i].status != GF_NP_OK) {  // skipped neighbour: set-up already reported 0 matches
        for (int j = tid; j < n1; j += NP_T) ex[j] = -1;
        return;
    }
    const int base = *total;
    // vMatchedIndices: the matched keypoints in ascending idx1
    int m[NP_PER], cnt = 0;
#pragma unroll
    for (int k = 0; k < NP_PER; k++) {
        const int idx1 = NP_PER * tid + k;
        m[k] = -1;
        if (idx1 < n1) {
            const int v = matches[idx1];
            if (v >= 0 && v < K2.n) m[k] = v;
            else ex[idx1] = -1;
        }
        cnt += m[k] >= 0;
    }
    int nm;
    int off = block_scan(cnt, sw, nm);
#pragma unroll
    for (int k = 0; k < NP_PER; k++)
        if (m[k] >= 0) {
            s_i1[off] = (uint16_t)(NP_PER * tid + k);
            s_i2[off] = (uint16_t)m[k];
            off++;
        }
    __syncthreads();
    // one lane per match while there are at most NP_T of them; a lane's matches are consecutive, so
    // the accepted ones are numbered by a scan of the lanes' counts. The positions wait in `tmp`
    // (each lane reads back only what it wrote): no per-lane array, the body is instantiated once.
    const int chunk = (nm + NP_T - 1) / NP_T;
    float Ow1[3], Ow2[3];
    camera_center(cur.Tcw, Ow1);
    camera_center(K2.Tcw, Ow2);
    int na_l = 0;
    for (int k = 0; k < chunk; k++) {
        const int j = tid * chunk + k;
        if (j >= nm) break;
        const int idx1 = s_i1[j], idx2 = s_i2[j];
        float p[3] = {0.f, 0.f, 0.f};
        const int e = np_match(cam, cur.Tcw, K2.Tcw, Ow1, Ow2, cur.kps[idx1], K2.kps[idx2], p);
        ex[idx1] = e;
        if (e == GF_NP_EXIT_ACCEPTED) {
            tmp[3 * j] = p[0];
            tmp[3 * j + 1] = p[1];
            tmp[3 * j + 2] = p[2];
            na_l++;
        } else {
            s_i2[j] = 0xffff;  // not accepted (a keypoint index is < 4096)
        }
    }
    int na;
    int r = base + block_scan(na_l, sw, na);
    for (int k = 0; k < chunk; k++) {
        const int j = tid * chunk + k;
        if (j >= nm) break;
        const int idx1 = s_i1[j], idx2 = s_i2[j];
        if (idx2 == 0xffff) continue;
        if (r < cap) {
            gf_newpoint P;
            P.neighbour = i;
            P.idx1 = idx1;
            P.idx2 = idx2;
            P.pos[0] = tmp[3 * j];
            P.pos[1] = tmp[3 * j + 1];
            P.pos[2] = tmp[3 * j + 2];
            points[r] = P;
        }
        cur.mp[idx1] = nmp + r;  // AddMapPoint (:398-399)
        K2.mp[idx2] = nmp + r;
        r++;
    }
    if (tid == 0) {
        rep[i].nmatches = nm;
        rep[i].naccepted = na;
        *total = base + na;
    }
}

NpCam make_cam(const gf_frame_info* fi) {
    NpCam c{};
    c.fx = fi->fx;
    c.fy = fi->fy;
    c.cx = fi->cx;
    c.cy = fi->cy;
    c.scale_factor = fi->scale_factor;
    c.nlevels = fi->nlevels;
    c.sf[0] = 1.f;
    for (int l = 1; l < fi->nlevels; l++) c.sf[l] = c.sf[l - 1] * fi->scale_factor;
    for (int l = 0; l < fi->nlevels; l++) c.sigma2[l] = c.sf[l] * c.sf[l];
    return c;
}

size_t al16(size_t x) { return (x + 15) & ~(size_t)15; }

int check_kf(const gf_newpoints_kf& k) {
    GF_CHECK(k.side.n >= 0 && k.side.n <= NP_MAX && k.side.nfv >= 0 && k.side.nfv <= k.side.n, GF_ERR_UNSUPPORTED,
             "at most 4096 keypoints per keyframe");
    GF_CHECK(k.side.n == 0 || (k.mp && k.side.fv_nodes && k.side.fv_start && k.side.fv_feats && k.side.desc &&
                               k.side.kps),
             GF_ERR_ARG, "null keyframe array");
    return GF_OK;
}

}  // namespace

extern "C" {

int gf_create_new_map_points_dev(gf_ctx* ctx, const gf_frame_info* fi, const gf_newpoints_kf* cur, int nneigh,
                                 const gf_newpoints_kf* neigh, const float* d_mp_pos, int nmp, int check_ori,
                                 int cap, gf_newpoints_neigh* d_report, gf_newpoint* d_points, int32_t* d_exits,
                                 int32_t* d_total, void* stream) {
    GF_CHECK(ctx && fi && cur && d_total, GF_ERR_ARG, "null arg");
    GF_CHECK(nneigh >= 0 && nneigh <= GF_NEWPTS_MAX_NEIGH, GF_ERR_UNSUPPORTED, "at most 20 neighbours");
    GF_CHECK(fi->nlevels >= 1 && fi->nlevels <= 16, GF_ERR_ARG, "nlevels must be in 1..16");
    GF_CHECK(cap >= 0 && nmp >= 0, GF_ERR_ARG, "negative cap / nmp");
    hipStream_t s = (hipStream_t)stream;
    GF_HIP(hipMemsetAsync(d_total, 0, sizeof(int32_t), s));
    if (nneigh == 0) return GF_OK;
    GF_CHECK(neigh && d_report && (cap == 0 || d_points) && (nmp == 0 || d_mp_pos), GF_ERR_ARG, "null arg");
    int rc = check_kf(*cur);
    if (rc) return rc;
    GF_CHECK(cur->side.n == 0 || d_exits, GF_ERR_ARG, "null exits");
    for (int i = 0; i < nneigh; i++)
        if ((rc = check_kf(neigh[i]))) return rc;
    const NpCam cam = make_cam(fi);
    const int n1 = cur->side.n;
    // scratch: the matcher pairs, the neighbour views, vMatches12 per neighbour, the matcher's counts
    // and the positions of one neighbour's matches
    const size_t o_pairs = 0, o_nk = al16(o_pairs + sizeof(gf::TriPairDev) * nneigh),
                 o_match = al16(o_nk + sizeof(NpKf) * nneigh),
                 o_nm = al16(o_match + sizeof(int32_t) * (size_t)nneigh * std::max(n1, 1)),
                 o_tmp = al16(o_nm + sizeof(int32_t) * nneigh), bytes = o_tmp + 12 * (size_t)NP_MAX;
    void* ws;
    if ((rc = gf::ws_get(ctx, 64, bytes, &ws))) return rc;
    uint8_t* base = (uint8_t*)ws;
    gf::TriPairDev* d_pairs = (gf::TriPairDev*)(base + o_pairs);
    NpKf* d_nk = (NpKf*)(base + o_nk);
    int32_t* d_match = (int32_t*)(base + o_match);
    int32_t* d_nm = (int32_t*)(base + o_nm);
    std::vector<uint8_t> h(o_match, 0);
    gf::TriPairDev* hp = (gf::TriPairDev*)(h.data() + o_pairs);
    NpKf* hk = (NpKf*)(h.data() + o_nk);
    NpKf kc{};
    memcpy(kc.Tcw, cur->Tcw, sizeof(kc.Tcw));
    kc.mp = cur->mp;
    kc.kps = cur->side.kps;
    kc.n = n1;
    for (int i = 0; i < nneigh; i++) {
        gf::TriPairDev T{};
        T.a = cur->side;
        T.a.mp = cur->mp;
        T.b = neigh[i].side;
        T.b.mp = neigh[i].mp;
        for (int l = 0; l < fi->nlevels; l++) T.sigma2[l] = cam.sigma2[l];
        T.nlevels = fi->nlevels;
        T.out = d_match + (size_t)i * std::max(n1, 1);
        hp[i] = T;
        NpKf K{};
        memcpy(K.Tcw, neigh[i].Tcw, sizeof(K.Tcw));
        K.mp = neigh[i].mp;
        K.kps = neigh[i].side.kps;
        K.n = neigh[i].side.n;
        hk[i] = K;
    }
    GF_HIP(hipMemcpyAsync(base, h.data(), o_match, hipMemcpyHostToDevice, s));
    {
        GF_PROF(ctx, s, "k_np_setup");
        GF_LAUNCH(k_np_setup, nneigh, NP_ST, 0, s, cam, kc, (const NpKf*)d_nk, d_pairs, d_mp_pos, nmp, d_report);
        GF_HIP(hipGetLastError());
    }
    for (int i = 0; i < nneigh; i++) {
        if ((rc = gf::search_tri_pairs(ctx, check_ori, 1, d_pairs + i, d_nm + i, s))) return rc;
        GF_PROF(ctx, s, "k_np_triangulate");
        GF_LAUNCH(k_np_triangulate, 1, NP_T, 0, s, cam, kc, (const NpKf*)d_nk, i,
                  (const int32_t*)(d_match + (size_t)i * std::max(n1, 1)), nmp, cap, d_report, d_points, d_exits,
                  (float*)(base + o_tmp), d_total);
        GF_HIP(hipGetLastError());
    }
    return GF_OK;
}

int gf_create_new_map_points(gf_ctx* ctx, const gf_frame_info* fi, const gf_newpoints_kf* cur, int nneigh,
                             const gf_newpoints_kf* neigh, const float* mp_pos, int nmp, int check_ori, int cap,
                             gf_newpoints_neigh* report, gf_newpoint* points, int32_t* exits, int* total) {
    GF_CHECK(ctx && fi && cur && total, GF_ERR_ARG, "null arg");
    GF_CHECK(nneigh >= 0 && nneigh <= GF_NEWPTS_MAX_NEIGH, GF_ERR_UNSUPPORTED, "at most 20 neighbours");
    GF_CHECK(cap >= 0 && nmp >= 0, GF_ERR_ARG, "negative cap / nmp");
    *total = 0;
    if (nneigh == 0) return GF_OK;
    GF_CHECK(neigh && report && (cap == 0 || points) && (nmp == 0 || mp_pos), GF_ERR_ARG, "null arg");
    int rc = check_kf(*cur);
    if (rc) return rc;
    GF_CHECK(cur->side.n == 0 || exits, GF_ERR_ARG, "null exits");
    for (int i = 0; i < nneigh; i++)
        if ((rc = check_kf(neigh[i]))) return rc;
    GF_HIP(hipSetDevice(ctx->device));
    // one staging block (slot 65): the keyframes' arrays, the positions, the outputs
    size_t off = 0;
    std::vector<std::pair<const void*, size_t>> parts;
    auto add = [&](const void* hsrc, size_t bytes) {
        const size_t o = off;
        parts.push_back({hsrc, bytes});
        off += al16(bytes);
        return o;
    };
    struct KfOff {
        size_t nodes, start, feats, desc, kps, mp;
    };
    auto add_kf = [&](const gf_newpoints_kf& k) {
        const gf_bow_side& sd = k.side;
        KfOff o;
        o.nodes = add(sd.fv_nodes, 4 * (size_t)sd.nfv);
        o.start = add(sd.n ? sd.fv_start : nullptr, sd.n ? 4 * (size_t)(sd.nfv + 1) : 0);
        o.feats = add(sd.fv_feats, 4 * (size_t)sd.n);
        o.desc = add(sd.desc, 32 * (size_t)sd.n);
        o.kps = add(sd.kps, sizeof(gf_keypoint) * (size_t)sd.n);
        o.mp = add(k.mp, 4 * (size_t)sd.n);
        return o;
    };
    std::vector<KfOff> ko(nneigh + 1);
    ko[0] = add_kf(*cur);
    for (int i = 0; i < nneigh; i++) ko[i + 1] = add_kf(neigh[i]);
    const int n1 = cur->side.n;
    const size_t o_pos = add(mp_pos, 12 * (size_t)nmp), o_rep = add(nullptr, sizeof(gf_newpoints_neigh) * nneigh),
                 o_pts = add(nullptr, sizeof(gf_newpoint) * (size_t)cap),
                 o_ex = add(nullptr, 4 * (size_t)nneigh * n1), o_tot = add(nullptr, 4);
    void* dbuf;
    if ((rc = gf::ws_get(ctx, 65, std::max(off, (size_t)16), &dbuf))) return rc;
    uint8_t* base = (uint8_t*)dbuf;
    size_t c = 0;
    for (auto& pr : parts) {
        if (pr.first && pr.second)
            GF_HIP(hipMemcpyAsync(base + c, pr.first, pr.second, hipMemcpyHostToDevice, ctx->stream));
        c += al16(pr.second);
    }
    auto dev_kf = [&](const gf_newpoints_kf& k, const KfOff& o) {
        gf_newpoints_kf d = k;
        d.side.fv_nodes = (const int32_t*)(base + o.nodes);
        d.side.fv_start = (const int32_t*)(base + o.start);
        d.side.fv_feats = (const int32_t*)(base + o.feats);
        d.side.desc = base + o.desc;
        d.side.kps = (const gf_keypoint*)(base + o.kps);
        d.side.mp = nullptr;
        d.mp = (int32_t*)(base + o.mp);
        return d;
    };
    const gf_newpoints_kf dcur = dev_kf(*cur, ko[0]);
    std::vector<gf_newpoints_kf> dn(nneigh);
    for (int i = 0; i < nneigh; i++) dn[i] = dev_kf(neigh[i], ko[i + 1]);
    rc = gf_create_new_map_points_dev(ctx, fi, &dcur, nneigh, dn.data(), (const float*)(base + o_pos), nmp, check_ori,
                                      cap, (gf_newpoints_neigh*)(base + o_rep), (gf_newpoint*)(base + o_pts),
                                      (int32_t*)(base + o_ex), (int32_t*)(base + o_tot), ctx->stream);
    if (rc) return rc;
    // everything comes back in one go; the caller's buffers are written after the single sync, and only
    // as far as the results reach (points[total..cap) and, on GF_ERR_CAP, the slot tables stay as they were)
    int32_t tot = 0;
    std::vector<gf_newpoint> hpts(cap);
    std::vector<std::vector<int32_t>> hmp(nneigh + 1);
    GF_HIP(hipMemcpyAsync(&tot, base + o_tot, 4, hipMemcpyDeviceToHost, ctx->stream));
    GF_HIP(hipMemcpyAsync(report, base + o_rep, sizeof(gf_newpoints_neigh) * nneigh, hipMemcpyDeviceToHost,
                          ctx->stream));
    if (n1) GF_HIP(hipMemcpyAsync(exits, base + o_ex, 4 * (size_t)nneigh * n1, hipMemcpyDeviceToHost, ctx->stream));
    if (cap)
        GF_HIP(hipMemcpyAsync(hpts.data(), base + o_pts, sizeof(gf_newpoint) * (size_t)cap, hipMemcpyDeviceToHost,
                              ctx->stream));
    for (int i = 0; i <= nneigh; i++) {
        const gf_newpoints_kf& d = i ? dn[i - 1] : dcur;
        hmp[i].resize(d.side.n);
        if (d.side.n)
            GF_HIP(hipMemcpyAsync(hmp[i].data(), d.mp, 4 * (size_t)d.side.n, hipMemcpyDeviceToHost, ctx->stream));
    }
    GF_HIP(hipStreamSynchronize(ctx->stream));
    *total = tot;
    if (tot > cap) return gf::fail(GF_ERR_CAP, "more new map points than cap");
    if (tot) memcpy(points, hpts.data(), sizeof(gf_newpoint) * (size_t)tot);
    for (int i = 0; i <= nneigh; i++) {
        const gf_newpoints_kf& k = i ? neigh[i - 1] : *cur;
        if (k.side.n) memcpy(k.mp, hmp[i].data(), 4 * (size_t)k.side.n);
    }
    return GF_OK;
}

}  // extern "C"
