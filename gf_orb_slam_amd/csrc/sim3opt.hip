// Optimizer::OptimizeSim3 (src/Optimizer.cc:2019-2215) on gfx950: the
// refinement of a loop candidate's Sim3 that LoopClosing::ComputeSim3 accepts
// or rejects the candidate by (LoopClosing.cc:335-339).
//
// One wave per problem (a keyframe pair), lanes over the matched pairs, SO_P
// pairs per pass. Each pair carries two edges, EdgeSim3ProjectXYZ (KF2's point
// into image 1) and EdgeInverseSim3ProjectXYZ (KF1's point into image 2); this
// g2o has no analytic Jacobian for either, so a linearisation is
// BaseBinaryEdge's central difference over 14 perturbed estimates. Those do
// not depend on the edge: lanes 0..14 build them (and their inverses) once per
// linearisation in LDS and every edge reads them. The sums over edges keep the
// reference's order: lane k owns accumulator k (28 lower H entries, 7 b
// entries, robust chi2) and adds the per-edge terms staged in LDS in the
// active-edge order, as in poseopt_core.h. The scalar LM logic (lambda
// schedule, 7x7 LDLT, exponential update, stop rules) runs redundantly on
// every lane from the shared sums. Every loop is bounded by the iteration and
// trial counts (at most 15 iterations of at most 10 trials).
//
// Reference: OptimizationAlgorithmLevenberg::solve
// core/optimization_algorithm_levenberg.cpp:61-164, BaseBinaryEdge
// core/base_binary_edge.hpp:55-122 and :147-196, g2o::Sim3
// types/sim3/sim3.h:70-142, :233, :266, the edges
// types/sim3/types_seven_dof_expmap.h:130-171.
#include "sim3opt_core.h"

#include <algorithm>
#include <vector>

namespace {
using namespace gfsim3opt;

__global__ __launch_bounds__(SO_T) void k_sim3_opt(Sim3OptArgs A) { sim3_opt_problem(A, blockIdx.x); }

}  // namespace

extern "C" {

int gf_optimize_sim3_dev(gf_ctx* ctx, int nprob, const float* d_X1, const float* d_X2, const float* d_z1,
                         const float* d_z2, const float* d_w1, const float* d_w2, const int32_t* d_offsets,
                         const float* d_K, const float* d_th2, double* d_S12, uint8_t* d_inlier, int32_t* d_nin,
                         int32_t* d_stats, void* stream) {
    GF_CHECK(ctx, GF_ERR_ARG, "gf_optimize_sim3_dev: null ctx");
    if (nprob <= 0) return GF_OK;
    GF_CHECK(d_X1 && d_X2 && d_z1 && d_z2 && d_w1 && d_w2 && d_offsets && d_K && d_th2 && d_S12 && d_inlier && d_nin,
             GF_ERR_ARG, "gf_optimize_sim3_dev: null buffer");
    Sim3OptArgs A{};
    A.X1 = d_X1;
    A.X2 = d_X2;
    A.z1 = d_z1;
    A.z2 = d_z2;
    A.w1 = d_w1;
    A.w2 = d_w2;
    A.offs = d_offsets;
    A.K = d_K;
    A.th2 = d_th2;
    A.est = d_S12;
    A.inl = d_inlier;
    A.nin = d_nin;
    A.stats = d_stats;
    hipStream_t s = (hipStream_t)stream;
    GF_PROF(ctx, s, "k_sim3_opt");
    GF_LAUNCH(k_sim3_opt, nprob, SO_T, 0, s, A);
    GF_HIP(hipGetLastError());
    return GF_OK;
}

int gf_optimize_sim3(gf_ctx* ctx, int n, const float* X1, const float* X2, const float* z1, const float* z2,
                     const float* w1, const float* w2, const float K1[4], const float K2[4], float th2, double S12[8],
                     uint8_t* inlier, int32_t* nin, int32_t* stats) {
    GF_CHECK(ctx && K1 && K2 && S12 && nin, GF_ERR_ARG, "gf_optimize_sim3: null arg");
    GF_CHECK(n >= 0 && (n == 0 || (X1 && X2 && z1 && z2 && w1 && w2 && inlier)), GF_ERR_ARG,
             "gf_optimize_sim3: bad pair list");
    GF_HIP(hipSetDevice(ctx->device));
    // one scratch block: the pair arrays, then the per-problem records
    size_t off = 0;
    auto add = [&](size_t bytes) {
        const size_t o = off;
        off += (bytes + 15) & ~(size_t)15;
        return o;
    };
    const size_t m = (size_t)n;
    const size_t o_x1 = add(12 * m), o_x2 = add(12 * m), o_z1 = add(8 * m), o_z2 = add(8 * m), o_w1 = add(4 * m),
                 o_w2 = add(4 * m), o_off = add(8), o_k = add(32), o_th = add(4), o_est = add(64), o_inl = add(m),
                 o_nin = add(4), o_st = add(16);
    void* dbuf;
    int rc = gf::ws_get(ctx, 0, off, &dbuf);
    if (rc) return rc;
    uint8_t* base = (uint8_t*)dbuf;
    hipStream_t s = ctx->stream;
    const int32_t offs[2] = {0, n};
    float K[8];
    for (int i = 0; i < 4; i++) K[i] = K1[i], K[4 + i] = K2[i];
    if (n) {
        GF_HIP(hipMemcpyAsync(base + o_x1, X1, 12 * m, hipMemcpyHostToDevice, s));
        GF_HIP(hipMemcpyAsync(base + o_x2, X2, 12 * m, hipMemcpyHostToDevice, s));
        GF_HIP(hipMemcpyAsync(base + o_z1, z1, 8 * m, hipMemcpyHostToDevice, s));
        GF_HIP(hipMemcpyAsync(base + o_z2, z2, 8 * m, hipMemcpyHostToDevice, s));
        GF_HIP(hipMemcpyAsync(base + o_w1, w1, 4 * m, hipMemcpyHostToDevice, s));
        GF_HIP(hipMemcpyAsync(base + o_w2, w2, 4 * m, hipMemcpyHostToDevice, s));
    }
    GF_HIP(hipMemcpyAsync(base + o_off, offs, 8, hipMemcpyHostToDevice, s));
    GF_HIP(hipMemcpyAsync(base + o_k, K, 32, hipMemcpyHostToDevice, s));
    GF_HIP(hipMemcpyAsync(base + o_th, &th2, 4, hipMemcpyHostToDevice, s));
    GF_HIP(hipMemcpyAsync(base + o_est, S12, 64, hipMemcpyHostToDevice, s));
    rc =gf_optimize_sim3_dev(ctx, 1, (const float*)(base + o_x1), (const float*)(base + o_x2),
                              (const float*)(base + o_z1), (const float*)(base + o_z2), (const float*)(base + o_w1),
                              (const float*)(base + o_w2), (const int32_t*)(base + o_off), (const float*)(base + o_k),
                              (const float*)(base + o_th), (double*)(base + o_est), base + o_inl,
                              (int32_t*)(base + o_nin), (int32_t*)(base + o_st), s);
    if (rc) return rc;
    int32_t st[4] = {0, 0, 0, 0}, ni = 0;
    GF_HIP(hipMemcpyAsync(S12, base + o_est, 64, hipMemcpyDeviceToHost, s));
    if (n) GF_HIP(hipMemcpyAsync(inlier, base + o_inl, m, hipMemcpyDeviceToHost, s));
    GF_HIP(hipMemcpyAsync(&ni, base + o_nin, 4, hipMemcpyDeviceToHost, s));
    GF_HIP(hipMemcpyAsync(st, base + o_st, 16, hipMemcpyDeviceToHost, s));
    GF_HIP(hipStreamSynchronize(s));
    *nin = ni;
    if (stats)
        for (int i = 0; i < 4; i++) stats[i] = st[i];
    return GF_OK;
}

}  // extern "C"
