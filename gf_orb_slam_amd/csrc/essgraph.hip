// Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:1768-2017) on gfx950: the
// 7-DoF pose graph over every keyframe of the map that LoopClosing::CorrectLoop
// runs after a loop is accepted (LoopClosing.cc:556), and the point correction
// of CorrectLoop itself (LoopClosing.cc:462-491).
//
// Host (gf_essgraph_plan_create): the edge set of :1832-1957 (integer logic;
// the reference's pointer-ordered sets and maps walked in keyframe-id order),
// the Hessian index (rank by id among the free keyframes), per 7x7 block the
// list of edges that add to it, and the tile envelope of the factor.
//
// Device, per Levenberg iteration:
//   k_eg_linearize  two edges per workgroup, 32 lanes each: lane 0 the error,
//                   lanes 1..28 the 28 perturbed errors of BaseBinaryEdge's
//                   central differences (base_binary_edge.hpp:147-196, the
//                   fixed vertex skipped), then the two 7x7 Jacobians
//   k_eg_blocks     one workgroup per 7x7 block of H (and its part of b): the
//                   block's edges are summed in the host's order, no atomics
// and per trial (optimization_algorithm_levenberg.cpp:102-149):
//   k_eg_scatter    H + lambda I into 64x64 f64 tiles: a keyframe is padded to
//                   8 rows (unit diagonal, zero right-hand side), a tile holds
//                   8 keyframes; only tiles inside the row envelope exist
//   k_eg_potrf / k_eg_trsm / k_eg_syrk   right-looking tile LLt per tile
//                   column: the diagonal factor in LDS, the panel solves one
//                   workgroup per tile, the trailing update
//                   A(i,j) -= L(i,k) L(j,k)^T on v_mfma_f64_16x16x4f64, for
//                   the tile rows whose envelope reaches column k only
//   k_eg_subst      forward and back substitution by one workgroup
//   k_eg_update     oplusImpl: Sim3(update) * estimate into the trial poses
//   k_eg_chi2 / k_eg_reduce   the errors of the trial, chi2 and computeScale in
//                   a fixed order
// The host reads (chi2, scale, pivot flag) back per trial and runs the
// reference's schedule: lambda0 = 1e-16 (setUserLambdaInit), push / pop /
// discardTop as a swap of the estimate and trial buffers, the cubic lambda
// update, 10 trials per iteration, the rho == 0 / qmax == 10 / _nBad >= 3
// rules, optimize(20). CHOLMOD's ordering is not reproduced (A25).
// k_eg_poses / k_eg_points write [R | t/s] (:1965-1983) and
// correctedSwr.map(Srw.map(p)) (:1986-2016); MapPoint::UpdateNormalAndDepth is
// left to the caller.
#include "essgraph_core.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <map>
#include <set>
#include <vector>

namespace {
using namespace gfess;

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int EG_TS = 64;             // tile side: 8 keyframes of 8 padded rows
constexpr int EG_TT = EG_TS * EG_TS;  // doubles per tile
constexpr int EG_JS = 105;            // per edge: Ji (49), Jj (49), error (7)
constexpr int EG_LP = EG_TS + 1;      // LDS row pitch
constexpr int EG_PT = 1024;           // threads of k_eg_potrf

struct EGArgs {
    int N, ne, nf, nt, npts, nblk;
    const float* Tcw;            // [N][16]
    const int32_t* corr;         // [N] row of corrected / noncorrected or -1
    const double* corrected;     // [ncorr][8]
    const double* noncorrected;  // [ncorr][8]
    const int32_t* edges;        // [ne][3] i, j, kind
    const int32_t* hidx;         // [N] Hessian index, -1 = fixed
    double* vScw;                // [N][8]
    double* est;                 // [N][8] the estimates
    double* trial;               // [N][8] the estimates of the trial in flight
    double* meas;                // [ne][8]
    double* J;                   // [ne][EG_JS]
    double* chi;                 // [ne]
    const int32_t* blk;          // [nblk][4] row index a, column index b <= a, items [i0, i1)
    const int32_t* items;        // [][2] edge, 0 = vertex 0 is the row / 1 = vertex 1 is the row
    double* Hblk;                // [nblk][49]
    double* tiles;               // the envelope's tiles, row by row
    const int32_t* first;        // [nt] lowest tile column of tile row r
    const int32_t* rowoff;       // [nt] tile index of (r, first[r])
    const int32_t* colrows;      // rows i > k with first[i] <= k, per tile column k
    const int32_t* colstart;     // [nt + 1]
    double* b;                   // [64 nt]
    double* x;                   // [64 nt] Solver::_x, kept when a factorisation fails
    double* y;                   // [64 nt]
    double* scal;                // [2] chi2, computeScale
    int32_t* flag;               // non-positive or non-finite pivot
    // write-back
    const float* pos;
    const uint8_t* bad;
    const int32_t* ref;
    const int32_t* cref;
    float* Tcw_out;
    float* pos_out;
};

__device__ __forceinline__ double* eg_tile(const EGArgs& A, int r, int c) {
    return A.tiles + (size_t)(A.rowoff[r] + c - A.first[r]) * EG_TT;
}

// :1797-1829: vScw and the vertex estimates
__global__ __launch_bounds__(64) void k_eg_vertices(EGArgs A) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= A.N) return;
    const int c = A.corr[i];
    const Sim3 S = c >= 0 ? sim3_load(A.corrected + 8 * (size_t)c) : sim3_from_pose(A.Tcw + 16 * (size_t)i);
    sim3_store(S, A.vScw + 8 * (size_t)i);
    sim3_store(S, A.est + 8 * (size_t)i);
}

// the measurements Sji = Sjw * Swi: :1842-1852 for a loop connection (vScw on
// both sides), :1874-1946 otherwise (the non-corrected pose where there is one)
__global__ __launch_bounds__(64) void k_eg_measure(EGArgs A) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= A.ne) return;
    const int i = A.edges[3 * e], j = A.edges[3 * e + 1], kind = A.edges[3 * e + 2];
    const int ci = A.corr[i], cj = A.corr[j];
    const bool ni = kind != 0 && ci >= 0, nj = kind != 0 && cj >= 0;
    const Sim3 Siw = sim3_load(ni ? A.noncorrected + 8 * (size_t)ci : A.vScw + 8 * (size_t)i);
    const Sim3 Sjw = sim3_load(nj ? A.noncorrected + 8 * (size_t)cj : A.vScw + 8 * (size_t)j);
    sim3_store(sim3_mul(Sjw, sim3_inverse(Siw)), A.meas + 8 * (size_t)e);
}

__global__ __launch_bounds__(64) void k_eg_linearize(EGArgs A) {
    __shared__ double errs[2][29][7];
    const int half = threadIdx.x >> 5, k = threadIdx.x & 31;
    const int e = 2 * blockIdx.x + half;
    const bool live = e < A.ne;
    int i = 0, j = 0;
    if (live) {
        i = A.edges[3 * e];
        j = A.edges[3 * e + 1];
    }
    const bool fix[2] = {live && A.hidx[i] < 0, live && A.hidx[j] < 0};
    if (live && k < 29) {
        const int side = k >= 15, kk = k == 0 ? 0 : (k - 1) % 14;
        double r[7] = {0, 0, 0, 0, 0, 0, 0};
        if (k == 0 || !fix[side]) {
            Sim3 v1 = sim3_load(A.est + 8 * (size_t)i), v2 = sim3_load(A.est + 8 * (size_t)j);
            if (k > 0) {
                double u[7];
                const int d = kk >> 1;
                const double dv = (kk & 1) ? -1e-9 : 1e-9;
#pragma unroll
                for (int c = 0; c < 7; c++) u[c] = c == d ? dv : 0.0;
                const Sim3 E = sim3_exp(u);
                if (side == 0)
                    v1 = sim3_mul(E, v1);
                else
                    v2 = sim3_mul(E, v2);
            }
            edge_error(sim3_load(A.meas + 8 * (size_t)e), v1, v2, r);
        }
#pragma unroll
        for (int c = 0; c < 7; c++) errs[half][k][c] = r[c];
    }
    __syncthreads();
    if (!live) return;
    double* out = A.J + (size_t)e * EG_JS;
    const double scalar = 1.0 / (2 * 1e-9);
    for (int t = k; t < 98; t += 32) {
        const int side = t / 49, r = (t % 49) / 7, d = t % 7;
        out[t] = fix[side] ? 0.0 : scalar * (errs[half][1 + 14 * side + 2 * d][r] - errs[half][2 + 14 * side + 2 * d][r]);
    }
    if (k < 7) out[98 + k] = errs[half][0][k];
    if (k == 7) {
        double c = 0;
        for (int a = 0; a < 7; a++) c += errs[half][0][a] * errs[half][0][a];
        A.chi[e] = c;
    }
}

// the errors of the trial estimates: computeActiveErrors after update()
__global__ __launch_bounds__(64) void k_eg_chi2(EGArgs A) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= A.ne) return;
    const int i = A.edges[3 * e], j = A.edges[3 * e + 1];
    double r[7];
    edge_error(sim3_load(A.meas + 8 * (size_t)e), sim3_load(A.trial + 8 * (size_t)i),
               sim3_load(A.trial + 8 * (size_t)j), r);
    double c = 0;
#pragma unroll
    for (int a = 0; a < 7; a++) c += r[a] * r[a];
    A.chi[e] = c;
}

// constructQuadraticForm (base_binary_edge.hpp:55-120) gathered per block:
// H(a, b) = sum Jrow^T Jcol, b(a) = sum Jrow^T (-error), the block's edges in
// the host's order
__global__ __launch_bounds__(64) void k_eg_blocks(EGArgs A) {
    const int q = blockIdx.x, t = threadIdx.x;
    const int a = A.blk[4 * q], bcol = A.blk[4 * q + 1], i0 = A.blk[4 * q + 2], i1 = A.blk[4 * q + 3];
    const bool diag = a == bcol;
    if (t < 49) {
        const int p = t / 7, c = t % 7;
        double s = 0;
        for (int it = i0; it < i1; it++) {
            const double* Je = A.J + (size_t)A.items[2 * it] * EG_JS;
            const int rs = A.items[2 * it + 1];
            const double* Jr = Je + 49 * rs;
            const double* Jc = Je + 49 * (diag ? rs : 1 - rs);
            double v = 0;
#pragma unroll
            for (int m = 0; m < 7; m++) v += Jr[7 * m + p] * Jc[7 * m + c];
            s += v;
        }
        A.Hblk[49 * (size_t)q + t] = s;
    } else if (t < 56 && diag) {
        const int p = t - 49;
        double s = 0;
        for (int it = i0; it < i1; it++) {
            const double* Je = A.J + (size_t)A.items[2 * it] * EG_JS;
            const double* Jr = Je + 49 * A.items[2 * it + 1];
            double v = 0;
#pragma unroll
            for (int m = 0; m < 7; m++) v += Jr[7 * m + p] * -Je[98 + m];
            s += v;
        }
        A.b[8 * a + p] = s;
    }
}

// H + lambda I into the (zeroed) tiles; workgroups past the blocks set the
// unit diagonal of the padding rows
__global__ __launch_bounds__(64) void k_eg_scatter(EGArgs A, double lambda) {
    const int q = blockIdx.x, t = threadIdx.x;
    if (q >= A.nblk) {
        const int r = q - A.nblk, row = EG_TS * r + t;
        if ((row & 7) == 7 || (row >> 3) >= A.nf) eg_tile(A, r, r)[t * EG_TS + t] = 1.0;
        if (q == A.nblk && t == 0) *A.flag = 0;
        return;
    }
    if (t >= 49) return;
    const int a = A.blk[4 * q], b = A.blk[4 * q + 1];
    const int p = t / 7, c = t % 7;
    double v = A.Hblk[49 * (size_t)q + t];
    if (a == b && p == c) v += lambda;
    eg_tile(A, a >> 3, b >> 3)[(8 * (a & 7) + p) * EG_TS + 8 * (b & 7) + c] = v;
}

// the diagonal tile's Cholesky factor (lower), in LDS: 64 dependent steps, the
// trailing update of a step spread over EG_PT threads
__global__ __launch_bounds__(EG_PT) void k_eg_potrf(EGArgs A, int k) {
    __shared__ double T[EG_TS][EG_LP];
    double* g = eg_tile(A, k, k);
    const int tid = threadIdx.x;
    for (int e = tid; e < EG_TT; e += EG_PT) T[e >> 6][e & 63] = g[e];
    __syncthreads();
    for (int j = 0; j < EG_TS; j++) {
        const double d = T[j][j];
        if (!(d > 0.0) || !isfinite(d)) {  // uniform: every thread reads the same pivot
            if (tid == 0) *A.flag = 1;
            return;
        }
        const double l = sqrt(d);
        __syncthreads();
        if (tid < EG_TS) {
            if (tid == j)
                T[j][j] = l;
            else if (tid > j)
                T[tid][j] /= l;
        }
        __syncthreads();
        for (int e = tid; e < EG_TT; e += EG_PT) {
            const int i = e >> 6, c = e & 63;
            if (c > j && i >= c) T[i][c] -= T[i][j] * T[c][j];
        }
        __syncthreads();
    }
    for (int e = tid; e < EG_TT; e += EG_PT) g[e] = T[e >> 6][e & 63];
}

// the panel: A(i, k) <- A(i, k) L(k, k)^-T for the rows i of column k's list
__global__ __launch_bounds__(256) void k_eg_trsm(EGArgs A, int k) {
    // L is read one entry by all lanes (a broadcast); B is kept transposed,
    // Bt[c][row], so that lane = row walks consecutive addresses: 64 KiB of LDS
    __shared__ double L[EG_TS][EG_TS];
    __shared__ double Bt[EG_TS][EG_TS];
    const int i = A.colrows[A.colstart[k] + blockIdx.x];
    const double* gl = eg_tile(A, k, k);
    double* gb = eg_tile(A, i, k);
    const int tid = threadIdx.x;
    for (int e = tid; e < EG_TT; e += 256) {
        L[e >> 6][e & 63] = gl[e];
        Bt[e & 63][e >> 6] = gb[e];
    }
    __syncthreads();
    // thread (row, part): the 64 dependent steps of a row, a step's updates of
    // the columns c2 > c dealt to the row's four parts (each entry still takes
    // its terms in column order)
    const int row = tid & 63, part = tid >> 6;
    for (int c = 0; c < EG_TS; c++) {
        const double x = Bt[c][row] / L[c][c];
        __syncthreads();  // every part has read Bt[c][row] before part 0 replaces it
        if (part == 0) Bt[c][row] = x;
        for (int c2 = c + 1 + part; c2 < EG_TS; c2 += 4) Bt[c2][row] -= x * L[c2][c];
        __syncthreads();
    }
    for (int e = tid; e < EG_TT; e += 256) gb[e] = Bt[e & 63][e >> 6];
}

// the trailing update A(i, j) -= L(i, k) L(j, k)^T over the pairs i >= j of
// column k's row list; wave w owns rows [16 w, 16 w + 16) of the tile. The
// accumulators start from A(i, j) and take -L(i, k) as the A operand, so an
// entry is A - l0 l0' - l1 l1' ... in column order. f64 16x16x4: A operand
// row = lane & 15, k = lane >> 4; C/D col = lane & 15, row = (lane >> 4) + 4 r.
__global__ __launch_bounds__(256) void k_eg_syrk(EGArgs A, int k) {
    const int32_t* rows = A.colrows + A.colstart[k];
    int ia = 0;
    while ((ia + 1) * (ia + 2) / 2 <= (int)blockIdx.x) ia++;
    const int ib = (int)blockIdx.x - ia * (ia + 1) / 2;
    const int i = rows[ia], j = rows[ib];
    const double* Li = eg_tile(A, i, k);
    const double* Lj = eg_tile(A, j, k);
    double* C = eg_tile(A, i, j);
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63, lr = l & 15, lk = l >> 4;
    d4 acc[4];
#pragma unroll
    for (int cb = 0; cb < 4; cb++)
#pragma unroll
        for (int r = 0; r < 4; r++) acc[cb][r] = C[(16 * w + lk + 4 * r) * EG_TS + 16 * cb + lr];
    for (int ks = 0; ks < EG_TS / 4; ks++) {
        const double a = -Li[(16 * w + lr) * EG_TS + 4 * ks + lk];
#pragma unroll
        for (int cb = 0; cb < 4; cb++) {
            const double bv = Lj[(16 * cb + lr) * EG_TS + 4 * ks + lk];
            acc[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bv, acc[cb], 0, 0, 0);
        }
    }
#pragma unroll
    for (int cb = 0; cb < 4; cb++)
#pragma unroll
        for (int r = 0; r < 4; r++) C[(16 * w + lk + 4 * r) * EG_TS + 16 * cb + lr] = acc[cb][r];
}

// L y = b, L^T x = y over the envelope by one workgroup. Nothing is written
// when the factorisation failed: x keeps the last solution.
__global__ __launch_bounds__(256) void k_eg_subst(EGArgs A) {
    __shared__ double L[EG_TS][EG_LP];
    __shared__ double part[4][EG_TS];
    __shared__ double s[EG_TS];
    if (*A.flag) return;
    const int tid = threadIdx.x, lane = tid & 63, pt = tid >> 6;
    for (int r = 0; r < A.nt; r++) {
        double acc = 0;
        for (int c = A.first[r] + pt; c < r; c += 4) {
            const double* T = eg_tile(A, r, c) + lane * EG_TS;
            const double* yc = A.y + EG_TS * c;
            for (int kk = 0; kk < EG_TS; kk++) acc += T[kk] * yc[kk];
        }
        part[pt][lane] = acc;
        const double* g = eg_tile(A, r, r);
        for (int e = tid; e < EG_TT; e += 256) L[e >> 6][e & 63] = g[e];
        __syncthreads();
        if (tid < EG_TS) s[tid] = A.b[EG_TS * r + tid] - ((part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid]));
        __syncthreads();
        for (int kk = 0; kk < EG_TS; kk++) {
            if (tid == kk) s[kk] = s[kk] / L[kk][kk];
            __syncthreads();
            if (tid < EG_TS && tid > kk) s[tid] -= L[tid][kk] * s[kk];
            __syncthreads();
        }
        if (tid < EG_TS) A.y[EG_TS * r + tid] = s[tid];
        __syncthreads();
    }
    for (int r = A.nt - 1; r >= 0; r--) {
        double acc = 0;
        for (int q = A.colstart[r] + pt; q < A.colstart[r + 1]; q += 4) {
            const int i = A.colrows[q];
            const double* T = eg_tile(A, i, r);
            const double* xi = A.x + EG_TS * i;
            for (int kk = 0; kk < EG_TS; kk++) acc += T[kk * EG_TS + lane] * xi[kk];
        }
        part[pt][lane] = acc;
        const double* g = eg_tile(A, r, r);
        for (int e = tid; e < EG_TT; e += 256) L[e >> 6][e & 63] = g[e];
        __syncthreads();
        if (tid < EG_TS) s[tid] = A.y[EG_TS * r + tid] - ((part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid]));
        __syncthreads();
        for (int kk = EG_TS - 1; kk >= 0; kk--) {
            if (tid == kk) s[kk] = s[kk] / L[kk][kk];
            __syncthreads();
            if (tid < kk) s[tid] -= L[kk][tid] * s[kk];
            __syncthreads();
        }
        if (tid < EG_TS) A.x[EG_TS * r + tid] = s[tid];
        __syncthreads();
    }
}

// SparseOptimizer::update: oplusImpl of every free vertex into the trial poses
__global__ __launch_bounds__(64) void k_eg_update(EGArgs A) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= A.N) return;
    const int h = A.hidx[i];
    Sim3 S = sim3_load(A.est + 8 * (size_t)i);
    if (h >= 0) {
        double u[7];
#pragma unroll
        for (int c = 0; c < 7; c++) u[c] = A.x[8 * (size_t)h + c];
        S = sim3_mul(sim3_exp(u), S);
    }
    sim3_store(S, A.trial + 8 * (size_t)i);
}

// activeRobustChi2 and computeScale: strided partial sums, then a fixed tree
__global__ __launch_bounds__(256) void k_eg_reduce(EGArgs A, double lambda) {
    __shared__ double sc[256], ss[256];
    const int tid = threadIdx.x;
    double c = 0, s = 0;
    for (int e = tid; e < A.ne; e += 256) c += A.chi[e];
    for (int q = tid; q < EG_TS * A.nt; q += 256) s += A.x[q] * (lambda * A.x[q] + A.b[q]);
    sc[tid] = c;
    ss[tid] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
            sc[tid] += sc[tid + o];
            ss[tid] += ss[tid + o];
        }
        __syncthreads();
    }
    if (tid == 0) {
        A.scal[0] = sc[0];
        A.scal[1] = ss[0];
    }
}

// :1965-1983: [R | t/s] in float
__global__ __launch_bounds__(64) void k_eg_poses(EGArgs A) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= A.N) return;
    const Sim3 S = sim3_load(A.est + 8 * (size_t)i);
    double R[9];
    gfse3::to_R(S.r, R);
    const double is = 1. / S.s;
    float* T = A.Tcw_out + 16 * (size_t)i;
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) T[4 * r + c] = (float)R[3 * r + c];
        T[4 * r + 3] = (float)(S.t[r] * is);
    }
    T[12] = T[13] = T[14] = 0.f;
    T[15] = 1.f;
}

// to[c].inverse().map(from[c].map(p)) with c = sel2[m] where that is >= 0, else
// sel[m]: :1986-2016 (from = vScw, to = the optimised estimates) and
// LoopClosing.cc:462-491 (from = NonCorrectedSim3, to = CorrectedSim3). A bad
// point or c < 0 is copied through.
__global__ __launch_bounds__(256) void k_eg_points(int npts, const float* pos, const uint8_t* bad, const int32_t* sel,
                                                   const int32_t* sel2, const double* from, const double* to,
                                                   float* out) {
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= npts) return;
    const float p0 = pos[3 * (size_t)m], p1 = pos[3 * (size_t)m + 1], p2 = pos[3 * (size_t)m + 2];
    float o0 = p0, o1 = p1, o2 = p2;
    int c = sel[m];
    if (sel2 && sel2[m] >= 0) c = sel2[m];
    if (!bad[m] && c >= 0) {
        const double p[3] = {(double)p0, (double)p1, (double)p2};
        double a[3], q[3];
        sim3_map(sim3_load(from + 8 * (size_t)c), p, a);
        sim3_map(sim3_inverse(sim3_load(to + 8 * (size_t)c)), a, q);
        o0 = (float)q[0];
        o1 = (float)q[1];
        o2 = (float)q[2];
    }
    out[3 * (size_t)m] = o0;
    out[3 * (size_t)m + 1] = o1;
    out[3 * (size_t)m + 2] = o2;
}

// ------------------------------------------------------------------ host
struct EGProblem {
    int N = 0, ne = 0, nf = 0, nt = 0, npts = 0, nblk = 0, ncorr = 0, loop_kf = 0;
    size_t ntiles = 0;
    std::vector<int32_t> edges;     // [ne][3]
    std::vector<int32_t> colstart;  // host copy: the factor loop's launch shapes
    std::vector<void*> allocs;
    EGArgs A{};
    // results
    std::vector<float> Tcw, pos;
    gf_essgraph_stats stats{};
    std::vector<double> tr_lambda, tr_chi;
    std::vector<uint8_t> tr_acc;
};

int eg_weight(const gf_essgraph_problem& P, int i, int j) {  // KeyFrame::GetWeight
    for (int k = P.cov_start[i]; k < P.cov_start[i + 1]; k++)
        if (P.cov_nbr[k] == j) return P.cov_weight[k];
    return 0;
}

// Optimizer.cc:1832-1957 -> rows (i, j, kind)
void eg_build_edges(const gf_essgraph_problem& P, std::vector<int32_t>& rows) {
    const int minFeat = 100;
    auto add = [&](int i, int j, int kind) {
        rows.push_back(i);
        rows.push_back(j);
        rows.push_back(kind);
    };
    std::set<std::pair<int, int>> sInsertedEdges;
    // SET LOOP EDGES: the map and its sets in id order (the index order)
    std::map<int, std::set<int>> lc;
    for (int k = 0; k < P.nlc; k++)
        for (int q = P.lc_start[k]; q < P.lc_start[k + 1]; q++) lc[P.lc_key[k]].insert(P.lc_nbr[q]);
    for (const auto& kv : lc) {
        const int i = kv.first;
        for (const int j : kv.second) {
            if ((i != P.cur_kf || j != P.loop_kf) && eg_weight(P, i, j) < minFeat) continue;
            add(i, j, 0);
            sInsertedEdges.insert(std::make_pair(std::min(i, j), std::max(i, j)));
        }
    }
    // SET NORMAL EDGES
    for (int i = 0; i < P.nkf; i++) {
        const int parent = P.parent[i];
        if (parent >= 0) add(i, parent, 1);
        const std::set<int> sLoopEdges(P.le_nbr + P.le_start[i], P.le_nbr + P.le_start[i + 1]);
        for (const int l : sLoopEdges)
            if (l < i) add(i, l, 2);
        for (int k = P.cov_start[i]; k < P.cov_start[i + 1]; k++) {
            if (P.cov_weight[k] < minFeat) break;  // GetCovisiblesByWeight: the ordered prefix
            const int n = P.cov_nbr[k];
            if (n == parent || P.parent[n] == i || sLoopEdges.count(n)) continue;
            if (n >= i) continue;
            if (sInsertedEdges.count(std::make_pair(n, i))) continue;
            add(i, n, 3);
        }
    }
}

int eg_validate(const gf_essgraph_problem& P, int p) {
    const std::string at = "gf_essgraph_plan_create: problem " + std::to_string(p) + ": ";
    GF_CHECK(P.nkf >= 2, GF_ERR_ARG, at + "fewer than 2 keyframes");
    GF_CHECK(P.nkf <= GF_ESSGRAPH_MAX_KF, GF_ERR_ARG, at + "more than GF_ESSGRAPH_MAX_KF keyframes");
    GF_CHECK(P.npts >= 0 && P.ncorr >= 0 && P.nlc >= 0, GF_ERR_ARG, at + "negative count");
    GF_CHECK(P.kf_id && P.kf_Tcw && P.parent && P.cov_start && P.le_start, GF_ERR_ARG, at + "null keyframe array");
    const int N = P.nkf;
    auto in = [N](int v) { return v >= 0 && v < N; };
    for (int i = 1; i < N; i++) GF_CHECK(P.kf_id[i] > P.kf_id[i - 1], GF_ERR_ARG, at + "kf_id is not strictly increasing");
    GF_CHECK(in(P.loop_kf) && in(P.cur_kf), GF_ERR_ARG, at + "loop_kf / cur_kf out of range");
    for (int i = 0; i < N; i++)
        GF_CHECK(P.parent[i] >= -1 && P.parent[i] < N && P.parent[i] != i, GF_ERR_ARG, at + "parent out of range");
    auto csr = [&](const int32_t* start, const int32_t* nbr, int rows, const char* what) {
        if (start[0] != 0) return gf::fail(GF_ERR_ARG, at + what + " does not start at 0");
        for (int i = 0; i < rows; i++)
            if (start[i + 1] < start[i]) return gf::fail(GF_ERR_ARG, at + what + " offsets decrease");
        if (start[rows] > 0 && !nbr) return gf::fail(GF_ERR_ARG, at + what + " is null");
        for (int k = 0; k < start[rows]; k++)
            if (!in(nbr[k])) return gf::fail(GF_ERR_ARG, at + what + " index out of range");
        return (int)GF_OK;
    };
    int rc = csr(P.cov_start, P.cov_nbr, N, "covisibility");
    if (rc) return rc;
    GF_CHECK(P.cov_start[N] == 0 || P.cov_weight, GF_ERR_ARG, at + "null covisibility weights");
    if ((rc = csr(P.le_start, P.le_nbr, N, "loop edges"))) return rc;
    if (P.nlc) {
        GF_CHECK(P.lc_key && P.lc_start, GF_ERR_ARG, at + "null loop connections");
        for (int k = 0; k < P.nlc; k++) GF_CHECK(in(P.lc_key[k]), GF_ERR_ARG, at + "loop connection key out of range");
        if ((rc = csr(P.lc_start, P.lc_nbr, P.nlc, "loop connections"))) return rc;
    }
    if (P.ncorr) {
        GF_CHECK(P.corr_idx && P.corrected && P.noncorrected, GF_ERR_ARG, at + "null corrected arrays");
        for (int c = 0; c < P.ncorr; c++) GF_CHECK(in(P.corr_idx[c]), GF_ERR_ARG, at + "corrected index out of range");
    }
    if (P.npts) {
        GF_CHECK(P.pt_pos && P.pt_bad && P.pt_ref && P.pt_corrected_ref, GF_ERR_ARG, at + "null point array");
        for (int m = 0; m < P.npts; m++)
            GF_CHECK(P.pt_ref[m] >= -1 && P.pt_ref[m] < N && P.pt_corrected_ref[m] >= -1 && P.pt_corrected_ref[m] < N,
                     GF_ERR_ARG, at + "point reference out of range");
    }
    return GF_OK;
}

template <typename T>
int eg_upload(EGProblem& Q, const T* host, size_t n, const T** out, hipStream_t s) {
    void* d = nullptr;
    GF_HIP(hipMalloc(&d, std::max<size_t>(n, 1) * sizeof(T)));
    Q.allocs.push_back(d);
    if (n) GF_HIP(hipMemcpyAsync(d, host, n * sizeof(T), hipMemcpyHostToDevice, s));
    *out = (const T*)d;
    return GF_OK;
}

template <typename T>
int eg_alloc(EGProblem& Q, size_t n, T** out) {
    void* d = nullptr;
    GF_HIP(hipMalloc(&d, std::max<size_t>(n, 1) * sizeof(T)));
    Q.allocs.push_back(d);
    *out = (T*)d;
    return GF_OK;
}

#define EG_TRY(expr)            \
    do {                        \
        const int _rc = (expr); \
        if (_rc) return _rc;    \
    } while (0)

// structure of one problem: edges, Hessian index, block gather lists, envelope
int eg_setup(gf_ctx* ctx, const gf_essgraph_problem& P, EGProblem& Q) {
    hipStream_t s = ctx->stream;
    const int N = P.nkf;
    Q.N = N;
    Q.npts = P.npts;
    Q.ncorr = P.ncorr;
    Q.loop_kf = P.loop_kf;
    eg_build_edges(P, Q.edges);
    Q.ne = (int)Q.edges.size() / 3;
    std::vector<int32_t> hidx(N), corr(N, -1);
    int nf = 0;
    for (int i = 0; i < N; i++) hidx[i] = i == P.loop_kf ? -1 : nf++;
    for (int c = 0; c < P.ncorr; c++) corr[P.corr_idx[c]] = c;
    Q.nf = nf;
    Q.nt = (nf + 7) / 8;
    // blocks (a, b <= a) with their items in edge order; a free keyframe
    // without an edge still owns its (empty) diagonal block
    std::map<std::pair<int, int>, std::vector<std::pair<int, int>>> blocks;
    for (int a = 0; a < nf; a++) blocks[{a, a}];
    std::vector<int32_t> first(Q.nt);
    for (int r = 0; r < Q.nt; r++) first[r] = r;
    for (int e = 0; e < Q.ne; e++) {
        const int h0 = hidx[Q.edges[3 * e]], h1 = hidx[Q.edges[3 * e + 1]];
        if (h0 >= 0) blocks[{h0, h0}].push_back({e, 0});
        if (h1 >= 0) blocks[{h1, h1}].push_back({e, 1});
        if (h0 >= 0 && h1 >= 0 && h0 != h1) {
            const int a = std::max(h0, h1), b = std::min(h0, h1);
            blocks[{a, b}].push_back({e, a == h0 ? 0 : 1});
            first[a >> 3] = std::min(first[a >> 3], b >> 3);
        }
    }
    // measurement only (scripts/essgraph_timing.py): every lower tile, as a
    // factorisation that ignores the envelope would visit
    if (const char* full = getenv("GF_ESSGRAPH_FULL_ENVELOPE"))
        if (full[0] == '1') std::fill(first.begin(), first.end(), 0);
    std::vector<int32_t> blk, items, rowoff(Q.nt), colrows, colstart(Q.nt + 1, 0);
    for (const auto& kv : blocks) {
        blk.push_back(kv.first.first);
        blk.push_back(kv.first.second);
        blk.push_back((int32_t)items.size() / 2);
        for (const auto& it : kv.second) {
            items.push_back(it.first);
            items.push_back(it.second);
        }
        blk.push_back((int32_t)items.size() / 2);
    }
    Q.nblk = (int)blk.size() / 4;
    size_t nt_total = 0;
    for (int r = 0; r < Q.nt; r++) {
        rowoff[r] = (int32_t)nt_total;
        nt_total += (size_t)(r - first[r] + 1);
    }
    GF_CHECK(nt_total <= GF_ESSGRAPH_MAX_TILES, GF_ERR_CAP,
             "gf_essgraph_plan_create: the factor's envelope exceeds GF_ESSGRAPH_MAX_TILES");
    Q.ntiles = nt_total;
    for (int k = 0; k < Q.nt; k++) {
        for (int i = k + 1; i < Q.nt; i++)
            if (first[i] <= k) colrows.push_back(i);
        colstart[k + 1] = (int32_t)colrows.size();
    }
    Q.colstart = colstart;

    EGArgs& A = Q.A;
    A.N = N;
    A.ne = Q.ne;
    A.nf = nf;
    A.nt = Q.nt;
    A.npts = P.npts;
    A.nblk = Q.nblk;
    EG_TRY(eg_upload(Q, P.kf_Tcw, (size_t)16 * N, &A.Tcw, s));
    EG_TRY(eg_upload(Q, corr.data(), (size_t)N, &A.corr, s));
    EG_TRY(eg_upload(Q, P.corrected, (size_t)8 * P.ncorr, &A.corrected, s));
    EG_TRY(eg_upload(Q, P.noncorrected, (size_t)8 * P.ncorr, &A.noncorrected, s));
    EG_TRY(eg_upload(Q, Q.edges.data(), Q.edges.size(), &A.edges, s));
    EG_TRY(eg_upload(Q, hidx.data(), (size_t)N, &A.hidx, s));
    EG_TRY(eg_upload(Q, blk.data(), blk.size(), &A.blk, s));
    EG_TRY(eg_upload(Q, items.data(), items.size(), &A.items, s));
    EG_TRY(eg_upload(Q, first.data(), first.size(), &A.first, s));
    EG_TRY(eg_upload(Q, rowoff.data(), rowoff.size(), &A.rowoff, s));
    EG_TRY(eg_upload(Q, colrows.data(), colrows.size(), &A.colrows, s));
    EG_TRY(eg_upload(Q, colstart.data(), colstart.size(), &A.colstart, s));
    EG_TRY(eg_upload(Q, P.pt_pos, (size_t)3 * P.npts, &A.pos, s));
    EG_TRY(eg_upload(Q, P.pt_bad, (size_t)P.npts, &A.bad, s));
    EG_TRY(eg_upload(Q, P.pt_ref, (size_t)P.npts, &A.ref, s));
    EG_TRY(eg_upload(Q, P.pt_corrected_ref, (size_t)P.npts, &A.cref, s));
    EG_TRY(eg_alloc(Q, (size_t)8 * N, &A.vScw));
    EG_TRY(eg_alloc(Q, (size_t)8 * N, &A.est));
    EG_TRY(eg_alloc(Q, (size_t)8 * N, &A.trial));
    EG_TRY(eg_alloc(Q, (size_t)8 * Q.ne, &A.meas));
    EG_TRY(eg_alloc(Q, (size_t)EG_JS * Q.ne, &A.J));
    EG_TRY(eg_alloc(Q, (size_t)Q.ne, &A.chi));
    EG_TRY(eg_alloc(Q, (size_t)49 * Q.nblk, &A.Hblk));
    EG_TRY(eg_alloc(Q, Q.ntiles * EG_TT, &A.tiles));
    EG_TRY(eg_alloc(Q, (size_t)EG_TS * Q.nt, &A.b));
    EG_TRY(eg_alloc(Q, (size_t)EG_TS * Q.nt, &A.x));
    EG_TRY(eg_alloc(Q, (size_t)EG_TS * Q.nt, &A.y));
    EG_TRY(eg_alloc(Q, (size_t)2, &A.scal));
    EG_TRY(eg_alloc(Q, (size_t)1, &A.flag));
    EG_TRY(eg_alloc(Q, (size_t)16 * N, &A.Tcw_out));
    EG_TRY(eg_alloc(Q, (size_t)3 * P.npts, &A.pos_out));
    Q.Tcw.assign((size_t)16 * N, 0.f);
    Q.pos.assign((size_t)3 * P.npts, 0.f);
    // the host arrays are read by the asynchronous copies above
    GF_HIP(hipStreamSynchronize(s));
    return GF_OK;
}

void eg_free(EGProblem& Q) {
    for (void* d : Q.allocs) (void)hipFree(d);
    Q.allocs.clear();
}

inline int eg_div(int n, int d) { return (n + d - 1) / d; }

// one trial's linear solve: (H + lambda I) x = b
int eg_linear_solve(gf_ctx* ctx, EGProblem& Q, const EGArgs& A, double lambda, hipStream_t s) {
    {
        GF_PROF(ctx, s, "eg_assemble");
        GF_HIP(hipMemsetAsync(A.tiles, 0, Q.ntiles * EG_TT * sizeof(double), s));
        GF_LAUNCH(k_eg_scatter, Q.nblk + Q.nt, 64, 0, s, A, lambda);
    }
    {
        GF_PROF(ctx, s, "eg_factor");
        for (int k = 0; k < Q.nt; k++) {
            GF_LAUNCH(k_eg_potrf, 1, EG_PT, 0, s, A, k);
            const int m = Q.colstart[k + 1] - Q.colstart[k];
            if (m > 0) {
                GF_LAUNCH(k_eg_trsm, m, 256, 0, s, A, k);
                GF_LAUNCH(k_eg_syrk, m * (m + 1) / 2, 256, 0, s, A, k);
            }
        }
    }
    {
        GF_PROF(ctx, s, "eg_subst");
        GF_LAUNCH(k_eg_subst, 1, 256, 0, s, A);
    }
    GF_HIP(hipGetLastError());
    return GF_OK;
}

int eg_read(const EGArgs& A, hipStream_t s, double* chi, double* scale, int* flag) {
    double sc[2];
    int32_t f = 0;
    GF_HIP(hipMemcpyAsync(sc, A.scal, sizeof(sc), hipMemcpyDeviceToHost, s));
    GF_HIP(hipMemcpyAsync(&f, A.flag, sizeof(f), hipMemcpyDeviceToHost, s));
    GF_HIP(hipStreamSynchronize(s));
    *chi = sc[0];
    *scale = sc[1];
    *flag = f;
    return GF_OK;
}

// optimizer.optimize(20) with OptimizationAlgorithmLevenberg::solve
// (optimization_algorithm_levenberg.cpp:61-164) and the write-back
int eg_solve(gf_ctx* ctx, EGProblem& Q, hipStream_t s) {
    EGArgs A = Q.A;
    const int gN = eg_div(Q.N, 64), gE = eg_div(Q.ne, 64);
    GF_HIP(hipMemsetAsync(A.x, 0, (size_t)EG_TS * Q.nt * sizeof(double), s));
    GF_HIP(hipMemsetAsync(A.b, 0, (size_t)EG_TS * Q.nt * sizeof(double), s));
    GF_HIP(hipMemsetAsync(A.flag, 0, sizeof(int32_t), s));
    GF_LAUNCH(k_eg_vertices, gN, 64, 0, s, A);
    if (Q.ne) GF_LAUNCH(k_eg_measure, gE, 64, 0, s, A);
    Q.tr_lambda.assign(GF_ESSGRAPH_TRACE, 0.0);
    Q.tr_chi.assign(GF_ESSGRAPH_TRACE, 0.0);
    Q.tr_acc.assign(GF_ESSGRAPH_TRACE, 0);
    double lambda = 0, ni = 2, currentChi = 0, chi0 = 0;
    int nBad = 0, iters = 0, trials = 0, stop = 0, ntr = 0;
    for (int iter = 0; iter < 20; iter++) {
        iters++;
        {
            GF_PROF(ctx, s, "eg_linearize");
            if (Q.ne) GF_LAUNCH(k_eg_linearize, eg_div(Q.ne, 2), 64, 0, s, A);
            GF_LAUNCH(k_eg_blocks, Q.nblk, 64, 0, s, A);
            GF_LAUNCH(k_eg_reduce, 1, 256, 0, s, A, 0.0);
        }
        double scale;
        int flag;
        EG_TRY(eg_read(A, s, &currentChi, &scale, &flag));
        const double iniChi = currentChi;
        if (iter == 0) {
            chi0 = currentChi;
            lambda = 1e-16;  // setUserLambdaInit(1e-16): computeLambdaInit returns it
            ni = 2;
            nBad = 0;
        }
        double rho = 0;
        int q = 0;
        do {
            trials++;
            EG_TRY(eg_linear_solve(ctx, Q, A, lambda, s));
            {
                GF_PROF(ctx, s, "eg_update");
                GF_LAUNCH(k_eg_update, gN, 64, 0, s, A);
                if (Q.ne) GF_LAUNCH(k_eg_chi2, gE, 64, 0, s, A);
                GF_LAUNCH(k_eg_reduce, 1, 256, 0, s, A, lambda);
            }
            double tempChi;
            EG_TRY(eg_read(A, s, &tempChi, &scale, &flag));
            if (flag) tempChi = DBL_MAX;  // ok2 == false
            rho = currentChi - tempChi;
            scale += 1e-3;
            rho /= scale;
            const bool good = rho > 0 && std::isfinite(tempChi);
            if (ntr < GF_ESSGRAPH_TRACE) {
                Q.tr_lambda[ntr] = lambda;
                Q.tr_chi[ntr] = tempChi;
                Q.tr_acc[ntr] = good;
                ntr++;
            }
            if (good) {
                double alpha = 1. - std::pow((2 * rho - 1), 3);
                alpha = std::min(alpha, 2. / 3.);
                const double scaleFactor = std::max(1. / 3., alpha);
                lambda *= scaleFactor;
                ni = 2;
                currentChi = tempChi;
                std::swap(A.est, A.trial);  // discardTop: the trial becomes the estimate
            } else {
                lambda *= ni;
                ni *= 2;  // pop: the estimate stays
            }
            q++;
        } while (rho < 0 && q < 10);
        if (q == 10 || rho == 0) {
            stop = rho == 0 ? 1 : 2;
            break;
        }
        if ((iniChi - currentChi) * 1e3 < iniChi)
            nBad++;
        else
            nBad = 0;
        if (nBad >= 3) {
            stop = 3;
            break;
        }
    }
    Q.stats.iterations = iters;
    Q.stats.trials = trials;
    Q.stats.stop = stop;
    Q.stats.ntrace = ntr;
    Q.stats.chi2_initial = chi0;
    Q.stats.chi2_final = currentChi;
    {
        GF_PROF(ctx, s, "eg_writeback");
        GF_LAUNCH(k_eg_poses, gN, 64, 0, s, A);
        if (Q.npts)
            GF_LAUNCH(k_eg_points, eg_div(Q.npts, 256), 256, 0, s, Q.npts, A.pos, A.bad, A.ref, A.cref,
                      (const double*)A.vScw, (const double*)A.est, A.pos_out);
    }
    GF_HIP(hipGetLastError());
    GF_HIP(hipMemcpyAsync(Q.Tcw.data(), A.Tcw_out, Q.Tcw.size() * sizeof(float), hipMemcpyDeviceToHost, s));
    if (Q.npts) GF_HIP(hipMemcpyAsync(Q.pos.data(), A.pos_out, Q.pos.size() * sizeof(float), hipMemcpyDeviceToHost, s));
    GF_HIP(hipStreamSynchronize(s));
    return GF_OK;
}

}  // namespace

struct gf_essgraph_plan {
    gf_ctx* ctx = nullptr;
    std::vector<EGProblem> probs;
    bool solved = false;
};

extern "C" {

int gf_essgraph_plan_create(gf_ctx* ctx, int nprob, const gf_essgraph_problem* probs, gf_essgraph_plan** out) {
    GF_CHECK(ctx && probs && out && nprob >= 1, GF_ERR_ARG, "gf_essgraph_plan_create: null or empty argument");
    for (int p = 0; p < nprob; p++) EG_TRY(eg_validate(probs[p], p));
    GF_HIP(hipSetDevice(ctx->device));
    gf_essgraph_plan* plan = new gf_essgraph_plan;
    plan->ctx = ctx;
    plan->probs.resize(nprob);
    for (int p = 0; p < nprob; p++) {
        const int rc = eg_setup(ctx, probs[p], plan->probs[p]);
        if (rc) {
            gf_essgraph_plan_destroy(plan);
            return rc;
        }
    }
    *out = plan;
    return GF_OK;
}

int gf_essgraph_plan_edges(gf_essgraph_plan* plan, int p, int32_t* rows, int cap, int* nedges) {
    GF_CHECK(plan && nedges && p >= 0 && p < (int)plan->probs.size(), GF_ERR_ARG, "gf_essgraph_plan_edges: bad argument");
    const EGProblem& Q = plan->probs[p];
    *nedges = Q.ne;
    if (rows)
        for (int e = 0; e < std::min(cap, Q.ne) * 3; e++) rows[e] = Q.edges[e];
    return GF_OK;
}

int gf_essgraph_plan_solve(gf_essgraph_plan* plan, void* stream) {
    GF_CHECK(plan, GF_ERR_ARG, "gf_essgraph_plan_solve: null plan");
    GF_HIP(hipSetDevice(plan->ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : plan->ctx->stream;
    // per-problem launch sets, one map after the other on the stream
    for (EGProblem& Q : plan->probs) EG_TRY(eg_solve(plan->ctx, Q, s));
    plan->solved = true;
    return GF_OK;
}

int gf_essgraph_plan_results(gf_essgraph_plan* plan, gf_essgraph_result* res) {
    GF_CHECK(plan && res, GF_ERR_ARG, "gf_essgraph_plan_results: null argument");
    GF_CHECK(plan->solved, GF_ERR_ARG, "gf_essgraph_plan_results: the plan has not been solved");
    for (size_t p = 0; p < plan->probs.size(); p++) {
        const EGProblem& Q = plan->probs[p];
        gf_essgraph_result& R = res[p];
        if (R.kf_Tcw) std::copy(Q.Tcw.begin(), Q.Tcw.end(), R.kf_Tcw);
        if (R.pt_pos) std::copy(Q.pos.begin(), Q.pos.end(), R.pt_pos);
        R.stats = Q.stats;
        if (R.trace_lambda) std::copy(Q.tr_lambda.begin(), Q.tr_lambda.end(), R.trace_lambda);
        if (R.trace_chi2) std::copy(Q.tr_chi.begin(), Q.tr_chi.end(), R.trace_chi2);
        if (R.trace_accepted) std::copy(Q.tr_acc.begin(), Q.tr_acc.end(), R.trace_accepted);
    }
    return GF_OK;
}

int gf_essgraph_plan_destroy(gf_essgraph_plan* plan) {
    if (!plan) return GF_OK;
    for (EGProblem& Q : plan->probs) eg_free(Q);
    delete plan;
    return GF_OK;
}

int gf_optimize_essential_graph(gf_ctx* ctx, const gf_essgraph_problem* prob, gf_essgraph_result* res) {
    GF_CHECK(ctx && prob && res, GF_ERR_ARG, "gf_optimize_essential_graph: null argument");
    gf_essgraph_plan* plan = nullptr;
    int rc = gf_essgraph_plan_create(ctx, 1, prob, &plan);
    if (rc) return rc;
    rc = gf_essgraph_plan_solve(plan, nullptr);
    if (!rc) rc = gf_essgraph_plan_results(plan, res);
    gf_essgraph_plan_destroy(plan);
    return rc;
}

int gf_correct_loop_points(gf_ctx* ctx, int npts, const float* pos, const uint8_t* bad, const int32_t* sel, int nsim,
                           const double* from, const double* to, float* pos_out) {
    GF_CHECK(ctx && npts >= 0 && nsim >= 0, GF_ERR_ARG, "gf_correct_loop_points: bad argument");
    if (npts == 0) return GF_OK;
    GF_CHECK(pos && bad && sel && pos_out && (nsim == 0 || (from && to)), GF_ERR_ARG,
             "gf_correct_loop_points: null array");
    for (int m = 0; m < npts; m++)
        GF_CHECK(sel[m] >= -1 && sel[m] < nsim, GF_ERR_ARG, "gf_correct_loop_points: sel out of range");
    GF_HIP(hipSetDevice(ctx->device));
    size_t off = 0;
    auto add = [&](size_t bytes) {
        const size_t o = off;
        off += (bytes + 15) & ~(size_t)15;
        return o;
    };
    const size_t m = (size_t)npts, o_pos = add(12 * m), o_bad = add(m), o_sel = add(4 * m),
                 o_from = add(64 * (size_t)nsim), o_to = add(64 * (size_t)nsim), o_out = add(12 * m);
    void* dbuf;
    const int rc = gf::ws_get(ctx, 0, off, &dbuf);
    if (rc) return rc;
    uint8_t* base = (uint8_t*)dbuf;
    hipStream_t s = ctx->stream;
    GF_HIP(hipMemcpyAsync(base + o_pos, pos, 12 * m, hipMemcpyHostToDevice, s));
    GF_HIP(hipMemcpyAsync(base + o_bad, bad, m, hipMemcpyHostToDevice, s));
    GF_HIP(hipMemcpyAsync(base + o_sel, sel, 4 * m, hipMemcpyHostToDevice, s));
    if (nsim) {
        GF_HIP(hipMemcpyAsync(base + o_from, from, 64 * (size_t)nsim, hipMemcpyHostToDevice, s));
        GF_HIP(hipMemcpyAsync(base + o_to, to, 64 * (size_t)nsim, hipMemcpyHostToDevice, s));
    }
    {
        GF_PROF(ctx, s, "k_eg_points");
        GF_LAUNCH(k_eg_points, eg_div(npts, 256), 256, 0, s, npts, (const float*)(base + o_pos),
                  (const uint8_t*)(base + o_bad), (const int32_t*)(base + o_sel), (const int32_t*)nullptr,
                  (const double*)(base + o_from), (const double*)(base + o_to), (float*)(base + o_out));
    }
    GF_HIP(hipGetLastError());
    GF_HIP(hipMemcpyAsync(pos_out, base + o_out, 12 * m, hipMemcpyDeviceToHost, s));
    GF_HIP(hipStreamSynchronize(s));
    return GF_OK;
}

}  // extern "C"
