// Device pieces of the loop-closure Sim3 solver (sim3.hip): the reference's
// ORB_SLAM::Sim3Solver (src/Sim3Solver.cc) in its operation order and types.
//   draw      the minimal-set draw of iterate() (:163-177) with its write to
//             position idx (the value drawn, not randi): an index can repeat
//             inside one set;
//   compute_T Horn 1987 on three pairs (:226-332): centroids, M, the float 4x4
//             N, cv::eigen, the angle-axis vector, cv::Rodrigues, scale,
//             translation, T12 and T21;
//   is_inlier Project + CheckInliers (:335-398) for one correspondence.
// The OpenCV calls are the restatement of docs/ORACLE_ASSUMPTIONS.md A22
// (Jacobi eigen-solver in float with n*n*30 sweeps at most, Rodrigues in
// double, Mat::dot / cv::norm accumulated in double, small Mat products as
// float sums left to right). No contraction (-ffp-contract=off).
#pragma once
#include "common.h"
#include "rng.h"

namespace gfsim3 {
namespace {

constexpr int kHyp = 32;  // floats of one hypothesis record: T12[16] R[9] t[3] s pad[3]

struct Cam {
    float fx, fy, cx, cy;
};

// A state from device memory is clamped to what the kernels can hold.
__device__ __forceinline__ gf_sim3_state load_state(const gf_sim3_state* states, int b, int cap) {
    gf_sim3_state st = states[b];
    st.n = min(max(st.n, 0), cap);
    return st;
}

// iterations this call may run: while(mnIterations<mRansacMaxIts && nCurrent<nIterations) (:158)
__device__ __forceinline__ int loop_count(const gf_sim3_state& st, int n_iterations) {
    if (st.n < st.min_inliers || st.n < 3) return 0;  // under three the reference indexes an empty vector
    const int a = st.max_iterations - st.iterations;
    const int L = a < n_iterations ? a : n_iterations;
    return L > 0 ? L : 0;
}

__device__ __forceinline__ int random_int(int32_t* s, int32_t* f, int32_t* r, int mn, int mx) {
    const int d = mx - mn + 1;
    return int(((double)gfrng::next(s, f, r) / ((double)2147483647 + 1.0)) * d) + mn;
}

// k_sim3_draw's body for solver b (one thread): three indices per iteration.
// vAvailableIndices is 0..n-1 with at most three overwritten slots (n >= 3:
// loop_count); the index is clamped to the problem all the same.
__device__ void draw_one(const gf_sim3_state* __restrict__ states, const gf_rng* __restrict__ rngs, int b,
                         int n_iterations, int lcap, int32_t* __restrict__ draws, int cap) {
    const gf_sim3_state st = load_state(states, b, cap);
    const int L = min(loop_count(st, n_iterations), lcap);
    int32_t s[31];
    for (int i = 0; i < 31; i++) s[i] = rngs[b].state[i];
    int32_t f = rngs[b].f, r = rngs[b].r;
    int32_t* out = draws + (size_t)b * lcap * 3;
    for (int h = 0; h < L; h++) {
        int p0 = -2, v0 = 0, p1 = -2, v1 = 0, size = st.n;  // overwritten (position, value) pairs
        for (int i = 0; i < 3; i++) {
            const int randi = random_int(s, &f, &r, 0, size - 1);
            int idx = randi, back = size - 1;
            if (p0 == randi) idx = v0;
            if (p1 == randi) idx = v1;
            if (p0 == size - 1) back = v0;
            if (p1 == size - 1) back = v1;
            idx = min(max(idx, 0), st.n - 1);
            out[h * 3 + i] = idx;
            // avail[idx] = back (the third write is never read)
            if (p0 == idx) v0 = back;
            else if (p1 == idx) v1 = back;
            else if (i == 0) p0 = idx, v0 = back;
            else p1 = idx, v1 = back;
            size--;
        }
    }
}

__device__ __forceinline__ float hypot_f(float a, float b) {
    a = fabsf(a);
    b = fabsf(b);
    if (a > b) {
        b /= a;
        return a * sqrtf(1 + b * b);
    }
    if (b > 0) {
        a /= b;
        return b * sqrtf(1 + a * a);
    }
    return 0;
}

// cv::eigen of a symmetric float 4x4 (cyclic-pivot Jacobi, eigenvalues sorted
// descending, eigenvectors as rows of V). A, V, W, ind live in LDS: they are
// indexed by the pivot. A NaN matrix never meets the stop test and ends at the
// sweep bound.
__device__ void jacobi4(float* A, float* V, float* W, int* ind) {
    const int n = 4;
    const float eps = 1.1920929e-07f;
    int* indR = ind;
    int* indC = ind + 4;
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) V[i * n + j] = i == j ? 1.f : 0.f;
    for (int k = 0; k < n; k++) {
        W[k] = A[(n + 1) * k];
        if (k < n - 1) {
            int m = k + 1;
            float mv = fabsf(A[n * k + m]);
            for (int i = k + 2; i < n; i++) {
                const float val = fabsf(A[n * k + i]);
                if (mv < val) mv = val, m = i;
            }
            indR[k] = m;
        }
        if (k > 0) {
            int m = 0;
            float mv = fabsf(A[k]);
            for (int i = 1; i < k; i++) {
                const float val = fabsf(A[n * i + k]);
                if (mv < val) mv = val, m = i;
            }
            indC[k] = m;
        }
    }
    for (int iters = 0; iters < n * n * 30; iters++) {
        int k = 0;
        float mv = fabsf(A[indR[0]]);
        for (int i = 1; i < n - 1; i++) {
            const float val = fabsf(A[n * i + indR[i]]);
            if (mv < val) mv = val, k = i;
        }
        int l = indR[k];
        for (int i = 1; i < n; i++) {
            const float val = fabsf(A[n * indC[i] + i]);
            if (mv < val) mv = val, k = indC[i], l = i;
        }
        const float p = A[n * k + l];
        if (fabsf(p) <= eps) break;
        const float y = (W[l] - W[k]) * 0.5f;
        float t = fabsf(y) + hypot_f(p, y);
        float s = hypot_f(p, t);
        const float c = t / s;
        s = p / s;
        t = (p / t) * p;
        if (y < 0) s = -s, t = -t;
        A[n * k + l] = 0;
        W[k] -= t;
        W[l] += t;
        float a0, b0;
#define GF_SIM3_ROT(v0, v1) a0 = v0, b0 = v1, v0 = a0 * c - b0 * s, v1 = a0 * s + b0 * c
        for (int i = 0; i < k; i++) GF_SIM3_ROT(A[n * i + k], A[n * i + l]);
        for (int i = k + 1; i < l; i++) GF_SIM3_ROT(A[n * k + i], A[n * i + l]);
        for (int i = l + 1; i < n; i++) GF_SIM3_ROT(A[n * k + i], A[n * l + i]);
        for (int i = 0; i < n; i++) GF_SIM3_ROT(V[n * k + i], V[n * l + i]);
#undef GF_SIM3_ROT
        for (int j = 0; j < 2; j++) {
            const int idx = j == 0 ? k : l;
            if (idx < n - 1) {
                int m = idx + 1;
                float mx = fabsf(A[n * idx + m]);
                for (int i = idx + 2; i < n; i++) {
                    const float val = fabsf(A[n * idx + i]);
                    if (mx < val) mx = val, m = i;
                }
                indR[idx] = m;
            }
            if (idx > 0) {
                int m = 0;
                float mx = fabsf(A[idx]);
                for (int i = 1; i < idx; i++) {
                    const float val = fabsf(A[n * i + idx]);
                    if (mx < val) mx = val, m = i;
                }
                indC[idx] = m;
            }
        }
    }
    for (int k = 0; k < n - 1; k++) {
        int m = k;
        for (int i = k + 1; i < n; i++)
            if (W[m] < W[i]) m = i;
        if (k != m) {
            const float w = W[m];
            W[m] = W[k];
            W[k] = w;
            for (int i = 0; i < n; i++) {
                const float v = V[n * m + i];
                V[n * m + i] = V[n * k + i];
                V[n * k + i] = v;
            }
        }
    }
}

// centroid (:215-224): cv::reduce sums a row as (p0 + p2) + p1, C = C/3 scales
// by (float)(1./3); P is [coordinate][point]
__device__ __forceinline__ void centroid(const float P[3][3], float Pr[3][3], float C[3]) {
    const float third = (float)(1. / 3);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        C[k] = ((P[k][0] + P[k][2]) + P[k][1]) * third;
#pragma unroll
        for (int i = 0; i < 3; i++) Pr[k][i] = P[k][i] - C[k];
    }
}

// computeT (:226-332) by one lane. P1/P2: [coordinate][point]. H receives the
// hypothesis record (T12[16] R[9] t[3] s), T21 the 3x4 inverse. lds: 44 words.
__device__ void compute_T(const float P1[3][3], const float P2[3][3], float* H, float* T21, float* lds) {
    float* A = lds;
    float* V = lds + 16;
    float* W = lds + 32;
    int* ind = (int*)(lds + 36);
    float Pr1[3][3], Pr2[3][3], O1[3], O2[3];
    centroid(P1, Pr1, O1);
    centroid(P2, Pr2, O2);
    float M[3][3];  // Pr2 * Pr1^T
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) M[a][b] = (Pr2[a][0] * Pr1[b][0] + Pr2[a][1] * Pr1[b][1]) + Pr2[a][2] * Pr1[b][2];
    const float N11 = M[0][0] + M[1][1] + M[2][2], N12 = M[1][2] - M[2][1], N13 = M[2][0] - M[0][2],
                N14 = M[0][1] - M[1][0], N22 = M[0][0] - M[1][1] - M[2][2], N23 = M[0][1] + M[1][0],
                N24 = M[2][0] + M[0][2], N33 = -M[0][0] + M[1][1] - M[2][2], N34 = M[1][2] + M[2][1],
                N44 = -M[0][0] - M[1][1] + M[2][2];
    A[0] = N11, A[1] = N12, A[2] = N13, A[3] = N14;
    A[4] = N12, A[5] = N22, A[6] = N23, A[7] = N24;
    A[8] = N13, A[9] = N23, A[10] = N33, A[11] = N34;
    A[12] = N14, A[13] = N24, A[14] = N34, A[15] = N44;
    jacobi4(A, V, W, ind);
    const float q0 = V[0], v0 = V[1], v1 = V[2], v2 = V[3];
    const double nrm = sqrt((double)v0 * v0 + (double)v1 * v1 + (double)v2 * v2);
    const double ang = atan2(nrm, (double)q0);
    const float alpha = (float)((2 * ang) * (1. / nrm));
    // cv::Rodrigues, vector -> matrix, in double
    double rx = v0 * alpha, ry = v1 * alpha, rz = v2 * alpha;
    const double theta = sqrt(rx * rx + ry * ry + rz * rz);
    float R[3][3];
    if (theta < 2.220446049250313e-16) {
#pragma unroll
        for (int a = 0; a < 3; a++)
#pragma unroll
            for (int b = 0; b < 3; b++) R[a][b] = a == b ? 1.f : 0.f;
    } else {
        const double c = cos(theta), s = sin(theta), c1 = 1. - c, itheta = 1. / theta;
        rx *= itheta, ry *= itheta, rz *= itheta;
        R[0][0] = (float)(c + c1 * (rx * rx) + s * 0.);
        R[0][1] = (float)(c * 0. + c1 * (rx * ry) + s * -rz);
        R[0][2] = (float)(c * 0. + c1 * (rx * rz) + s * ry);
        R[1][0] = (float)(c * 0. + c1 * (rx * ry) + s * rz);
        R[1][1] = (float)(c + c1 * (ry * ry) + s * 0.);
        R[1][2] = (float)(c * 0. + c1 * (ry * rz) + s * -rx);
        R[2][0] = (float)(c * 0. + c1 * (rx * rz) + s * -ry);
        R[2][1] = (float)(c * 0. + c1 * (ry * rz) + s * rx);
        R[2][2] = (float)(c + c1 * (rz * rz) + s * 0.);
    }
    float P3[3][3];  // R * Pr2
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int i = 0; i < 3; i++) P3[a][i] = (R[a][0] * Pr2[0][i] + R[a][1] * Pr2[1][i]) + R[a][2] * Pr2[2][i];
    // Mat::dot: double accumulation, four products per step, then one by one
    double nom = 0;
    nom += (double)Pr1[0][0] * P3[0][0] + (double)Pr1[0][1] * P3[0][1] + (double)Pr1[0][2] * P3[0][2] +
           (double)Pr1[1][0] * P3[1][0];
    nom += (double)Pr1[1][1] * P3[1][1] + (double)Pr1[1][2] * P3[1][2] + (double)Pr1[2][0] * P3[2][0] +
           (double)Pr1[2][1] * P3[2][1];
    nom += (double)Pr1[2][2] * P3[2][2];
    double den = 0;
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int i = 0; i < 3; i++) den += P3[a][i] * P3[a][i];
    const float sc = (float)(nom / den);
    float t[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float ro = (R[a][0] * O2[0] + R[a][1] * O2[1]) + R[a][2] * O2[2];
        t[a] = O1[a] - (float)((double)sc * (double)ro);
    }
    const float isc = (float)(1.0 / (double)sc);
#pragma unroll
    for (int a = 0; a < 3; a++) {
        float si[3];
#pragma unroll
        for (int b = 0; b < 3; b++) {
            H[a * 4 + b] = R[a][b] * sc;
            H[16 + a * 3 + b] = R[a][b];
            si[b] = R[b][a] * isc;
            T21[a * 4 + b] = si[b];
        }
        H[a * 4 + 3] = t[a];
        H[25 + a] = t[a];
        T21[a * 4 + 3] = -((si[0] * t[0] + si[1] * t[1]) + si[2] * t[2]);
    }
    H[12] = H[13] = H[14] = 0.f;
    H[15] = 1.f;
    H[28] = sc;
    H[29] = H[30] = H[31] = 0.f;
}

// mvnMaxError is a vector<size_t> (Sim3Solver.h:79-80): 9.210*sigma2 truncated
__device__ __forceinline__ float max_error(float sigma2) {
    return (float)(unsigned long long)(9.210 * (double)sigma2);
}

// Project (:377-398): K * (T[0:3,0:3] X + T[0:3,3]), T a row-major 3x4
__device__ __forceinline__ void project(const float* T, float x, float y, float z, const Cam& k, float* u, float* v) {
    const float X = ((T[0] * x + T[1] * y) + T[2] * z) + T[3];
    const float Y = ((T[4] * x + T[5] * y) + T[6] * z) + T[7];
    const float Z = ((T[8] * x + T[9] * y) + T[10] * z) + T[11];
    const float invz = 1 / Z;
    *u = k.fx * (X * invz) + k.cx;
    *v = k.fy * (Y * invz) + k.cy;
}

// CheckInliers (:335-359) for one correspondence; NaN errors compare false
__device__ __forceinline__ bool is_inlier(const float* x1, const float* x2, float s1, float s2, const float* T12,
                                          const float* T21, const Cam& k1, const Cam& k2) {
    // FromCameraToImage (:400-418)
    const float iz1 = 1 / x1[2], iz2 = 1 / x2[2];
    const float u1 = k1.fx * (x1[0] * iz1) + k1.cx, v1 = k1.fy * (x1[1] * iz1) + k1.cy;
    const float u2 = k2.fx * (x2[0] * iz2) + k2.cx, v2 = k2.fy * (x2[1] * iz2) + k2.cy;
    float pu, pv, qu, qv;
    project(T12, x2[0], x2[1], x2[2], k1, &pu, &pv);  // vP2im1
    project(T21, x1[0], x1[1], x1[2], k2, &qu, &qv);  // vP1im2
    const float d1x = u1 - pu, d1y = v1 - pv, d2x = qu - u2, d2y = qv - v2;
    const float err1 = (float)((double)d1x * d1x + (double)d1y * d1y);
    const float err2 = (float)((double)d2x * d2x + (double)d2y * d2y);
    return err1 < max_error(s1) && err2 < max_error(s2);
}

}  // namespace
}  // namespace gfsim3
