// OpenCV's small CV_32F matrix operations restated for the device, shared by
// the monocular initializer (initializer.hip) and CreateNewMapPoints
// (newpoints.hip): the float Jacobi SVD, the 3x3 inverse / determinant, the
// small gemm, cv::norm, and the order-preserving float keys of the radix
// selects. docs/ORACLE_ASSUMPTIONS.md A1 / A17 list the readings.
#pragma once
#include <cfloat>
#include <cmath>

#include "common.h"

namespace gfcv {
namespace {

struct CvRng {  // cv::RNG
    uint64_t state;
    __device__ unsigned next() {
        state = (uint64_t)(unsigned)state * 4164903690ULL + (unsigned)(state >> 32);
        return (unsigned)state;
    }
};

// JacobiSVDImpl_<float> (eps 2 FLT_EPSILON, minval FLT_MIN): At holds N rows of
// length M (M x M storage, rows >= N zero); W singular values, Vt (N x N) the
// right vectors as rows. N1 > 0 completes/normalises rows 0..N1-1 of At (the
// left vectors, with cv::RNG(0x12345678) for null ones); N1 = 0 skips that
// step, which touches nothing but the left vectors.
template <int M, int N, int N1>
__device__ void jacobi_f(float* At, float* Wout, float* Vt) {
    const double minval = FLT_MIN;
    const float eps = FLT_EPSILON * 2;
    double W[N];
    constexpr int max_iter = M > 30 ? M : 30;
#pragma unroll
    for (int i = 0; i < N; i++) {
        double sd = 0;
#pragma unroll
        for (int k = 0; k < M; k++) {
            const float t = At[i * M + k];
            sd += (double)t * (double)t;
        }
        W[i] = sd;
#pragma unroll
        for (int k = 0; k < N; k++) Vt[i * N + k] = 0.f;
        Vt[i * N + i] = 1.f;
    }
    for (int iter = 0; iter < max_iter; iter++) {
        bool changed = false;
#pragma unroll
        for (int i = 0; i < N - 1; i++)
#pragma unroll
            for (int j = i + 1; j < N; j++) {
                float *Ai = At + i * M, *Aj = At + j * M;
                double a = W[i], p = 0, b = W[j];
#pragma unroll
                for (int k = 0; k < M; k++) p += (double)Ai[k] * (double)Aj[k];
                if (fabs(p) <= (double)eps * sqrt(a * b)) continue;
                p *= 2;
                const double beta = a - b, gamma = sqrt(p * p + beta * beta);
                float c, s;
                if (beta < 0) {
                    const double delta = (gamma - beta) * 0.5;
                    s = (float)sqrt(delta / gamma);
                    c = (float)(p / (gamma * (double)s * 2));
                } else {
                    c = (float)sqrt((gamma + beta) / (gamma * 2));
                    s = (float)(p / (gamma * (double)c * 2));
                }
                a = b = 0;
#pragma unroll
                for (int k = 0; k < M; k++) {
                    const float t0 = c * Ai[k] + s * Aj[k];
                    const float t1 = -s * Ai[k] + c * Aj[k];
                    Ai[k] = t0;
                    Aj[k] = t1;
                    a += (double)t0 * (double)t0;
                    b += (double)t1 * (double)t1;
                }
                W[i] = a;
                W[j] = b;
                changed = true;
                float *Vi = Vt + i * N, *Vj = Vt + j * N;
#pragma unroll
                for (int k = 0; k < N; k++) {
                    const float t0 = c * Vi[k] + s * Vj[k];
                    const float t1 = -s * Vi[k] + c * Vj[k];
                    Vi[k] = t0;
                    Vj[k] = t1;
                }
            }
        if (!changed) break;
    }
#pragma unroll
    for (int i = 0; i < N; i++) {
        double sd = 0;
#pragma unroll
        for (int k = 0; k < M; k++) {
            const float t = At[i * M + k];
            sd += (double)t * (double)t;
        }
        W[i] = sqrt(sd);
    }
    // selection sort, descending (compile-time indices: the swaps are selects)
#pragma unroll
    for (int i = 0; i < N - 1; i++) {
        int j = i;
#pragma unroll
        for (int k = i + 1; k < N; k++)
            if (W[j] < W[k]) j = k;
#pragma unroll
        for (int k = i + 1; k < N; k++) {
            if (j != k) continue;
            const double tw = W[i];
            W[i] = W[k];
            W[k] = tw;
#pragma unroll
            for (int q = 0; q < M; q++) {
                const float t = At[i * M + q];
                At[i * M + q] = At[k * M + q];
                At[k * M + q] = t;
            }
#pragma unroll
            for (int q = 0; q < N; q++) {
                const float t = Vt[i * N + q];
                Vt[i * N + q] = Vt[k * N + q];
                Vt[k * N + q] = t;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < N; i++) Wout[i] = (float)W[i];
    if constexpr (N1 > 0) {
        CvRng rng{0x12345678};
        for (int i = 0; i < N1; i++) {
            double sd = i < N ? W[i < N ? i : 0] : 0.;
            for (int ii = 0; ii < 100 && sd <= minval; ii++) {
                const float val0 = (float)(1. / M);
                for (int k = 0; k < M; k++) At[i * M + k] = (rng.next() & 256) != 0 ? val0 : -val0;
                for (int it = 0; it < 2; it++)
                    for (int j = 0; j < i; j++) {
                        sd = 0;
                        for (int k = 0; k < M; k++) sd += (double)(At[i * M + k] * At[j * M + k]);
                        float asum = 0;
                        for (int k = 0; k < M; k++) {
                            const float t = (float)((double)At[i * M + k] - sd * (double)At[j * M + k]);
                            At[i * M + k] = t;
                            asum += fabsf(t);
                        }
                        asum = asum > eps * 100 ? 1 / asum : 0;
                        for (int k = 0; k < M; k++) At[i * M + k] *= asum;
                    }
                sd = 0;
                for (int k = 0; k < M; k++) {
                    const float t = At[i * M + k];
                    sd += (double)t * (double)t;
                }
                sd = sqrt(sd);
            }
            const float s = (float)(sd > minval ? 1 / sd : 0.);
            for (int k = 0; k < M; k++) At[i * M + k] *= s;
        }
    }
}

// cv::SVD::compute(A R x C, FULL_UV) on CV_32F: Ta is an M x M work buffer
// (M = max(R, C)); u (R x R) only when FULLU.
template <int R, int C, bool FULLU>
__device__ void svd_f(const float* A, float* Ta, float* w, float* u, float* vt) {
    constexpr bool at = R < C;
    constexpr int M = at ? C : R, N = at ? R : C;
#pragma unroll
    for (int i = 0; i < M * M; i++) Ta[i] = 0.f;
#pragma unroll
    for (int i = 0; i < N; i++)
#pragma unroll
        for (int k = 0; k < M; k++) Ta[i * M + k] = at ? A[i * C + k] : A[k * C + i];
    float V[N * N];
    jacobi_f<M, N, FULLU ? M : 0>(Ta, w, V);
    if constexpr (!at) {
        if constexpr (FULLU)
#pragma unroll
            for (int i = 0; i < R; i++)
#pragma unroll
                for (int j = 0; j < R; j++) u[i * R + j] = Ta[j * M + i];
#pragma unroll
        for (int i = 0; i < C * C; i++) vt[i] = V[i];
    } else {
        if constexpr (FULLU)
#pragma unroll
            for (int i = 0; i < R; i++)
#pragma unroll
                for (int j = 0; j < R; j++) u[i * R + j] = V[j * N + i];
#pragma unroll
        for (int i = 0; i < C * C; i++) vt[i] = Ta[i];
    }
}

// small cv::gemm (docs A1): float products summed left to right, then the
// MatExpr scale as a double multiply rounded to float
template <int R, int K, int C>
__device__ void gemm_f(const float* A, const float* B, float* D, double alpha = 1.0) {
    float out[R * C];
#pragma unroll
    for (int i = 0; i < R; i++)
#pragma unroll
        for (int j = 0; j < C; j++) {
            float s = A[i * K] * B[j];
#pragma unroll
            for (int q = 1; q < K; q++) s = s + A[i * K + q] * B[q * C + j];
            out[i * C + j] = alpha == 1.0 ? s : (float)((double)s * alpha);
        }
#pragma unroll
    for (int i = 0; i < R * C; i++) D[i] = out[i];
}

__device__ void transpose3(const float* A, float* T) {
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) T[j * 3 + i] = A[i * 3 + j];
}

__device__ double det3(const float* m) {
    return m[0] * ((double)m[4] * m[8] - (double)m[5] * m[7]) - m[1] * ((double)m[3] * m[8] - (double)m[5] * m[6]) +
           m[2] * ((double)m[3] * m[7] - (double)m[4] * m[6]);
}

__device__ void inv3(const float* S, float* D) {
    double d = det3(S);
    if (d == 0.) {
        for (int i = 0; i < 9; i++) D[i] = 0.f;
        return;
    }
    d = 1. / d;
    D[0] = (float)(((double)S[4] * S[8] - (double)S[5] * S[7]) * d);
    D[1] = (float)(((double)S[2] * S[7] - (double)S[1] * S[8]) * d);
    D[2] = (float)(((double)S[1] * S[5] - (double)S[2] * S[4]) * d);
    D[3] = (float)(((double)S[5] * S[6] - (double)S[3] * S[8]) * d);
    D[4] = (float)(((double)S[0] * S[8] - (double)S[2] * S[6]) * d);
    D[5] = (float)(((double)S[2] * S[3] - (double)S[0] * S[5]) * d);
    D[6] = (float)(((double)S[3] * S[7] - (double)S[4] * S[6]) * d);
    D[7] = (float)(((double)S[1] * S[6] - (double)S[0] * S[7]) * d);
    D[8] = (float)(((double)S[0] * S[4] - (double)S[1] * S[3]) * d);
}

__device__ double norm3(const float* v) {  // cv::norm NORM_L2 (double accumulation)
    double s = 0;
    for (int i = 0; i < 3; i++) s += (double)v[i] * (double)v[i];
    return sqrt(s);
}

__device__ void scale3(const float* v, double alpha, float* out) {  // MatExpr Mat / s
    const float a = (float)alpha;
    for (int i = 0; i < 3; i++) out[i] = v[i] * a;
}

__device__ __forceinline__ uint32_t ord_key(float c) {  // order-preserving float -> uint
    const uint32_t u = __float_as_uint(c);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_val(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

}  // namespace
}  // namespace gfcv
