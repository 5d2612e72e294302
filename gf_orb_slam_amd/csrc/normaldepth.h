// MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:285-324) of one point, in
// pieces a kernel calls while it walks the point's observations in
// observation-map order: the arithmetic of gf_update_normal_and_depth
// (neighbors.hip) and of the initial map's points (initmap.hip).
// cv::norm is a double sum cast to float and Mat / scalar one float factor
// (float)(1 / scalar) (docs/ORACLE_ASSUMPTIONS.md A22).
#pragma once
#include "common.h"

namespace gfnd {

__device__ __forceinline__ float norm3(const float* d) {  // cv::norm: a double sum, cast to float
    return (float)sqrt(((double)d[0] * d[0] + (double)d[1] * d[1]) + (double)d[2] * d[2]);
}

// Ow = -Rcw^T tcw of a row-major 4x4 (or 3x4) pose (KeyFrame::SetPose): float
// products summed left to right, then the sign
__device__ __forceinline__ void camera_center(const float* T, float* Ow) {
#pragma unroll
    for (int c = 0; c < 3; c++) Ow[c] = -((T[c] * T[3] + T[4 + c] * T[7]) + T[8 + c] * T[11]);
}

// one observation of the sum at :302-309: nr += (X - Ow) / cv::norm(X - Ow)
__device__ __forceinline__ void add_view(const float* X, const float* Ow, float* nr) {
    const float d[3] = {X[0] - Ow[0], X[1] - Ow[1], X[2] - Ow[2]};
    const float f = (float)(1.0 / (double)norm3(d));  // normali / cv::norm(normali): one float factor
#pragma unroll
    for (int c = 0; c < 3; c++) nr[c] = nr[c] + d[c] * f;
}

// :311-322 with the sum nr over n observations: Ow_ref the reference
// keyframe's centre, sf its scale factor, scale_level = GetScaleFactor(level)
// and scale_mirror = GetScaleFactor(nLevels - 1 - level)
__device__ __forceinline__ void finish(const float* X, const float* Ow_ref, const float* nr, int n, float sf,
                                       float scale_level, float scale_mirror, float* normal, float& min_dist,
                                       float& max_dist) {
    const float PC[3] = {X[0] - Ow_ref[0], X[1] - Ow_ref[1], X[2] - Ow_ref[2]};
    const float dist = norm3(PC);
    min_dist = ((1.0f / sf) * dist) / scale_level;  // :320
    max_dist = (sf * dist) * scale_mirror;          // :321
    const float fn = (float)(1.0 / (double)n);      // normal / n (:322)
#pragma unroll
    for (int c = 0; c < 3; c++) normal[c] = nr[c] * fn;
}

}  // namespace gfnd
