// KeyFrame::ComputeSceneMedianDepth (src/KeyFrame.cc:659-689) in pieces: the
// depth of one map point in the keyframe and the exact selection of the
// element std::sort would put at a given rank, by a 4-pass radix select over
// order-preserving keys in LDS. Used by k_np_setup (newpoints.hip) and
// k_initmap_finish (initmap.hip).
#pragma once
#include "cvsvd_core.h"

namespace gfsel {

// z = (float)(Rcw.row(2).dot(x3Dw) + zcw): Mat::dot sums in double
__device__ __forceinline__ float scene_depth(const float* Tcw, const float* p) {
    const double d = (double)Tcw[8] * (double)p[0] + (double)Tcw[9] * (double)p[1] + (double)Tcw[10] * (double)p[2];
    return (float)(d + (double)Tcw[11]);
}

// The key (gfcv::ord_key) of rank `rank` (0-based, ascending) among keys[0, nd),
// nd > 0, 8 bits a pass. Called by all NT threads of the workgroup; keys, the
// 256 bins of hist and the two scalars live in LDS and the caller has
// synchronised after writing keys. Returns the same value in every thread; gfcv::key_val turns it back
// into the float.
template <int NT>
__device__ uint32_t radix_select(const uint32_t* keys, int nd, int rank, int* hist, uint32_t* s_prefix, int* s_rank) {
    const int tid = threadIdx.x;
    if (tid == 0) {
        *s_prefix = 0;
        *s_rank = rank;
    }
    for (int pass = 0; pass < 4; pass++) {
        const int shift = 24 - 8 * pass;
        const uint32_t mask = pass ? 0xffffffffu << (32 - 8 * pass) : 0u;
        for (int b = tid; b < 256; b += NT) hist[b] = 0;
        __syncthreads();
        const uint32_t pre = *s_prefix;
        for (int j = tid; j < nd; j += NT) {
            const uint32_t k = keys[j];
            if ((k & mask) == pre) atomicAdd(&hist[(k >> shift) & 255], 1);
        }
        __syncthreads();
        if (tid == 0) {
            int r = *s_rank, d = 0;
            while (d < 255 && r >= hist[d]) r -= hist[d++];
            *s_rank = r;
            *s_prefix = pre | ((uint32_t)d << shift);
        }
        __syncthreads();
    }
    return *s_prefix;
}

}  // namespace gfsel
