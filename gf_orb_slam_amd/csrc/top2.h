// Wave-level pieces shared by the window matchers that walk their queries in
// order (reloc.hip, searchinit.hip): the reference's best / second-best loop
// over a candidate sequence split across the lanes, the rotation bin and
// ComputeThreeMaxima.
#pragma once
#include <climits>

#include "match_common.h"

// best / second best / position / keypoint of a candidate sequence
struct Top2 {
    int d1, p1, i1, d2;
};

__device__ __forceinline__ Top2 top2_init() { return Top2{INT_MAX, INT_MAX, -1, INT_MAX}; }

// The reference's loop: dist < best -> second = best, best = dist; else dist < second -> second = dist.
__device__ __forceinline__ void top2_push(Top2& t, int d, int pos, int idx) {
    if (d < t.d1) {
        t.d2 = t.d1;
        t.d1 = d;
        t.p1 = pos;
        t.i1 = idx;
    } else if (d < t.d2) {
        t.d2 = d;
    }
}

// Lanes hold disjoint, position-ordered parts of the sequence: the merged
// best is the smaller distance (ties: earlier position) and the second best
// the smaller of the winner's second and the loser's best.
__device__ __forceinline__ Top2 top2_reduce(Top2 t) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int od1 = __shfl_xor(t.d1, o, 64), op1 = __shfl_xor(t.p1, o, 64);
        const int oi1 = __shfl_xor(t.i1, o, 64), od2 = __shfl_xor(t.d2, o, 64);
        if (od1 < t.d1 || (od1 == t.d1 && op1 < t.p1)) {
            t.d2 = min(od2, t.d1);
            t.d1 = od1;
            t.p1 = op1;
            t.i1 = oi1;
        } else {
            t.d2 = min(t.d2, od1);
        }
    }
    return t;
}

__device__ __forceinline__ int rot_bin(float a1, float a2) {
    float rot = a1 - a2;
    if (rot < 0.0) rot += 360.0f;
    int bin = (int)roundf(rot * (1.0f / HISTO_LENGTH));
    if (bin == HISTO_LENGTH) bin = 0;
    return bin;
}

// ComputeThreeMaxima (ORBmatcher.cc:2338-2379) over the bin counts: keep[0..2]
// = ind1, ind2, ind3 (-1: none). One lane calls it.
__device__ __forceinline__ void three_maxima(const int* hist, int* keep) {
    int max1 = 0, max2 = 0, max3 = 0, ind1 = -1, ind2 = -1, ind3 = -1;
    for (int i = 0; i < HISTO_LENGTH; i++) {
        const int s = hist[i];
        if (s > max1) {
            max3 = max2;
            max2 = max1;
            max1 = s;
            ind3 = ind2;
            ind2 = ind1;
            ind1 = i;
        } else if (s > max2) {
            max3 = max2;
            max2 = s;
            ind3 = ind2;
            ind2 = i;
        } else if (s > max3) {
            max3 = s;
            ind3 = i;
        }
    }
    if (max2 < 0.1f * (float)max1) {
        ind2 = -1;
        ind3 = -1;
    } else if (max3 < 0.1f * (float)max1) {
        ind3 = -1;
    }
    keep[0] = ind1;
    keep[1] = ind2;
    keep[2] = ind3;
}
