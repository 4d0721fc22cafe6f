// The k best (value, index) of what ONE lane streams, sorted, in registers: the piece alts_step_kernel (step_alts.h) and the k-best form of the
// fused scoring kernel (score.h) share.  Order: value descending, and among equals the entry pushed first in front -- a lane pushes in
// ascending index, so that is "lower index first".  Every access is constant-indexed and unrolled (a dynamically indexed array would go to
// scratch).  An empty slot holds (`floor`, 0x7fffffff): nothing at or below `floor` ever enters, and no real index compares above it.
#pragma once
#include "common.h"

namespace txo {

constexpr int KBEST_MAX = 8;

struct KBest {
    float val[KBEST_MAX]; int idx[KBEST_MAX];
    __device__ inline void clear(float floor) {
#pragma unroll
        for (int s = 0; s < KBEST_MAX; ++s) { val[s] = floor; idx[s] = 0x7fffffff; }
    }
    // slot s takes its upper neighbour where v goes in front of that one, v itself where v goes in front of slot s only
    __device__ inline void push(float v, int j) {
#pragma unroll
        for (int s = KBEST_MAX - 1; s >= 1; --s) {
            const bool shift = v > val[s - 1], here = v > val[s];
            val[s] = shift ? val[s - 1] : (here ? v : val[s]);
            idx[s] = shift ? idx[s - 1] : (here ? j : idx[s]);
        }
        const bool here = v > val[0];
        val[0] = here ? v : val[0]; idx[0] = here ? j : idx[0];
    }
    __device__ inline void pop(float floor) {
#pragma unroll
        for (int s = 0; s + 1 < KBEST_MAX; ++s) { val[s] = val[s + 1]; idx[s] = idx[s + 1]; }
        val[KBEST_MAX - 1] = floor; idx[KBEST_MAX - 1] = 0x7fffffff;
    }
};

}  // namespace txo
