// fusion_shared.h -- what fusion_tile.h (the forward kernel) and fusion_grad_tile.h (the backward kernel) both need, stated once so
// that one unit (fusion_lengths.hip) can include the two: the layer's shape, the wave reductions and the liveness rule of the
// per-cloud-length forms.
#pragma once
#include "common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int C1 = 64, C2 = 64, C3 = 128, NB = 64;  // layer widths 4 -> 64 -> 64 -> 128  // mocopci.py:749-755, fusion k = 32 + 32
constexpr int WAVES = 4;

// register r of lane half h of an accumulator tile -> its channel: mcp_chan_of (common.h)

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

// Per-cloud lengths: whether point p (of element bb) is live, p - bb n < min(max(len[bb], 0), n).  A wave walks one point, so the
// answer is the same in every lane: read from the first, the length is a scalar load and the step over a padded point a scalar branch.
__device__ __forceinline__ bool fusion_live(const int *__restrict__ len, long long p, long long bb, int n) {
    const int b1 = __builtin_amdgcn_readfirstlane((int)bb), at = __builtin_amdgcn_readfirstlane((int)(p - bb * n));
    return at < min(max(len[b1], 0), n);
}

}  // namespace
