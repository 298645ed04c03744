// attention_dropout.h -- the attention dropout mask shared by every attention kernel that draws one (attention_grad.hip: head dims
// 8 / 16; attention_wide_grad.hip: head widths 32 / 64 / 256), forward and backward.
#pragma once
#include <stdint.h>

// Attention dropout (net.train(): mocopci.py:660-662 drops entries of the softmax matrix at rate 0.05).  The keep / drop decision of
// entry (row, key) is a counter-based hash of (seed, row, key) -- row = the query's index over (batch, head, query) -- so the forward
// and both backward kernels regenerate the same mask without storing it.  m = 1 / (1 - p) for a kept entry, 0 for a dropped one.
__device__ __forceinline__ float drop_scale(uint32_t seed, uint32_t row, uint32_t key, uint32_t threshold, float inv_keep) {
    uint32_t x = seed ^ (row * 0x9E3779B1u) ^ (key * 0x85EBCA77u);
    x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16;
    return x >= threshold ? inv_keep : 0.f;
}

// drop probability -> (threshold of the 32-bit hash below which an entry is dropped, 1 / (1 - p))
static inline bool drop_params(float drop_p, uint32_t *threshold, float *inv_keep) {
    if (!(drop_p >= 0.f && drop_p < 1.f)) return false;
    *threshold = (uint32_t)((double)drop_p * 4294967296.0);
    *inv_keep = (float)(1.0 / (1.0 - (double)drop_p));
    return true;
}
