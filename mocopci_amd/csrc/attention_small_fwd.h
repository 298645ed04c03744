// attention_small_fwd.h -- the inference forward of the narrow-head attention (head dims 8 / 16), stated once for mcp_attention /
// mcp_attention_small (attention.hip) and mcp_attention_lengths (attention_lengths.hip: the same kernel with one AttnLengths behind its
// parameters); both launch it through attention_forward_run (attention_forward.h).  The arrangement is described at the head of attention.hip.
#pragma once
#include "attention_wide_fwd.h"  // f32x16, WAVES; attention_lengths.h

namespace {

typedef mcp_f2 f2;  // scalar pair: see common.h (no packed-fp32 instructions)
constexpr int KT = 64;  // keys per LDS stage (two 32-key MFMA tiles)

// lens: empty (attention.hip: the plain kernel) or one AttnLengths (attention_lengths.hip: the key loop ends at the element's own
// length kl, rows at or beyond ql are zeros, an element without keys is zeros)
template <int HD, class... L>
__global__ __launch_bounds__(64 * WAVES) void attention_small_kernel(int nq, int nk, int heads, const float *__restrict__ q, int qs,
                                                                     const float *__restrict__ k, int ks, const float *__restrict__ v,
                                                                     int vs, float scale_log2e, float *__restrict__ out, int os, int kv_shift,
                                                                     L... lens) {
    constexpr bool LEN = sizeof...(L) != 0;
    constexpr int KS = HD + 1;  // padded K row stride (floats): A-operand reads are conflict-free
    __shared__ float kt[2][KT * KS];
    __shared__ __attribute__((aligned(16))) float vt[2][KT * HD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, col = lane & 31;
    const int head = blockIdx.y, bf = blockIdx.z;
    const int qi = blockIdx.x * (32 * WAVES) + wave * 32 + col;
    const int ql = attn_qlen(nq, bf, lens...);   // the element's own lengths (nq, nk without)
    const bool live = qi < ql;
    q += ((size_t)bf * nq + (live ? qi : 0)) * qs + head * HD;
    int bkv = bf + kv_shift;  // keys / values of batch element (bf + kv_shift) mod BF (0 <= kv_shift < BF)
    if (bkv >= (int)gridDim.z) bkv -= (int)gridDim.z;
    const int kl = attn_klen(nk, bkv, lens...);
    if constexpr (LEN) {
        // a query block wholly beyond the length, or an element without keys: zeros, before anything is loaded
        if ((int)blockIdx.x * (32 * WAVES) >= ql || kl == 0) {
            if (qi < nq) attn_zero_row<HD / 2>(out + ((size_t)bf * nq + qi) * os + head * HD + h * (HD / 2));
            return;
        }
    }
    k += (size_t)bkv * nk * ks + head * HD;
    v += (size_t)bkv * nk * vs + head * HD;

    // B operand: Q[query][2s + h], pre-scaled so that p = exp2(s - m)
    float qf[HD / 2];
#pragma unroll
    for (int s = 0; s < HD / 2; ++s) qf[s] = q[2 * s + h] * scale_log2e;

    float m = -INFINITY, l = 0.f;
    // output accumulators as float pairs: P.V runs on v_pk_fma_f32 (two fma per lane and instruction)
    f2 o[HD / 2];
#pragma unroll
    for (int d = 0; d < HD / 2; ++d) o[d] = f2{0.f, 0.f};

    // stage loader: thread t loads one float4 of K or V
    constexpr int F4_PER_TILE = KT * HD / 4;                 // float4s per K (or V) stage
    constexpr int LOADS = (2 * F4_PER_TILE + 64 * WAVES - 1) / (64 * WAVES);
    float4 pre[LOADS];
    auto fetch = [&](int t) {
#pragma unroll
        for (int u = 0; u < LOADS; ++u) {
            const int e = tid + u * 64 * WAVES;
            const bool isv = e >= F4_PER_TILE;
            const int f = isv ? e - F4_PER_TILE : e;
            const int row = f / (HD / 4), c4 = f % (HD / 4);
            const int key = t * KT + row;
            pre[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (e < 2 * F4_PER_TILE && key < kl) {
                const float *src = (isv ? v + (size_t)key * vs : k + (size_t)key * ks) + c4 * 4;
                pre[u] = *reinterpret_cast<const float4 *>(src);
            }
        }
    };
    auto stash = [&](int buf) {
#pragma unroll
        for (int u = 0; u < LOADS; ++u) {
            const int e = tid + u * 64 * WAVES;
            if (e >= 2 * F4_PER_TILE) continue;
            const bool isv = e >= F4_PER_TILE;
            const int f = isv ? e - F4_PER_TILE : e;
            const int row = f / (HD / 4), c4 = f % (HD / 4);
            if (isv) {
                *reinterpret_cast<float4 *>(&vt[buf][row * HD + c4 * 4]) = pre[u];
            } else {
                float *dst = &kt[buf][row * KS + c4 * 4];
                dst[0] = pre[u].x; dst[1] = pre[u].y; dst[2] = pre[u].z; dst[3] = pre[u].w;
            }
        }
    };

    const int stages = (kl + KT - 1) / KT;
    fetch(0);
    stash(0);
    for (int t = 0; t < stages; ++t) {
        const int cur = t & 1;
        if (t + 1 < stages) fetch(t + 1);
        __syncthreads();
#pragma unroll
        for (int sub = 0; sub < KT / 32; ++sub) {
            const float *ka = &kt[cur][(sub * 32 + col) * KS + h];
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
            for (int s = 0; s < HD / 2; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ka[2 * s], qf[s], acc, 0, 0, 0);
            // keys beyond kl must not contribute
            const int kbase = t * KT + sub * 32;
            if (kbase + 32 > kl) {
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (kbase + mcp_chan_of(r, h) >= kl) acc[r] = -INFINITY;
            }
            float mt = acc[0];
#pragma unroll
            for (int r = 1; r < 16; ++r) mt = fmaxf(mt, acc[r]);
            const float mn = fmaxf(m, mt);
            if (mn == -INFINITY) continue;  // this half has seen no valid key yet
            const float alpha = __builtin_amdgcn_exp2f(m - mn);
            m = mn;
            l *= alpha;
            const f2 alpha2 = {alpha, alpha};
#pragma unroll
            for (int d = 0; d < HD / 2; ++d) o[d] = o[d] * alpha2;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float p = __builtin_amdgcn_exp2f(acc[r] - mn);
                l += p;
                const float *vr = &vt[cur][(sub * 32 + mcp_chan_of(r, h)) * HD];
                const f2 p2 = {p, p};
#pragma unroll
                for (int d = 0; d < HD; d += 4) {
                    const float4 vv = *reinterpret_cast<const float4 *>(vr + d);
                    o[d / 2 + 0] = mcp_f2_fma(p2, f2{vv.x, vv.y}, o[d / 2 + 0]);
                    o[d / 2 + 1] = mcp_f2_fma(p2, f2{vv.z, vv.w}, o[d / 2 + 1]);
                }
            }
        }
        if (t + 1 < stages) stash(cur ^ 1);
    }
    // merge the two lane halves of each query (log-sum-exp combine)
    const float mo = __shfl_xor(m, 32), lo = __shfl_xor(l, 32);
    const float mm = fmaxf(m, mo);
    const float a0 = m == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(m - mm), a1 = mo == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(mo - mm);
    const float lsum = l * a0 + lo * a1;
    const float inv = 1.0f / lsum;
    float res[HD];
#pragma unroll
    for (int d = 0; d < HD; ++d) {
        const float od = (d & 1) ? o[d / 2].y : o[d / 2].x;
        res[d] = (od * a0 + __shfl_xor(od, 32) * a1) * inv;
    }
    if (live && h == 0) {
        float *dst = out + ((size_t)bf * nq + qi) * os + head * HD;
#pragma unroll
        for (int d = 0; d < HD; d += 4) *reinterpret_cast<float4 *>(dst + d) = make_float4(res[d], res[d + 1], res[d + 2], res[d + 3]);
    }
    if constexpr (LEN) {
        if (!live && qi < nq && h == 0) attn_zero_row<HD>(out + ((size_t)bf * nq + qi) * os + head * HD);
    }
}

}  // namespace
