// attention_forward.h -- the host side of the inference attention, stated once for attention.hip (mcp_attention, mcp_attention_small,
// mcp_attention_wide: no lengths) and attention_lengths.hip (mcp_attention_lengths: one AttnLengths behind every kernel's parameters),
// with the wide heads' __global__ wrappers around the bodies of attention_wide_fwd.h.  attention_forward_run holds the alignment /
// stride / rotation checks, the dispatch by head width, the key-split rule at width 256 and the grids, all from the PADDED sizes (the
// host never reads a length): a short element of a key-split launch leaves waves of its workgroups without a key stage, which the
// merge weighs with 0.  Each unit emits only the kernels of its own pack.
#pragma once
#include <type_traits>

#include "attention_small_fwd.h"  // attention_small_kernel; through it attention_wide_fwd.h: f32x16, WAVES, the wide-head kernels' bodies

namespace {

// keys / values of batch element (bf + kv_shift) mod BF (0 <= kv_shift < BF)
__device__ __forceinline__ int kv_batch(int kv_shift) {
    const int bkv = (int)blockIdx.z + kv_shift;
    return bkv >= (int)gridDim.z ? bkv - (int)gridDim.z : bkv;
}

// The wrappers keep one name per form (a kernel's symbol is its name in every profile and resource table), so they are two pairs;
// wide_kernel below picks by the pack.
template <int HD>
__global__ __launch_bounds__(64 * WAVES, 1) void attention_wide_kernel(int nq, int nk, const float *__restrict__ q, int qs,
                                                                       const float *__restrict__ k, int ks, const float *__restrict__ v,
                                                                       int vs, float scale_log2e, float *__restrict__ out, int os, int kv_shift) {
    extern __shared__ __attribute__((aligned(16))) float lds_w[];
    attention_wide_body<HD, false>(lds_w, nq, nk, (int)gridDim.y, q, qs, k, ks, v, vs, kv_batch(kv_shift), scale_log2e, 0, 0, 0.f, out, os, nullptr);
}
template <int HD>
__global__ __launch_bounds__(64 * WAVES, 1) void attention_wide_lengths_kernel(int nq, int nk, const float *__restrict__ q, int qs,
                                                                               const float *__restrict__ k, int ks, const float *__restrict__ v,
                                                                               int vs, float scale_log2e, float *__restrict__ out, int os,
                                                                               int kv_shift, AttnLengths len) {
    extern __shared__ __attribute__((aligned(16))) float lds_w[];
    attention_wide_body<HD, false>(lds_w, nq, nk, (int)gridDim.y, q, qs, k, ks, v, vs, kv_batch(kv_shift), scale_log2e, 0, 0, 0.f, out, os, nullptr,
                                   len);
}

// the keys split over the waves of a workgroup
template <int HD>
__global__ __launch_bounds__(64 * WAVES, 1) void attention_wide_ksplit_kernel(int nq, int nk, const float *__restrict__ q, int qs,
                                                                              const float *__restrict__ k, int ks, const float *__restrict__ v,
                                                                              int vs, float scale_log2e, float *__restrict__ out, int os, int kv_shift) {
    extern __shared__ __attribute__((aligned(16))) float lds_ws[];
    attention_wide_ksplit_body<HD, false>(lds_ws, nq, nk, (int)gridDim.y, q, qs, k, ks, v, vs, kv_batch(kv_shift), scale_log2e, 0, 0, 0.f, out, os,
                                          nullptr);
}
template <int HD>
__global__ __launch_bounds__(64 * WAVES, 1) void attention_wide_ksplit_lengths_kernel(int nq, int nk, const float *__restrict__ q, int qs,
                                                                                      const float *__restrict__ k, int ks,
                                                                                      const float *__restrict__ v, int vs, float scale_log2e,
                                                                                      float *__restrict__ out, int os, int kv_shift,
                                                                                      AttnLengths len) {
    extern __shared__ __attribute__((aligned(16))) float lds_ws[];
    attention_wide_ksplit_body<HD, false>(lds_ws, nq, nk, (int)gridDim.y, q, qs, k, ks, v, vs, kv_batch(kv_shift), scale_log2e, 0, 0, 0.f, out, os,
                                          nullptr, len);
}

template <int HD, bool SPLIT, class... L>
constexpr auto wide_kernel() {
    constexpr bool LEN = sizeof...(L) != 0;
    if constexpr (SPLIT && LEN) return attention_wide_ksplit_lengths_kernel<HD>;
    else if constexpr (SPLIT) return attention_wide_ksplit_kernel<HD>;
    else if constexpr (LEN) return attention_wide_lengths_kernel<HD>;
    else return attention_wide_kernel<HD>;
}

// One forward launch; hd is one of 8 / 16 / 32 / 64 / 256 (the callers' check: the entry points differ in the widths they take).
// lens: empty, or one AttnLengths.
template <class... L>
int attention_forward_run(int bf, int nq, int nk, int heads, int hd, const float *q, int q_stride, const float *k, int k_stride, const float *v,
                          int v_stride, int kv_shift, float scale, float *out, int out_stride, hipStream_t s, L... lens) {
    // float4 accesses: every row start and head offset must be 16-byte aligned
    if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out) & 15) return MCP_ERR_BAD_ARG;
    if ((q_stride | k_stride | v_stride | out_stride) & 3) return MCP_ERR_BAD_ARG;
    if (kv_shift < 0 || kv_shift >= bf) return MCP_ERR_BAD_ARG;
    const float sl2 = scale * 1.44269504088896340736f;
    const dim3 block(64 * WAVES);
    auto small = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(mcp_divup(nq, 32 * WAVES), heads, bf), block, 0, s, nq, nk, heads, q, q_stride, k, k_stride, v, v_stride, sl2, out,
                           out_stride, kv_shift, lens...);
        return mcp_launch_status();
    };
    auto wide = [&](auto width, auto split) {   // as compile-time constants; split: a wave takes 32 queries and a share of the keys
        constexpr int HD = decltype(width)::value;
        constexpr bool SPLIT = decltype(split)::value;
        constexpr auto kern = wide_kernel<HD, SPLIT, L...>();
        using Cfg = std::conditional_t<SPLIT, WideSplitCfg<HD>, WideCfg<HD>>;
        if (const int rc = mcp_allow_lds<kern>()) return rc;
        hipLaunchKernelGGL(kern, dim3(mcp_divup(nq, SPLIT ? 32 : 32 * WAVES), heads, bf), block, Cfg::LDS_BYTES, s, nq, nk, q, q_stride, k, k_stride, v,
                           v_stride, sl2, out, out_stride, kv_shift, lens...);
        return mcp_launch_status();
    };
    using std::integral_constant;
    mcp_prof_begin(MCP_KERNEL_ATTENTION, s);
    const int rc = hd == 8    ? small(attention_small_kernel<8, L...>)
                   : hd == 16 ? small(attention_small_kernel<16, L...>)
                   : hd == 32 ? wide(integral_constant<int, 32>{}, std::false_type{})
                   : hd == 64 ? wide(integral_constant<int, 64>{}, std::false_type{})
                   : wide_keys_split(bf, nq, nk, heads) ? wide(integral_constant<int, 256>{}, std::true_type{})
                                                        : wide(integral_constant<int, 256>{}, std::false_type{});
    mcp_prof_end(MCP_KERNEL_ATTENTION, s);
    return rc;
}

}  // namespace
