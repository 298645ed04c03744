// attention.hip -- fp32 flash-style attention for tiny head dims (8, 16) on gfx950.
//
// Caller-side block of the hot path: InterFrameAttentionInterpretation
// (mocopci.py:650-667: [5 frames x B, 8 heads, N<=2048 tokens, head_dim 8/16]) and CrossAttention of the
// EI cross-formers (mocopci.py:72-86).  The reference materialises the (heads, N, N) score tensor
// (640 MiB per sample at N=2048).  Library flash kernels pad head_dim 8 to their MFMA K and run far from
// the exp/FMA floor, so:
//   * a wave owns 32 queries (MFMA column = lane & 31); S^T = K . Q^T per 32-key tile is hd/2
//     v_mfma_f32_32x32x2_f32 (exact fp32) with Q (pre-scaled by scale*log2 e) resident in VGPRs and the
//     K tile read from a padded LDS image (bank-conflict-free);
//   * lane-half h ends up with 16 of the tile's 32 keys for its query and runs its OWN online softmax
//     stream (max, sum, O[hd]) over them -- no cross-lane traffic per tile; the two halves are merged
//     once at the end;
//   * P.V (N = hd = 8/16 columns) would waste 3/4 of an MFMA, so it runs on packed fp32 FMAs with V rows
//     read as LDS broadcasts;
//   * q, k, v are read in place from the projection outputs (row strides), out is written token-major,
//     so no permute/contiguous copies surround the call.
#include "attention_small_fwd.h"  // attention_small_kernel; through it attention_wide_fwd.h: f32x16, WAVES, chan_of, the wide-head kernels' bodies

namespace {

// ---- wide heads: the bodies are in attention_wide_fwd.h.  Keys / values of batch element (bf + kv_shift) mod BF (0 <= kv_shift < BF) ----
__device__ __forceinline__ int kv_batch(int kv_shift) {
    const int bkv = (int)blockIdx.z + kv_shift;
    return bkv >= (int)gridDim.z ? bkv - (int)gridDim.z : bkv;
}

template <int HD>
__global__ __launch_bounds__(64 * WAVES, 1) void attention_wide_kernel(int nq, int nk, const float *__restrict__ q, int qs,
                                                                       const float *__restrict__ k, int ks, const float *__restrict__ v,
                                                                       int vs, float scale_log2e, float *__restrict__ out, int os, int kv_shift) {
    extern __shared__ __attribute__((aligned(16))) float lds_w[];
    attention_wide_body<HD, false>(lds_w, nq, nk, (int)gridDim.y, q, qs, k, ks, v, vs, kv_batch(kv_shift), scale_log2e, 0, 0, 0.f, out, os, nullptr);
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
int launch_wide_ksplit(int bf, int nq, int nk, int heads, const float *q, int qs, const float *k, int ks, const float *v, int vs, float sl2,
                       float *out, int os, int kv_shift, hipStream_t s) {
    auto kern = attention_wide_ksplit_kernel<HD>;
    static McpPerDeviceOnce attr_once;
    if (attr_once.need()) {
        { const hipError_t attr_e_ = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); if (attr_e_ != hipSuccess) return (int)attr_e_; }
        attr_once.done();
    }
    hipLaunchKernelGGL(kern, dim3(mcp_divup(nq, 32), heads, bf), dim3(64 * WAVES), WideSplitCfg<HD>::LDS_BYTES, s, nq, nk, q, qs, k, ks, v, vs, sl2,
                       out, os, kv_shift);
    return mcp_launch_status();
}

template <int HD>
int launch_wide(int bf, int nq, int nk, int heads, const float *q, int qs, const float *k, int ks, const float *v, int vs, float sl2,
                float *out, int os, int kv_shift, hipStream_t s) {
    auto kern = attention_wide_kernel<HD>;
    static McpPerDeviceOnce attr_once;
    if (attr_once.need()) {
        { const hipError_t attr_e_ = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); if (attr_e_ != hipSuccess) return (int)attr_e_; }
        attr_once.done();
    }
    hipLaunchKernelGGL(kern, dim3(mcp_divup(nq, 32 * WAVES), heads, bf), dim3(64 * WAVES), WideCfg<HD>::LDS_BYTES, s, nq, nk, q, qs, k, ks, v,
                       vs, sl2, out, os, kv_shift);
    return mcp_launch_status();
}

}  // namespace

namespace {
int attention_any(int bf, int nq, int nk, int heads, int hd, const float *q, int q_stride, const float *k, int k_stride, const float *v,
                  int v_stride, int kv_shift, float scale, float *out, int out_stride, hipStream_t s) {
    // float4 accesses: every row start and head offset must be 16-byte aligned
    if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out) & 15) return MCP_ERR_BAD_ARG;
    if ((q_stride | k_stride | v_stride | out_stride) & 3) return MCP_ERR_BAD_ARG;
    if (kv_shift < 0 || kv_shift >= bf) return MCP_ERR_BAD_ARG;
    const float sl2 = scale * 1.44269504088896340736f;
    const dim3 grid(mcp_divup(nq, 32 * WAVES), heads, bf);
    int rc;
    mcp_prof_begin(MCP_KERNEL_ATTENTION, s);
    if (hd == 8 || hd == 16) {
        if (hd == 8)
            hipLaunchKernelGGL(attention_small_kernel<8>, grid, dim3(64 * WAVES), 0, s, nq, nk, heads, q, q_stride, k, k_stride, v, v_stride, sl2,
                               out, out_stride, kv_shift);
        else
            hipLaunchKernelGGL(attention_small_kernel<16>, grid, dim3(64 * WAVES), 0, s, nq, nk, heads, q, q_stride, k, k_stride, v, v_stride,
                               sl2, out, out_stride, kv_shift);
        rc = mcp_launch_status();
    } else {
        rc = hd == 32   ? launch_wide<32>(bf, nq, nk, heads, q, q_stride, k, k_stride, v, v_stride, sl2, out, out_stride, kv_shift, s)
             : hd == 64 ? launch_wide<64>(bf, nq, nk, heads, q, q_stride, k, k_stride, v, v_stride, sl2, out, out_stride, kv_shift, s)
                        : wide_keys_split(bf, nq, nk, heads)
                              ? launch_wide_ksplit<256>(bf, nq, nk, heads, q, q_stride, k, k_stride, v, v_stride, sl2, out, out_stride, kv_shift, s)
                              : launch_wide<256>(bf, nq, nk, heads, q, q_stride, k, k_stride, v, v_stride, sl2, out, out_stride, kv_shift, s);
    }
    mcp_prof_end(MCP_KERNEL_ATTENTION, s);
    return rc;
}
}  // namespace

MCP_EXPORT int mcp_attention_small(int bf, int nq, int nk, int heads, int hd, const float *q, int q_stride, const float *k,
                                   int k_stride, const float *v, int v_stride, float scale, float *out, int out_stride,
                                   mcp_stream_t stream) {
    MCP_CHECK_ARGS(bf > 0 && nq > 0 && nk > 0 && heads > 0 && q && k && v && out);
    if (hd != 8 && hd != 16) return MCP_ERR_UNSUPPORTED;
    return attention_any(bf, nq, nk, heads, hd, q, q_stride, k, k_stride, v, v_stride, 0, scale, out, out_stride, (hipStream_t)stream);
}

MCP_EXPORT int mcp_attention_wide(int bf, int nq, int nk, int heads, int hd, const float *q, int q_stride, const float *k,
                                  int k_stride, const float *v, int v_stride, float scale, float *out, int out_stride,
                                  mcp_stream_t stream) {
    MCP_CHECK_ARGS(bf > 0 && nq > 0 && nk > 0 && heads > 0 && q && k && v && out);
    if (hd != 32 && hd != 64 && hd != 256) return MCP_ERR_UNSUPPORTED;
    return attention_any(bf, nq, nk, heads, hd, q, q_stride, k, k_stride, v, v_stride, 0, scale, out, out_stride, (hipStream_t)stream);
}

MCP_EXPORT int mcp_attention(int bf, int nq, int nk, int heads, int hd, const float *q, int q_stride, const float *k, int k_stride,
                             const float *v, int v_stride, int kv_batch_shift, float scale, float *out, int out_stride,
                             mcp_stream_t stream) {
    MCP_CHECK_ARGS(bf > 0 && nq > 0 && nk > 0 && heads > 0 && q && k && v && out);
    if (hd != 8 && hd != 16 && hd != 32 && hd != 64 && hd != 256) return MCP_ERR_UNSUPPORTED;
    return attention_any(bf, nq, nk, heads, hd, q, q_stride, k, k_stride, v, v_stride, kv_batch_shift, scale, out, out_stride,
                         (hipStream_t)stream);
}
