// attention_lengths.hip -- mcp_attention_lengths: mcp_attention (head widths 8 / 16 / 32 / 64 / 256, key / value rotation, row strides)
// over a padded batch whose elements have their own query and key lengths (attention_lengths.h).  No kernel body lives here: the wide
// heads run the two bodies of attention_wide_fwd.h, the narrow heads attention_small_kernel of attention_small_fwd.h, each with one
// AttnLengths behind the parameters of mcp_attention's kernels.  The dispatch at width 256 is attention.hip's, from the PADDED sizes
// (the host never reads a length): a short element of a key-split launch leaves waves of its workgroups without a key stage, which
// the merge weighs with 0.
#include "attention_small_fwd.h"  // and through it attention_wide_fwd.h

namespace {

// keys / values of batch element (bf + kv_shift) mod BF (0 <= kv_shift < BF)
__device__ __forceinline__ int kv_batch(int kv_shift) {
    const int bkv = (int)blockIdx.z + kv_shift;
    return bkv >= (int)gridDim.z ? bkv - (int)gridDim.z : bkv;
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
__global__ __launch_bounds__(64 * WAVES, 1) void attention_wide_ksplit_lengths_kernel(int nq, int nk, const float *__restrict__ q, int qs,
                                                                                      const float *__restrict__ k, int ks,
                                                                                      const float *__restrict__ v, int vs, float scale_log2e,
                                                                                      float *__restrict__ out, int os, int kv_shift,
                                                                                      AttnLengths len) {
    extern __shared__ __attribute__((aligned(16))) float lds_ws[];
    attention_wide_ksplit_body<HD, false>(lds_ws, nq, nk, (int)gridDim.y, q, qs, k, ks, v, vs, kv_batch(kv_shift), scale_log2e, 0, 0, 0.f, out, os,
                                          nullptr, len);
}

// dynamic LDS above the 64 KB default: the attribute is set once per device and kernel instantiation
template <auto KERN>
int allow_lds() {
    static McpPerDeviceOnce attr_once;
    if (attr_once.need()) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(KERN), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return (int)e;
        attr_once.done();
    }
    return MCP_OK;
}

template <int HD>
int launch_wide_lengths(int bf, int nq, int nk, int heads, const float *q, int qs, const float *k, int ks, const float *v, int vs, float sl2,
                        float *out, int os, int kv_shift, AttnLengths len, hipStream_t s) {
    if constexpr (HD == 256) {
        if (wide_keys_split(bf, nq, nk, heads)) {
            constexpr auto kern = attention_wide_ksplit_lengths_kernel<HD>;
            if (const int rc = allow_lds<kern>()) return rc;
            hipLaunchKernelGGL(kern, dim3(mcp_divup(nq, 32), heads, bf), dim3(64 * WAVES), WideSplitCfg<HD>::LDS_BYTES, s, nq, nk, q, qs, k, ks, v,
                               vs, sl2, out, os, kv_shift, len);
            return mcp_launch_status();
        }
    }
    constexpr auto kern = attention_wide_lengths_kernel<HD>;
    if (const int rc = allow_lds<kern>()) return rc;
    hipLaunchKernelGGL(kern, dim3(mcp_divup(nq, 32 * WAVES), heads, bf), dim3(64 * WAVES), WideCfg<HD>::LDS_BYTES, s, nq, nk, q, qs, k, ks, v, vs,
                       sl2, out, os, kv_shift, len);
    return mcp_launch_status();
}

}  // namespace

MCP_EXPORT int mcp_attention_lengths(int bf, int nq, int nk, int heads, int hd, const float *q, int q_stride, const float *k, int k_stride,
                                     const float *v, int v_stride, int kv_batch_shift, float scale, const int *qlen, const int *klen, float *out,
                                     int out_stride, mcp_stream_t stream) {
    if (!qlen && !klen)
        return mcp_attention(bf, nq, nk, heads, hd, q, q_stride, k, k_stride, v, v_stride, kv_batch_shift, scale, out, out_stride, stream);
    MCP_CHECK_ARGS(bf > 0 && nq > 0 && nk > 0 && heads > 0 && q && k && v && out);
    if (hd != 8 && hd != 16 && hd != 32 && hd != 64 && hd != 256) return MCP_ERR_UNSUPPORTED;
    if (((uintptr_t)qlen | (uintptr_t)klen) & 3) return MCP_ERR_BAD_ARG;
    // float4 accesses: every row start and head offset must be 16-byte aligned
    if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out) & 15) return MCP_ERR_BAD_ARG;
    if ((q_stride | k_stride | v_stride | out_stride) & 3) return MCP_ERR_BAD_ARG;
    if (kv_batch_shift < 0 || kv_batch_shift >= bf) return MCP_ERR_BAD_ARG;
    hipStream_t s = (hipStream_t)stream;
    const float sl2 = scale * 1.44269504088896340736f;
    const AttnLengths len{qlen, klen};
    mcp_prof_begin(MCP_KERNEL_ATTENTION, s);
    int rc;
    if (hd == 8 || hd == 16) {
        const dim3 grid(mcp_divup(nq, 32 * WAVES), heads, bf);
        if (hd == 8)
            hipLaunchKernelGGL((attention_small_kernel<8, AttnLengths>), grid, dim3(64 * WAVES), 0, s, nq, nk, heads, q, q_stride, k, k_stride, v,
                               v_stride, sl2, out, out_stride, kv_batch_shift, len);
        else
            hipLaunchKernelGGL((attention_small_kernel<16, AttnLengths>), grid, dim3(64 * WAVES), 0, s, nq, nk, heads, q, q_stride, k, k_stride, v,
                               v_stride, sl2, out, out_stride, kv_batch_shift, len);
        rc = mcp_launch_status();
    } else {
#define MCP_ATT_ARGS bf, nq, nk, heads, q, q_stride, k, k_stride, v, v_stride, sl2, out, out_stride, kv_batch_shift, len, s
        rc = hd == 32 ? launch_wide_lengths<32>(MCP_ATT_ARGS) : hd == 64 ? launch_wide_lengths<64>(MCP_ATT_ARGS) : launch_wide_lengths<256>(MCP_ATT_ARGS);
#undef MCP_ATT_ARGS
    }
    mcp_prof_end(MCP_KERNEL_ATTENTION, s);
    return rc;
}
