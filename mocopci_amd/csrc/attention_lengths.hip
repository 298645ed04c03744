// attention_lengths.hip -- mcp_attention_lengths: mcp_attention (head widths 8 / 16 / 32 / 64 / 256, key / value rotation, row strides)
// over a padded batch whose elements have their own query and key lengths (attention_lengths.h).  No kernel body and no dispatch live
// here: attention_forward.h states the host side once for this unit and attention.hip, and called with one AttnLengths it launches the
// length forms of the same kernels (the bodies of attention_wide_fwd.h, attention_small_kernel of attention_small_fwd.h), decided
// from the PADDED sizes as the dense call decides.
#include "attention_forward.h"

MCP_EXPORT int mcp_attention_lengths(int bf, int nq, int nk, int heads, int hd, const float *q, int q_stride, const float *k, int k_stride,
                                     const float *v, int v_stride, int kv_batch_shift, float scale, const int *qlen, const int *klen, float *out,
                                     int out_stride, mcp_stream_t stream) {
    if (!qlen && !klen)
        return mcp_attention(bf, nq, nk, heads, hd, q, q_stride, k, k_stride, v, v_stride, kv_batch_shift, scale, out, out_stride, stream);
    MCP_CHECK_ARGS(bf > 0 && nq > 0 && nk > 0 && heads > 0 && q && k && v && out);
    if (hd != 8 && hd != 16 && hd != 32 && hd != 64 && hd != 256) return MCP_ERR_UNSUPPORTED;
    if (((uintptr_t)qlen | (uintptr_t)klen) & 3) return MCP_ERR_BAD_ARG;   // scalar loads only
    return attention_forward_run(bf, nq, nk, heads, hd, q, q_stride, k, k_stride, v, v_stride, kv_batch_shift, scale, out, out_stride,
                                 (hipStream_t)stream, AttnLengths{qlen, klen});
}
