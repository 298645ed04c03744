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
// The host side (checks, dispatch, grids) and the wide heads' kernels are in attention_forward.h, shared with attention_lengths.hip.
#include "attention_forward.h"  // attention_forward_run; with no lengths here

MCP_EXPORT int mcp_attention_small(int bf, int nq, int nk, int heads, int hd, const float *q, int q_stride, const float *k,
                                   int k_stride, const float *v, int v_stride, float scale, float *out, int out_stride,
                                   mcp_stream_t stream) {
    MCP_CHECK_ARGS(bf > 0 && nq > 0 && nk > 0 && heads > 0 && q && k && v && out);
    if (hd != 8 && hd != 16) return MCP_ERR_UNSUPPORTED;
    return attention_forward_run(bf, nq, nk, heads, hd, q, q_stride, k, k_stride, v, v_stride, 0, scale, out, out_stride, (hipStream_t)stream);
}

MCP_EXPORT int mcp_attention_wide(int bf, int nq, int nk, int heads, int hd, const float *q, int q_stride, const float *k,
                                  int k_stride, const float *v, int v_stride, float scale, float *out, int out_stride,
                                  mcp_stream_t stream) {
    MCP_CHECK_ARGS(bf > 0 && nq > 0 && nk > 0 && heads > 0 && q && k && v && out);
    if (hd != 32 && hd != 64 && hd != 256) return MCP_ERR_UNSUPPORTED;
    return attention_forward_run(bf, nq, nk, heads, hd, q, q_stride, k, k_stride, v, v_stride, 0, scale, out, out_stride, (hipStream_t)stream);
}

MCP_EXPORT int mcp_attention(int bf, int nq, int nk, int heads, int hd, const float *q, int q_stride, const float *k, int k_stride,
                             const float *v, int v_stride, int kv_batch_shift, float scale, float *out, int out_stride,
                             mcp_stream_t stream) {
    MCP_CHECK_ARGS(bf > 0 && nq > 0 && nk > 0 && heads > 0 && q && k && v && out);
    if (hd != 8 && hd != 16 && hd != 32 && hd != 64 && hd != 256) return MCP_ERR_UNSUPPORTED;
    return attention_forward_run(bf, nq, nk, heads, hd, q, q_stride, k, k_stride, v, v_stride, kv_batch_shift, scale, out, out_stride,
                                 (hipStream_t)stream);
}
