// fusion_grad.hip -- backward of the fused attentive fusion (mcp_fusion; MultiFrameEstimatier.knn_group + fusion,
// mocopci.py:798-819) for gfx950.  The reference differentiates the layer with autograd over the materialised
// (B,128,N,64) activations; here one wave owns one point at a time, re-evaluates the layer in the forward's MFMA layout and
// back-propagates inside the kernel:
//
//   phase 1  the forward again (both 32-neighbour halves): score s_j = max_c h3_j[c] with its arg-max channel c*_j, softmax a_j,
//            then ds_j = a_j (g.nb_j - sum_k a_k g.nb_k) and dz3_j = [s_j > 0] ds_j -- the only non-zero of dL/dz3_j sits at c*_j;
//   phase 2  per half: layers 1 and 2 again (h1, h2 stay in registers), and
//              dh2_j = dz3_j W3[c*_j,:]           a row gather (W3 rows from L2), no MFMA
//              dh1   = W2^T dz2                   split-bf16 MFMA, the gradient tile chained as B operand like the forward's activations
//              dx0_j = W1^T dz1_j, dr_j, dnb_j    VALU; d_nb (B,N,64,3) leaves for the caller's deterministic segmented scatter
//            and the weight gradients, whose contraction runs over the NEIGHBOUR axis (the MFMA column of every tensor above), so
//            each operand goes through a per-wave LDS tile once, written in accumulator layout and read back with 8 consecutive
//            neighbours per lane:
//              dW3 += OneHot(c*) . (dz3 h2)^T     the one-hot operand is exact in bf16: 3 MFMAs per product instead of 6
//              dW2 += dz2 . h1^T                  6 MFMAs per product (both operands split three ways)
//              dW1, db1, db2, db3                 in-lane sums over the transposed operands (lane = channel)
//   The weight gradients accumulate in registers over all points of a wave (one wave per SIMD: 192 accumulator registers), points
//   are dealt to waves statically, the four waves of a workgroup are added in wave order through LDS, and a second kernel adds the
//   workgroups' partial vectors in workgroup order: every sum has a fixed order, so the gradients repeat bit for bit.
//   Per point 672 bf16 MFMAs (forward: 288) + 16 f32 ones.
//
// The kernel and the host's walk (fgr_run) are stated in fusion_grad_tile.h, which fusion_lengths.hip shares (per-cloud lengths);
// FGR_LEN 0: the kernel without lengths.  Here: the dense entry points.
#define FGR_LEN 0
#include "fusion_grad_tile.h"

MCP_EXPORT int mcp_fusion_grad_floats(void) { return G_FLOATS; }

MCP_EXPORT size_t mcp_fusion_grad_workspace_bytes(int b, int n) {
    if (b <= 0 || n <= 0) return 0;
    return (size_t)grad_grid((long long)b * n) * G_FLOATS * sizeof(float);
}

MCP_EXPORT int mcp_fusion_grad(int b, int n, int nb, const float *p1, const float *p2, const int *idx, const int *idx2, const float *w1,
                               const float *b1, const float *w2, const float *b2, const float *w3, const float *b3, const float *grad_out,
                               float *grad_p1, float *grad_nb, float *grad_weights, void *workspace, size_t workspace_bytes,
                               mcp_stream_t stream) {
    return fgr_run(b, n, nb, p1, p2, idx, idx2, w1, b1, w2, b2, w3, b3, grad_out, grad_p1, grad_nb, grad_weights, workspace, workspace_bytes,
                   (hipStream_t)stream);
}
