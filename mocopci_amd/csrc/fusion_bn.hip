// fusion_bn.hip -- the attentive fusion layer in net.train() mode (batch statistics) over every point of the call: the kernels and the
// entry points.  The passes themselves -- what they compute, their layouts and the order of every sum -- are stated once in
// fusion_bn_pass.h, shared with the per-cloud-length form (fusion_bn_lengths.hip); FBN_LEN 0: every kernel is a pass without lengths.
#define FBN_LEN 0
#include "fusion_bn_pass.h"

MCP_EXPORT int mcp_fusion_bn_floats(void) { return BN_FLOATS; }

MCP_EXPORT size_t mcp_fusion_bn_workspace_bytes(int b, int n) {
    if (b <= 0 || n <= 0) return 0;
    return fwd_workspace_floats((long long)b * n) * sizeof(float);
}

// The layer on BATCH statistics, forward.  bn (1024 floats): per layer mean | rstd | gamma | beta, natural channel order, layers
// 4 -> 64 -> 64 -> 128; the caller fills gamma and beta, this call fills mean and rstd (from the b clouds it is given: one
// reference call = one set of statistics) and writes the biased variances to var (64 | 64 | 128 floats) for the running estimates.
MCP_EXPORT int mcp_fusion_bn_forward(int b, int n, int nb, const float *p1, const float *p2, const int *idx, const int *idx2, const float *w1,
                                     const float *b1, const float *w2, const float *b2, const float *w3, const float *b3, float eps, float *bn, float *var,
                                     float *out, void *workspace, size_t workspace_bytes, mcp_stream_t stream) {
    return bn_forward(b, n, nb, p1, p2, idx, idx2, w1, b1, w2, b2, w3, b3, eps, bn, var, out, nullptr, nullptr, nullptr, nullptr, workspace,
                      workspace_bytes, stream);
}

// The same forward that also keeps, per (point, neighbour) row (rows = b * n * 64), the neighbour's score, the layer-3 channel it comes
// from and zhat3 there: save_c (int32), save_z, save_s (floats), caller-owned -- mcp_fusion_bn_backward_saved then skips the
// re-evaluation of the whole layer in its first pass.
MCP_EXPORT int mcp_fusion_bn_forward_save(int b, int n, int nb, const float *p1, const float *p2, const int *idx, const int *idx2, const float *w1,
                                          const float *b1, const float *w2, const float *b2, const float *w3, const float *b3, float eps, float *bn,
                                          float *var, float *out, int *save_c, float *save_z, float *save_s, void *workspace, size_t workspace_bytes,
                                          mcp_stream_t stream) {
    MCP_CHECK_ARGS(save_c && save_z && save_s);
    return bn_forward(b, n, nb, p1, p2, idx, idx2, w1, b1, w2, b2, w3, b3, eps, bn, var, out, save_c, save_z, save_s, nullptr, workspace,
                      workspace_bytes, stream);
}

MCP_EXPORT size_t mcp_fusion_bn_grad_workspace_bytes(int b, int n) {
    if (b <= 0 || n <= 0) return 0;
    return bwd_workspace_floats((long long)b * n) * sizeof(float);
}

// The layer on batch statistics, backward (one reference call; bn as mcp_fusion_bn_forward left it).  grad_out (B,N,3).  Scratch the
// caller provides: row_c (rows int32), row_dy, row_a (rows floats), dy2, dy1 (rows x 64 floats), rows = b * n * 64.  Writes grad_p1
// (B,N,3), grad_nb (B,N,64,3) (for the caller's scatter into dL/dp2), grad_weights (12800 floats, mcp_fusion_grad's layout; the
// conv-bias entries are 0: a bias in front of a batch-statistics BatchNorm has no gradient) and grad_affine (512 floats: per layer
// dgamma | dbeta -- 64 | 64, 64 | 64, 128 | 128).
MCP_EXPORT int mcp_fusion_bn_backward(int b, int n, int nb, const float *p1, const float *p2, const int *idx, const int *idx2, const float *w1,
                                      const float *b1, const float *w2, const float *b2, const float *w3, const float *b3, const float *bn,
                                      const float *grad_out, int *row_c, float *row_dy, float *row_a, float *dy2, float *dy1, float *grad_p1,
                                      float *grad_nb, float *grad_weights, float *grad_affine, void *workspace, size_t workspace_bytes,
                                      mcp_stream_t stream) {
    return bn_backward(b, n, nb, p1, p2, idx, idx2, w1, b1, w2, b2, w3, b3, bn, grad_out, nullptr, nullptr, nullptr, row_c, row_dy, row_a, dy2,
                       dy1, grad_p1, grad_nb, grad_weights, grad_affine, workspace, workspace_bytes, stream);
}

// mcp_fusion_bn_backward with what mcp_fusion_bn_forward_save kept: the first pass reads (score, c*, zhat3) instead of re-evaluating the layer.
MCP_EXPORT int mcp_fusion_bn_backward_saved(int b, int n, int nb, const float *p1, const float *p2, const int *idx, const int *idx2, const float *w1,
                                            const float *b1, const float *w2, const float *b2, const float *w3, const float *b3, const float *bn,
                                            const float *grad_out, const int *save_c, const float *save_z, const float *save_s, int *row_c, float *row_dy,
                                            float *row_a, float *dy2, float *dy1, float *grad_p1, float *grad_nb, float *grad_weights, float *grad_affine,
                                            void *workspace, size_t workspace_bytes, mcp_stream_t stream) {
    MCP_CHECK_ARGS(save_c && save_z && save_s);
    return bn_backward(b, n, nb, p1, p2, idx, idx2, w1, b1, w2, b2, w3, b3, bn, grad_out, save_c, save_z, save_s, row_c, row_dy, row_a, dy2, dy1,
                       grad_p1, grad_nb, grad_weights, grad_affine, workspace, workspace_bytes, stream);
}
