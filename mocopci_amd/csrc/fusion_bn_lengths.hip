// fusion_bn_lengths.hip -- the train-mode fusion layer (fusion_bn.hip) on a padded batch of clouds of different sizes: point p of
// element bb is live iff p < len[bb], and every statistic, every mean term of the backward and every weight / affine gradient runs
// over the m = 64 * (live points) rows of live points only.  The passes are fusion_bn_pass.h's with one FbnLengths behind their
// parameters (there: what a padded point costs and what is written for it); the grids, the deal of points to workgroups and the order
// of every sum are the dense unit's, so a call with every length n gives the dense call's bits.  Nothing here reads a length on the
// host, allocates or uses an atomic.  Both pairs of the dense unit have their form here: the one whose backward re-evaluates the layer
// in its first pass, and the one whose forward keeps every live neighbour's score for it (the *_save_lengths / *_saved_lengths entries).
#define FBN_LEN 1
#include "fusion_bn_pass.h"

namespace {

__global__ void fusion_bn_len_count_kernel(int *__restrict__ count, int value) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *count = value;
}

}  // namespace

// mcp_fusion_bn_forward with per-cloud lengths (include/mocopci_hip.h).  len == NULL: the dense entry point; count then receives b * n.
MCP_EXPORT int mcp_fusion_bn_forward_lengths(int b, int n, int nb, const float *p1, const float *p2, const int *idx, const int *idx2, const int *len,
                                             const float *w1, const float *b1, const float *w2, const float *b2, const float *w3, const float *b3, float eps,
                                             float *bn, float *var, float *out, int *count, void *workspace, size_t workspace_bytes, mcp_stream_t stream) {
    if (!len) {
        const int rc = mcp_fusion_bn_forward(b, n, nb, p1, p2, idx, idx2, w1, b1, w2, b2, w3, b3, eps, bn, var, out, workspace, workspace_bytes, stream);
        if (rc != MCP_OK || !count) return rc;
        const long long total = (long long)b * n;
        hipLaunchKernelGGL(fusion_bn_len_count_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, count, (int)(total > 0x7FFFFFFFLL ? 0x7FFFFFFFLL : total));
        return mcp_launch_status();
    }
    return bn_forward(b, n, nb, p1, p2, idx, idx2, w1, b1, w2, b2, w3, b3, eps, bn, var, out, nullptr, nullptr, nullptr, count, workspace,
                      workspace_bytes, stream, FbnLengths{len, b});
}

// mcp_fusion_bn_forward_save with per-cloud lengths: mcp_fusion_bn_forward_lengths that also keeps every LIVE point's scores (a padded
// point's rows of save_c / save_z / save_s are not written).  len == NULL: the dense entry point; count then receives b * n.
MCP_EXPORT int mcp_fusion_bn_forward_save_lengths(int b, int n, int nb, const float *p1, const float *p2, const int *idx, const int *idx2, const int *len,
                                                  const float *w1, const float *b1, const float *w2, const float *b2, const float *w3, const float *b3,
                                                  float eps, float *bn, float *var, float *out, int *count, int *save_c, float *save_z, float *save_s,
                                                  void *workspace, size_t workspace_bytes, mcp_stream_t stream) {
    MCP_CHECK_ARGS(save_c && save_z && save_s);
    if (!len) {
        const int rc = mcp_fusion_bn_forward_save(b, n, nb, p1, p2, idx, idx2, w1, b1, w2, b2, w3, b3, eps, bn, var, out, save_c, save_z, save_s, workspace,
                                                  workspace_bytes, stream);
        if (rc != MCP_OK || !count) return rc;
        const long long total = (long long)b * n;
        hipLaunchKernelGGL(fusion_bn_len_count_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, count, (int)(total > 0x7FFFFFFFLL ? 0x7FFFFFFFLL : total));
        return mcp_launch_status();
    }
    return bn_forward(b, n, nb, p1, p2, idx, idx2, w1, b1, w2, b2, w3, b3, eps, bn, var, out, save_c, save_z, save_s, count, workspace, workspace_bytes,
                      stream, FbnLengths{len, b});
}

// mcp_fusion_bn_backward_saved with per-cloud lengths: the first pass reads what mcp_fusion_bn_forward_save_lengths kept, of live points only.
MCP_EXPORT int mcp_fusion_bn_backward_saved_lengths(int b, int n, int nb, const float *p1, const float *p2, const int *idx, const int *idx2, const int *len,
                                                    const float *w1, const float *b1, const float *w2, const float *b2, const float *w3, const float *b3,
                                                    const float *bn, const float *grad_out, const int *save_c, const float *save_z, const float *save_s,
                                                    int *row_c, float *row_dy, float *row_a, float *dy2, float *dy1, float *grad_p1, float *grad_nb,
                                                    float *grad_weights, float *grad_affine, void *workspace, size_t workspace_bytes, mcp_stream_t stream) {
    MCP_CHECK_ARGS(save_c && save_z && save_s);
    if (!len)
        return mcp_fusion_bn_backward_saved(b, n, nb, p1, p2, idx, idx2, w1, b1, w2, b2, w3, b3, bn, grad_out, save_c, save_z, save_s, row_c, row_dy, row_a,
                                            dy2, dy1, grad_p1, grad_nb, grad_weights, grad_affine, workspace, workspace_bytes, stream);
    return bn_backward(b, n, nb, p1, p2, idx, idx2, w1, b1, w2, b2, w3, b3, bn, grad_out, save_c, save_z, save_s, row_c, row_dy, row_a, dy2, dy1, grad_p1,
                       grad_nb, grad_weights, grad_affine, workspace, workspace_bytes, stream, FbnLengths{len, b});
}

// mcp_fusion_bn_backward with per-cloud lengths (the first pass re-evaluates the layer).
MCP_EXPORT int mcp_fusion_bn_backward_lengths(int b, int n, int nb, const float *p1, const float *p2, const int *idx, const int *idx2, const int *len,
                                              const float *w1, const float *b1, const float *w2, const float *b2, const float *w3, const float *b3,
                                              const float *bn, const float *grad_out, int *row_c, float *row_dy, float *row_a, float *dy2, float *dy1,
                                              float *grad_p1, float *grad_nb, float *grad_weights, float *grad_affine, void *workspace,
                                              size_t workspace_bytes, mcp_stream_t stream) {
    if (!len)
        return mcp_fusion_bn_backward(b, n, nb, p1, p2, idx, idx2, w1, b1, w2, b2, w3, b3, bn, grad_out, row_c, row_dy, row_a, dy2, dy1, grad_p1, grad_nb,
                                      grad_weights, grad_affine, workspace, workspace_bytes, stream);
    return bn_backward(b, n, nb, p1, p2, idx, idx2, w1, b1, w2, b2, w3, b3, bn, grad_out, nullptr, nullptr, nullptr, row_c, row_dy, row_a, dy2,
                       dy1, grad_p1, grad_nb, grad_weights, grad_affine, workspace, workspace_bytes, stream, FbnLengths{len, b});
}
