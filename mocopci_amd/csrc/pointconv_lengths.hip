// pointconv_lengths.hip -- PointConv / PointConvD after the sampling on a padded batch whose elements have their own number of
// centres: centre i of element bb is live iff i < qlen[bb] (clamped to [0, s] in the kernel; the host never reads a length).  No kernel
// text and no dispatch live here: the forward kernels are pointconv_tile.h's with one PcLengths behind their parameters, launched by
// that header's pc_agg_run / pc_linear_run; the backward kernel is pointconv_grad_tile.h's under PCG_LEN 1 (there: what a padded
// centre costs and what is written for it), launched by its pcg_run.  Those are the functions the dense units call, deciding from the
// PADDED shape, so a call with every length s gives the dense call's bits.  qlen == NULL is the dense entry point itself.
#define PCG_LEN 1
#include "pointconv_tile.h"
#include "pointconv_grad_tile.h"

// mcp_pointconv_agg with per-element centre lengths (include/mocopci_hip.h)
MCP_EXPORT int mcp_pointconv_agg_lengths(int b, int n, int s, int d, int k, const float *s_xyz, const float *new_xyz, const float *s_points,
                                         const int *idx, const int *qlen, const float *w0, const float *b0, const float *w1, const float *b1,
                                         const float *w2, const float *b2, float *out, mcp_stream_t stream) {
    if (!qlen) return mcp_pointconv_agg(b, n, s, d, k, s_xyz, new_xyz, s_points, idx, w0, b0, w1, b1, w2, b2, out, stream);
    return pc_agg_run(b, n, s, d, k, s_xyz, new_xyz, s_points, idx, w0, b0, w1, b1, w2, b2, out, (hipStream_t)stream, PcLengths{qlen});
}

// mcp_pointconv_linear with per-element centre lengths: a padded centre's row is zero, not leaky(bias)
MCP_EXPORT int mcp_pointconv_linear_lengths(int b, int n, int s, int d, int k, const float *s_xyz, const float *new_xyz, const float *s_points,
                                            const int *idx, const int *qlen, const float *w0, const float *b0, const float *w1, const float *b1,
                                            const float *w2, const float *b2, const float *packed, int c_out, float slope, float *out,
                                            mcp_stream_t stream) {
    if (!qlen) return mcp_pointconv_linear(b, n, s, d, k, s_xyz, new_xyz, s_points, idx, w0, b0, w1, b1, w2, b2, packed, c_out, slope, out, stream);
    return pc_linear_run(b, n, s, d, k, s_xyz, new_xyz, s_points, idx, w0, b0, w1, b1, w2, b2, packed, c_out, slope, out, (hipStream_t)stream,
                         PcLengths{qlen});
}

// mcp_pointconv_agg_grad with per-element centre lengths (workspace: mcp_pointconv_agg_grad_workspace_bytes, as for the dense call)
MCP_EXPORT int mcp_pointconv_agg_grad_lengths(int b, int n, int s, int d, int k, const float *s_xyz, const float *new_xyz, const float *s_points,
                                              const int *idx, const int *qlen, const float *w0, const float *b0, const float *w1, const float *b1,
                                              const float *w2, const float *b2, const float *grad_out, float *grad_new_xyz, float *grad_gxyz,
                                              float *grad_rows, float *grad_weights, void *workspace, size_t workspace_bytes, mcp_stream_t stream) {
    if (!qlen)
        return mcp_pointconv_agg_grad(b, n, s, d, k, s_xyz, new_xyz, s_points, idx, w0, b0, w1, b1, w2, b2, grad_out, grad_new_xyz, grad_gxyz, grad_rows,
                                      grad_weights, workspace, workspace_bytes, stream);
    return pcg_run(b, n, s, d, k, s_xyz, new_xyz, s_points, idx, w0, b0, w1, b1, w2, b2, grad_out, grad_new_xyz, grad_gxyz, grad_rows, grad_weights, workspace,
                   workspace_bytes, (hipStream_t)stream, qlen);
}
