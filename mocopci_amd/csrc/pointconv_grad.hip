// pointconv_grad.hip -- backward of the fused PointConv grouping + WeightNet + aggregation (mcp_pointconv_agg; mocopci.py:1218-1266
// group / group_query, :1289-1300 WeightNet, :1330-1335 the matmul) for gfx950.  The reference differentiates the layer with autograd
// over the materialised (B,S,32,3+D) grouping and three (B,8,32,S) WeightNet activations.  Here a lane owns one (centre, neighbour)
// pair -- a wave two centres -- and everything of that pair stays in its registers:
//   * the WeightNet 3 -> 8 -> 8 -> 8 again, in the forward's fma order (same ReLU masks);
//   * with A = dL/dout of the centre ((3+D) x 8, staged once per wave in LDS and read as broadcasts):
//       d[dxyz | feat][k][c] = sum_m A[c][m] w[k][m]      -> grad_rows (B,S,32,D), and the coordinate part joins the WeightNet's
//       dw[k][m]             = sum_c [dxyz | feat][k][c] A[c][m]
//     one pass over the gathered feature row serves both (16 fma per channel);
//   * back through the WeightNet to dxyz: grad_gxyz (B,S,32,3) per pair, dL/dnew_xyz = -sum_k per centre;
//   * the 176 WeightNet weight gradients are sums over pairs: per-lane accumulators over the wave's pairs, one butterfly per wave at
//     the end, waves in wave order, workgroups in workgroup order by a second kernel -- fixed orders, bit-reproducible.
// grad_rows / grad_gxyz are scattered into dL/ds_points and dL/ds_xyz by the caller's deterministic segmented reduction.
#define PCG_LEN 0
#include "pointconv_grad_tile.h"   // pointconv_agg_grad_kernel and its host side (pcg_run); pointconv_lengths.hip holds the length form

MCP_EXPORT int mcp_pointconv_agg_grad_floats(void) { return G_FLOATS; }

MCP_EXPORT size_t mcp_pointconv_agg_grad_workspace_bytes(int b, int s) {
    if (b <= 0 || s <= 0) return 0;
    return (size_t)grad_grid((long long)b * s) * G_FLOATS * sizeof(float);
}

MCP_EXPORT int mcp_pointconv_agg_grad(int b, int n, int s, int d, int k, const float *s_xyz, const float *new_xyz, const float *s_points, const int *idx,
                                      const float *w0, const float *b0, const float *w1, const float *b1, const float *w2, const float *b2,
                                      const float *grad_out, float *grad_new_xyz, float *grad_gxyz, float *grad_rows, float *grad_weights,
                                      void *workspace, size_t workspace_bytes, mcp_stream_t stream) {
    return pcg_run(b, n, s, d, k, s_xyz, new_xyz, s_points, idx, w0, b0, w1, b1, w2, b2, grad_out, grad_new_xyz, grad_gxyz, grad_rows, grad_weights, workspace,
                   workspace_bytes, (hipStream_t)stream);
}
