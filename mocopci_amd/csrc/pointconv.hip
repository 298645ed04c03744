// pointconv.hip -- fused grouping + WeightNet + neighbour aggregation of PointConv / PointConvD for gfx950.
//
// Reference (mocopci.py:1218-1266 group/group_query, :1289-1300 WeightNet, :1330-1335 / :1381-1387):
//   idx -> two K5 gathers (+ permute copies) -> cat [dxyz | feats] (B,S,32,3+D) -> WeightNet 3->8->8->8
//   (three Conv2d+ReLU launches on (B,8,32,S)) -> batched matmul (3+D,32)x(32,8) per point -> (B,S,(3+D)*8).
// At level 0 the intermediates are 280 MiB per tensor.  Here one workgroup owns PPB points:
//   phase 1: one thread per (point, neighbour) gathers the neighbour coordinate, forms dxyz and runs
//            the 3->8->8->8 MLP in registers (weights arrive as scalar loads), leaving dxyz and the
//            8 kernel weights in LDS;
//   phase 2: one thread per (point, 4 consecutive channels) walks the 32 neighbours: the gathered feature
//            rows are read as one float4 per lane (coalesced row segments), the 8 weights are LDS
//            broadcasts shared by the four channels, and the (3+D) x 8 aggregate is accumulated as
//            ascending-k fma chains and written as 128 contiguous bytes.
// The following Linear((3+D)*8 -> C_out) + LeakyReLU (mocopci.py:1336-1342) runs in the same kernel for D = 32 / 64
// (pointconv_linear_kernel below: levels 0, 1 and the refinement stage); wider layers write the aggregate and use mcp_linear.
#include "pointconv_tile.h"   // the kernels and their host side (pc_agg_run, pc_linear_run); with an empty length pack here, pointconv_lengths.hip holds the length forms

MCP_EXPORT int mcp_pointconv_agg(int b, int n, int s, int d, int k, const float *s_xyz, const float *new_xyz, const float *s_points,
                                 const int *idx, const float *w0, const float *b0, const float *w1, const float *b1, const float *w2,
                                 const float *b2, float *out, mcp_stream_t stream) {
    return pc_agg_run(b, n, s, d, k, s_xyz, new_xyz, s_points, idx, w0, b0, w1, b1, w2, b2, out, (hipStream_t)stream);
}

// PointConv / PointConvD after the sampling, whole (mocopci.py:1330-1342, :1381-1393): grouping, WeightNet, aggregation,
// Linear((3+D)*8 -> C_out) and LeakyReLU(slope) in one launch.  packed: the mcp_linear_pack image of the Linear (one piece of
// (3+D)*8 columns) with its bias.  (D, C_out) in {(32, 32), (64, 64)}, 32 neighbours; anything else: MCP_ERR_UNSUPPORTED
// (use mcp_pointconv_agg + mcp_linear).  Bit-identical to that pair from 16384 rows up.
MCP_EXPORT int mcp_pointconv_linear(int b, int n, int s, int d, int k, const float *s_xyz, const float *new_xyz, const float *s_points,
                                    const int *idx, const float *w0, const float *b0, const float *w1, const float *b1, const float *w2,
                                    const float *b2, const float *packed, int c_out, float slope, float *out, mcp_stream_t stream) {
    return pc_linear_run(b, n, s, d, k, s_xyz, new_xyz, s_points, idx, w0, b0, w1, b1, w2, b2, packed, c_out, slope, out, (hipStream_t)stream);
}
