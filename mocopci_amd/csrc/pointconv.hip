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
#include "pointconv_tile.h"   // the kernels; with an empty length pack here, pointconv_lengths.hip holds the length forms

MCP_EXPORT int mcp_pointconv_agg(int b, int n, int s, int d, int k, const float *s_xyz, const float *new_xyz, const float *s_points,
                                 const int *idx, const float *w0, const float *b0, const float *w1, const float *b1, const float *w2,
                                 const float *b2, float *out, mcp_stream_t stream) {
    MCP_CHECK_ARGS(b > 0 && n > 0 && s > 0 && d > 0 && s_xyz && new_xyz && s_points && idx && w0 && b0 && w1 && b1 && w2 && b2 && out);
    if (k != K) return MCP_ERR_UNSUPPORTED;
    if (((uintptr_t)out) & 15) return MCP_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    const long long total = (long long)b * s;
    const bool vec4 = !(d & 3) && !(((uintptr_t)s_points) & 15);  // float4 gathers of 4 adjacent channels need both
    mcp_prof_begin(MCP_KERNEL_POINTCONV, st);
    // points per workgroup so that PPB * d / 4 phase-2 items fill the 256 threads: 32 at d = 32, 16 at d = 64, 8 from d = 128 up;
    // one workgroup per PPB points (no persistent loop in practice): the dispatcher balances around whatever else holds CUs
    auto launch = [&](auto kern, int ppb) {
        const unsigned grid = (unsigned)min((total + ppb - 1) / ppb, 1LL << 20);
        hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, st, total, n, s, d, s_xyz, new_xyz, s_points, idx, w0, b0, w1, b1, w2, b2, out);
    };
    if (total <= 16384 || !vec4) {
        const unsigned grid = (unsigned)min((total + LPPB - 1) / LPPB, 1LL << 20);
        if (d >= 256 && total <= 8192)
            hipLaunchKernelGGL(pointconv_agg_lowlevel_kernel<1024>, dim3(grid), dim3(1024), 0, st, total, n, s, d, s_xyz, new_xyz, s_points, idx, w0, b0, w1, b1, w2, b2, out);
        else
            hipLaunchKernelGGL(pointconv_agg_lowlevel_kernel<256>, dim3(grid), dim3(256), 0, st, total, n, s, d, s_xyz, new_xyz, s_points, idx, w0, b0, w1, b1, w2, b2, out);
    } else if (d <= 32) launch(pointconv_agg_kernel<256, 32>, 32);
    else if (d <= 64) launch(pointconv_agg_kernel<256, 16>, 16);
    else launch(pointconv_agg_kernel<256, 8>, 8);
    mcp_prof_end(MCP_KERNEL_POINTCONV, st);
    return mcp_launch_status();
}

// PointConv / PointConvD after the sampling, whole (mocopci.py:1330-1342, :1381-1393): grouping, WeightNet, aggregation,
// Linear((3+D)*8 -> C_out) and LeakyReLU(slope) in one launch.  packed: the mcp_linear_pack image of the Linear (one piece of
// (3+D)*8 columns) with its bias.  (D, C_out) in {(32, 32), (64, 64)}, 32 neighbours; anything else: MCP_ERR_UNSUPPORTED
// (use mcp_pointconv_agg + mcp_linear).  Bit-identical to that pair from 16384 rows up.
MCP_EXPORT int mcp_pointconv_linear(int b, int n, int s, int d, int k, const float *s_xyz, const float *new_xyz, const float *s_points,
                                    const int *idx, const float *w0, const float *b0, const float *w1, const float *b1, const float *w2,
                                    const float *b2, const float *packed, int c_out, float slope, float *out, mcp_stream_t stream) {
    MCP_CHECK_ARGS(b > 0 && n > 0 && s > 0 && d > 0 && s_xyz && new_xyz && s_points && idx && w0 && b0 && w1 && b1 && w2 && b2 && packed && out);
    if (k != K || !((d == 32 && c_out == 32) || (d == 64 && c_out == 64))) return MCP_ERR_UNSUPPORTED;
    if ((((uintptr_t)out) | ((uintptr_t)s_points) | ((uintptr_t)packed)) & 15) return MCP_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    const long long total = (long long)b * s;
    const unsigned grid = (unsigned)min((total + FPPB - 1) / FPPB, 1LL << 20);
    mcp_prof_begin(MCP_KERNEL_POINTCONV, st);
    if (d == 32) {
        auto kern = pointconv_linear_kernel<32, 1>;
        static McpPerDeviceOnce attr_once;
        if (attr_once.need()) {
            { const hipError_t attr_e_ = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); if (attr_e_ != hipSuccess) return (int)attr_e_; }
            attr_once.done();
        }
        constexpr int lds = FusedCfg<32, 1>::LDS_BYTES;
        hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, st, total, n, s, s_xyz, new_xyz, s_points, idx, w0, b0, w1, b1, w2,
                           b2, packed, c_out, slope, out);
    } else {
        auto kern = pointconv_linear_kernel<64, 2>;
        static McpPerDeviceOnce attr_once;
        if (attr_once.need()) {
            { const hipError_t attr_e_ = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); if (attr_e_ != hipSuccess) return (int)attr_e_; }
            attr_once.done();
        }
        constexpr int lds = FusedCfg<64, 2>::LDS_BYTES;
        hipLaunchKernelGGL(kern, dim3(grid), dim3(512), lds, st, total, n, s, s_xyz, new_xyz, s_points, idx, w0, b0, w1, b1, w2,
                           b2, packed, c_out, slope, out);
    }
    mcp_prof_end(MCP_KERNEL_POINTCONV, st);
    return mcp_launch_status();
}
