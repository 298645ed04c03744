// pointconv_lengths.hip -- PointConv / PointConvD after the sampling on a padded batch whose elements have their own number of
// centres: centre i of element bb is live iff i < qlen[bb] (clamped to [0, s] in the kernel; the host never reads a length).  No kernel
// text lives here: the forward kernels are pointconv_tile.h's with one PcLengths behind their parameters, the backward kernel is
// pointconv_grad_tile.h's under PCG_LEN 1 (there: what a padded centre costs and what is written for it).  The dispatch, the grids and
// the order of every sum are the dense units', from the PADDED shape, so a call with every length s gives the dense call's bits.
// qlen == NULL is the dense entry point itself.
#define PCG_LEN 1
#include "pointconv_tile.h"
#include "pointconv_grad_tile.h"

// mcp_pointconv_agg with per-element centre lengths (include/mocopci_hip.h)
MCP_EXPORT int mcp_pointconv_agg_lengths(int b, int n, int s, int d, int k, const float *s_xyz, const float *new_xyz, const float *s_points,
                                         const int *idx, const int *qlen, const float *w0, const float *b0, const float *w1, const float *b1,
                                         const float *w2, const float *b2, float *out, mcp_stream_t stream) {
    if (!qlen) return mcp_pointconv_agg(b, n, s, d, k, s_xyz, new_xyz, s_points, idx, w0, b0, w1, b1, w2, b2, out, stream);
    MCP_CHECK_ARGS(b > 0 && n > 0 && s > 0 && d > 0 && s_xyz && new_xyz && s_points && idx && w0 && b0 && w1 && b1 && w2 && b2 && out);
    if (k != K) return MCP_ERR_UNSUPPORTED;
    if ((((uintptr_t)out) & 15) || (((uintptr_t)qlen) & 3)) return MCP_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    const long long total = (long long)b * s;
    const bool vec4 = !(d & 3) && !(((uintptr_t)s_points) & 15);  // float4 gathers of 4 adjacent channels need both
    const PcLengths len{qlen};
    mcp_prof_begin(MCP_KERNEL_POINTCONV, st);
    // mcp_pointconv_agg's dispatch and grids, from the padded shape
    auto launch = [&](auto kern, int ppb) {
        const unsigned grid = (unsigned)min((total + ppb - 1) / ppb, 1LL << 20);
        hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, st, total, n, s, d, s_xyz, new_xyz, s_points, idx, w0, b0, w1, b1, w2, b2, out, len);
    };
    if (total <= 16384 || !vec4) {
        const unsigned grid = (unsigned)min((total + LPPB - 1) / LPPB, 1LL << 20);
        if (d >= 256 && total <= 8192)
            hipLaunchKernelGGL((pointconv_agg_lowlevel_kernel<1024, PcLengths>), dim3(grid), dim3(1024), 0, st, total, n, s, d, s_xyz, new_xyz, s_points, idx, w0, b0, w1, b1, w2, b2, out, len);
        else
            hipLaunchKernelGGL((pointconv_agg_lowlevel_kernel<256, PcLengths>), dim3(grid), dim3(256), 0, st, total, n, s, d, s_xyz, new_xyz, s_points, idx, w0, b0, w1, b1, w2, b2, out, len);
    } else if (d <= 32) launch(pointconv_agg_kernel<256, 32, PcLengths>, 32);
    else if (d <= 64) launch(pointconv_agg_kernel<256, 16, PcLengths>, 16);
    else launch(pointconv_agg_kernel<256, 8, PcLengths>, 8);
    mcp_prof_end(MCP_KERNEL_POINTCONV, st);
    return mcp_launch_status();
}

namespace {

template <int D, int NT>
int launch_linear_lengths(long long total, int n, int s, const float *s_xyz, const float *new_xyz, const float *s_points, const int *idx,
                          const float *w0, const float *b0, const float *w1, const float *b1, const float *w2, const float *b2,
                          const float *packed, int c_out, float slope, float *out, PcLengths len, hipStream_t st) {
    constexpr auto kern = pointconv_linear_kernel<D, NT, PcLengths>;
    static McpPerDeviceOnce attr_once;
    if (attr_once.need()) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return (int)e;
        attr_once.done();
    }
    const unsigned grid = (unsigned)min((total + FPPB - 1) / FPPB, 1LL << 20);
    using C = FusedCfg<D, NT>;
    constexpr int threads = C::THREADS, lds = C::LDS_BYTES;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(threads), lds, st, total, n, s, s_xyz, new_xyz, s_points, idx, w0, b0, w1, b1, w2, b2, packed, c_out,
                       slope, out, len);
    return MCP_OK;
}

}  // namespace

// mcp_pointconv_linear with per-element centre lengths: a padded centre's row is zero, not leaky(bias)
MCP_EXPORT int mcp_pointconv_linear_lengths(int b, int n, int s, int d, int k, const float *s_xyz, const float *new_xyz, const float *s_points,
                                            const int *idx, const int *qlen, const float *w0, const float *b0, const float *w1, const float *b1,
                                            const float *w2, const float *b2, const float *packed, int c_out, float slope, float *out,
                                            mcp_stream_t stream) {
    if (!qlen) return mcp_pointconv_linear(b, n, s, d, k, s_xyz, new_xyz, s_points, idx, w0, b0, w1, b1, w2, b2, packed, c_out, slope, out, stream);
    MCP_CHECK_ARGS(b > 0 && n > 0 && s > 0 && d > 0 && s_xyz && new_xyz && s_points && idx && w0 && b0 && w1 && b1 && w2 && b2 && packed && out);
    if (k != K || !((d == 32 && c_out == 32) || (d == 64 && c_out == 64))) return MCP_ERR_UNSUPPORTED;
    if (((((uintptr_t)out) | ((uintptr_t)s_points) | ((uintptr_t)packed)) & 15) || (((uintptr_t)qlen) & 3)) return MCP_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    const long long total = (long long)b * s;
    const PcLengths len{qlen};
    mcp_prof_begin(MCP_KERNEL_POINTCONV, st);
    const int rc = d == 32 ? launch_linear_lengths<32, 1>(total, n, s, s_xyz, new_xyz, s_points, idx, w0, b0, w1, b1, w2, b2, packed, c_out, slope, out, len, st)
                           : launch_linear_lengths<64, 2>(total, n, s, s_xyz, new_xyz, s_points, idx, w0, b0, w1, b1, w2, b2, packed, c_out, slope, out, len, st);
    if (rc != MCP_OK) return rc;
    mcp_prof_end(MCP_KERNEL_POINTCONV, st);
    return mcp_launch_status();
}

// mcp_pointconv_agg_grad with per-element centre lengths (workspace: mcp_pointconv_agg_grad_workspace_bytes, as for the dense call)
MCP_EXPORT int mcp_pointconv_agg_grad_lengths(int b, int n, int s, int d, int k, const float *s_xyz, const float *new_xyz, const float *s_points,
                                              const int *idx, const int *qlen, const float *w0, const float *b0, const float *w1, const float *b1,
                                              const float *w2, const float *b2, const float *grad_out, float *grad_new_xyz, float *grad_gxyz,
                                              float *grad_rows, float *grad_weights, void *workspace, size_t workspace_bytes, mcp_stream_t stream) {
    if (!qlen)
        return mcp_pointconv_agg_grad(b, n, s, d, k, s_xyz, new_xyz, s_points, idx, w0, b0, w1, b1, w2, b2, grad_out, grad_new_xyz, grad_gxyz, grad_rows,
                                      grad_weights, workspace, workspace_bytes, stream);
    MCP_CHECK_ARGS(b > 0 && n > 0 && s > 0 && s_xyz && new_xyz && s_points && idx && w0 && b0 && w1 && b1 && w2 && b2 && grad_out && grad_new_xyz &&
                   grad_gxyz && grad_rows && grad_weights && workspace);
    if (k != K || d < 4 || (d & 3) || d > MAX_D) return MCP_ERR_UNSUPPORTED;
    if (((((uintptr_t)s_points) | ((uintptr_t)grad_out) | ((uintptr_t)grad_rows)) & 15) || (((uintptr_t)qlen) & 3)) return MCP_ERR_BAD_ARG;
    const long long total = (long long)b * s;
    const unsigned grid = grad_grid(total);
    if (workspace_bytes < (size_t)grid * G_FLOATS * sizeof(float)) return MCP_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    size_t lds = (size_t)WAVES * 2 * (d + 3) * WN * sizeof(float);
    if (lds < (size_t)WAVES * G_FLOATS * sizeof(float)) lds = (size_t)WAVES * G_FLOATS * sizeof(float);
    static McpPerDeviceOnce attr_once;
    if (attr_once.need()) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(pointconv_agg_grad_lengths_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return (int)e;
        attr_once.done();
    }
    mcp_prof_begin(MCP_KERNEL_POINTCONV, st);
    hipLaunchKernelGGL(pointconv_agg_grad_lengths_kernel, dim3(grid), dim3(64 * WAVES), lds, st, total, n, s, d, s_xyz, new_xyz, s_points, idx, w0, b0, w1, b1, w2,
                       b2, grad_out, grad_new_xyz, grad_gxyz, grad_rows, static_cast<float *>(workspace), qlen);
    hipLaunchKernelGGL(pointconv_grad_reduce_kernel, dim3(1), dim3(256), 0, st, static_cast<const float *>(workspace), (int)grid, grad_weights);
    mcp_prof_end(MCP_KERNEL_POINTCONV, st);
    return mcp_launch_status();
}
