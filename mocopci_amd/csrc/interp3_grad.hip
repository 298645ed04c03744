// interp3_grad.hip -- backward of the inverse-distance weights of UpsampleFlow / PointWarping (mcp_interp3_weights, interp3.hip;
// mocopci.py:1475-1478, :1495-1498) for gfx950:
//     r_j = sparse[idx3_j] - dense,  d_j = max(|r_j|, 1e-10),  inv_j = 1 / d_j,  w_j = inv_j / (inv_0 + inv_1 + inv_2).
// With gw = dL/dw:  dL/dinv_j = (gw_j - sum_i gw_i w_i) / sum_i inv_i = sum_{i != j} w_i (gw_j - gw_i) / sum_i inv_i (the weights sum to 1;
// this form has no cancellation when one neighbour is much nearer than the others and its weight is within rounding of 1),  dL/dd_j = -inv_j^2 dL/dinv_j,  dL/dr_j = dL/dd_j r_j / |r_j|
// where |r_j| >= 1e-10 and 0 where the clamp held (torch's norm + clamp give exactly that: no 1e10 / 1e20 factor is ever formed).
// One thread per dense point recomputes the three distances with the forward's expressions; grad_nb (B,N,3,3) = dL/dr_j leaves for
// the caller's deterministic segmented scatter into dL/dsparse, grad_dense = -(dL/dr_0 + dL/dr_1) - dL/dr_2 in the forward's
// association order.  No atomics, no cross-thread sums: bit-reproducible.
#include "common.h"

namespace {
constexpr int BLK = 256;

__global__ __launch_bounds__(BLK) void interp3_weights_grad_kernel(int n, int s, const float *__restrict__ dense, const float *__restrict__ sparse,
                                                                   const int *__restrict__ idx3, const float *__restrict__ grad_w3,
                                                                   float *__restrict__ grad_dense, float *__restrict__ grad_nb) {
    const int b = blockIdx.y;
    const int p = blockIdx.x * BLK + threadIdx.x;
    if (p >= n) return;
    const size_t at = (size_t)b * n + p;
    const float *x = dense + at * 3;
    const int *id = idx3 + at * 3;
    const float *gw = grad_w3 + at * 3;
    const float x0 = x[0], x1 = x[1], x2 = x[2];
    float r[3][3], nr[3], inv[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float *y = sparse + ((size_t)b * s + id[j]) * 3;
        r[j][0] = y[0] - x0; r[j][1] = y[1] - x1; r[j][2] = y[2] - x2;
        nr[j] = sqrtf((r[j][0] * r[j][0] + r[j][1] * r[j][1]) + r[j][2] * r[j][2]);
        inv[j] = 1.0f / (nr[j] < 1e-10f ? 1e-10f : nr[j]);
    }
    const float nrm = (inv[0] + inv[1]) + inv[2];
    const float w0 = inv[0] / nrm, w1 = inv[1] / nrm, w2 = inv[2] / nrm;
    const float w[3] = {w0, w1, w2};
    float g[3][3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        if (nr[j] < 1e-10f) {  // the clamp held: d_j does not depend on r_j
            g[j][0] = 0.f; g[j][1] = 0.f; g[j][2] = 0.f;
        } else {
            const int a = j == 0 ? 1 : 0, c = j == 2 ? 1 : 2;  // the other two neighbours, in list order
            const float dinv = (w[a] * (gw[j] - gw[a]) + w[c] * (gw[j] - gw[c])) / nrm;
            const float dd = -(inv[j] * inv[j]) * dinv;
            const float f = dd / nr[j];
            g[j][0] = f * r[j][0]; g[j][1] = f * r[j][1]; g[j][2] = f * r[j][2];
        }
    }
    if (grad_nb) {
        float *o = grad_nb + at * 9;
#pragma unroll
        for (int j = 0; j < 3; ++j) { o[3 * j + 0] = g[j][0]; o[3 * j + 1] = g[j][1]; o[3 * j + 2] = g[j][2]; }
    }
    if (grad_dense) {
        float *o = grad_dense + at * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = -((g[0][c] + g[1][c]) + g[2][c]);
    }
}
}  // namespace

MCP_EXPORT int mcp_interp3_weights_grad(int b, int n, int s, const float *dense, const float *sparse, const int *idx3, const float *grad_w3,
                                        float *grad_dense, float *grad_nb, mcp_stream_t stream) {
    MCP_CHECK_ARGS(b > 0 && n > 0 && s > 0 && dense && sparse && idx3 && grad_w3 && (grad_dense || grad_nb));
    hipLaunchKernelGGL(interp3_weights_grad_kernel, dim3(mcp_divup(n, BLK), b), dim3(BLK), 0, (hipStream_t)stream, n, s, dense, sparse, idx3, grad_w3,
                       grad_dense, grad_nb);
    return mcp_launch_status();
}
