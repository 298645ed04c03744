// emd.hip -- approximate Earth Mover's Distance (metric of test.py:90) for gfx950.
//
// Reference: models/EMD/cuda/emd_kernel.cu:29-162 (approxmatch: 10-level soft auction, level = -4^j for
// j = 7..-1 then 0) and :204-247 (matchcost).  The reference launches <<<32,512>>> with a grid-stride over
// the batch, i.e. ONE workgroup does all 30*n*m exponentials of a batch element, and it materialises
// match (B,m,n) -- 256 MiB per element at 8192 points, read-modify-written once per level.
// Here every pass of every level is a chip-wide launch (lane = one point of one set, the other set
// streamed through LDS tiles of (x,y,z,weight)), and because the cost  sum match*d^2  is linear in the
// per-level transfers w it is accumulated where w is produced: match is written only if the caller asks
// for it (the reference's approxmatch_forward API).  Per-lane summation order over the streamed set is the
// reference's (ascending index), so the iteration reproduces the reference up to __expf's rounding.
//
// Every kernel is stated once with a compile-time LEN (emd_lengths.h).  LEN == false is the plain metric: len1 / len2 are
// never touched.  LEN == true (mcp_emd_lengths / mcp_emd_keep_lengths) runs element b of a padded batch on its prefixes
// xyz1[b, :len1[b]], xyz2[b, :len2[b]] with the padded strides, bit for bit as the plain kernels on copies of the prefixes:
// the mass ratio multiL / multiR is derived per element in emd_init_kernel, every streamed loop stops at the length, and a
// workgroup whose rows are all padding returns before any load or barrier.
#include "common.h"
#include "emd_lengths.h"

namespace {

constexpr int BLK = 256, TILE = 1024;

struct EmdWs {
    float *remainL, *remainR, *ratioL, *ratioR, *costk;
};
__device__ __forceinline__ EmdWs ws_of(float *ws, int b, int n, int m) {
    float *base = ws + (size_t)b * (3 * (size_t)n + 2 * (size_t)m);
    return EmdWs{base, base + n, base + n + m, base + 2 * (size_t)n + m, base + 2 * (size_t)n + 2 * (size_t)m};
}
__device__ __forceinline__ float d2(float x1, float y1, float z1, float x2, float y2, float z2) {
    return mcp_sqdist3(x2, y2, z2, x1, y1, z1);  // (x2-x1)^2 + (y2-y1)^2 + (z2-z1)^2, shared canon
}

// LEN: multiL / multiR are the integer division of emd_kernel.cu:32-38 on the element's own counts (the arguments are unused)
template <bool LEN>
__global__ __launch_bounds__(BLK) void emd_init_kernel(int n, int m, float multiL, float multiR, float *__restrict__ ws,
                                                       const int *__restrict__ len1, const int *__restrict__ len2) {
    int nl, ml;
    emd_counts<LEN>(len1, len2, blockIdx.y, n, m, nl, ml);
    if (LEN) {
        if (nl == 0) return;  // an empty side: no pass touches this element's workspace
        if (nl >= ml) { multiL = 1.f; multiR = (float)(nl / ml); } else { multiL = (float)(ml / nl); multiR = 1.f; }
    }
    const EmdWs w = ws_of(ws, blockIdx.y, n, m);
    const int i = blockIdx.x * BLK + threadIdx.x;
    if (i < nl) { w.remainL[i] = multiL; w.costk[i] = 0.f; }
    if (i < ml) w.remainR[i] = multiR;
}

// PASS 1: ratioL[k] = remainL[k] / (1e-9 + sum_l exp(level*d) * remainR[l])             emd_kernel.cu:56-84
// PASS 3: w = exp(level*d)*ratioL[k]*ratioR[l]; match[l][k] += w; remainL[k] -= sum w    emd_kernel.cu:120-151
//         (+ cost_k += w*d, the fused matchcost)
template <int PASS, bool LEN>
__global__ __launch_bounds__(BLK) void emd_left_kernel(float level, int n, int m, const float *__restrict__ xyz1,
                                                       const float *__restrict__ xyz2, float *__restrict__ ws,
                                                       float *__restrict__ match, const int *__restrict__ len1,
                                                       const int *__restrict__ len2) {
    __shared__ float4 tile[TILE];
    const int b = blockIdx.y;
    int nl, ml;
    emd_counts<LEN>(len1, len2, b, n, m, nl, ml);
    if (LEN && (int)blockIdx.x * BLK >= nl) return;  // workgroup-uniform: nothing but padding here (row 0 is live below)
    const EmdWs w = ws_of(ws, b, n, m);
    const int k = blockIdx.x * BLK + threadIdx.x;
    const bool live = k < nl;
    const float *p1 = xyz1 + ((size_t)b * n + (live ? k : 0)) * 3;
    const float x1 = p1[0], y1 = p1[1], z1 = p1[2];
    const float *p2 = xyz2 + (size_t)b * m * 3;
    const float *wsrc = PASS == 1 ? w.remainR : w.ratioR;
    const float rl = (PASS == 3 && live) ? w.ratioL[k] : 0.f;
    float suml = PASS == 1 ? 1e-9f : 0.f, cost = 0.f;
    float *mrow = match ? match + (size_t)b * n * m + k : nullptr;
    for (int l0 = 0; l0 < ml; l0 += TILE) {
        const int lend = min(ml, l0 + TILE) - l0;
        __syncthreads();
        for (int l = threadIdx.x; l < lend; l += BLK)
            tile[l] = make_float4(p2[(size_t)(l0 + l) * 3], p2[(size_t)(l0 + l) * 3 + 1], p2[(size_t)(l0 + l) * 3 + 2], wsrc[l0 + l]);
        __syncthreads();
        if (live) {
            for (int l = 0; l < lend; ++l) {
                const float4 t = tile[l];
                const float d = d2(x1, y1, z1, t.x, t.y, t.z);
                if (PASS == 1) {
                    suml += __expf(level * d) * t.w;
                } else {
                    const float ww = __expf(level * d) * rl * t.w;
                    if (mrow) mrow[(size_t)(l0 + l) * n] += ww;
                    suml += ww;
                    cost += ww * d;
                }
            }
        }
    }
    if (live) {
        if (PASS == 1) {
            w.ratioL[k] = w.remainL[k] / suml;
        } else {
            w.remainL[k] = fmaxf(0.0f, w.remainL[k] - suml);
            w.costk[k] += cost;
        }
    }
}

// PASS 2: sumr = remainR[l] * sum_k exp(level*d)*ratioL[k]; ratioR, remainR update           emd_kernel.cu:86-118
template <bool LEN>
__global__ __launch_bounds__(BLK) void emd_right_kernel(float level, int n, int m, const float *__restrict__ xyz1,
                                                        const float *__restrict__ xyz2, float *__restrict__ ws,
                                                        const int *__restrict__ len1, const int *__restrict__ len2) {
    __shared__ float4 tile[TILE];
    const int b = blockIdx.y;
    int nl, ml;
    emd_counts<LEN>(len1, len2, b, n, m, nl, ml);
    if (LEN && (int)blockIdx.x * BLK >= ml) return;  // workgroup-uniform: nothing but padding here
    const EmdWs w = ws_of(ws, b, n, m);
    const int l = blockIdx.x * BLK + threadIdx.x;
    const bool live = l < ml;
    const float *p2 = xyz2 + ((size_t)b * m + (live ? l : 0)) * 3;
    const float x2 = p2[0], y2 = p2[1], z2 = p2[2];
    const float *p1 = xyz1 + (size_t)b * n * 3;
    float sumr = 0.f;
    for (int k0 = 0; k0 < nl; k0 += TILE) {
        const int kend = min(nl, k0 + TILE) - k0;
        __syncthreads();
        for (int k = threadIdx.x; k < kend; k += BLK)
            tile[k] = make_float4(p1[(size_t)(k0 + k) * 3], p1[(size_t)(k0 + k) * 3 + 1], p1[(size_t)(k0 + k) * 3 + 2], w.ratioL[k0 + k]);
        __syncthreads();
        if (live) {
            for (int k = 0; k < kend; ++k) {
                const float4 t = tile[k];
                sumr += __expf(level * d2(t.x, t.y, t.z, x2, y2, z2)) * t.w;
            }
        }
    }
    if (live) {
        const float rr = w.remainR[l];
        sumr *= rr;
        const float consumption = fminf(rr / (sumr + 1e-9f), 1.0f);
        w.ratioR[l] = consumption * rr;
        w.remainR[l] = fmaxf(0.0f, rr - sumr);
    }
}

// cost[b] = sum_k costk[b][k]   (fixed-shape tree: deterministic; the strided loop and the tree depend only on the count)
template <bool LEN>
__global__ __launch_bounds__(BLK) void emd_reduce_kernel(int n, int m, const float *__restrict__ ws_c, float *__restrict__ cost,
                                                         const int *__restrict__ len1, const int *__restrict__ len2) {
    __shared__ float part[BLK];
    float *ws = const_cast<float *>(ws_c);
    int nl, ml;
    emd_counts<LEN>(len1, len2, blockIdx.x, n, m, nl, ml);
    const EmdWs w = ws_of(ws, blockIdx.x, n, m);
    float s = 0.f;
    for (int k = threadIdx.x; k < nl; k += BLK) s += w.costk[k];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int h = BLK / 2; h > 0; h >>= 1) {
        if (threadIdx.x < h) part[threadIdx.x] += part[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) cost[blockIdx.x] = part[0];
}

// levels[b][j] = ratioL_j (n floats) | ratioR_j (m floats): the level's two ratios, as pass 3 of level j read them
// (LEN: only the live entries; the padded ones stay unwritten and mcp_emd_grad_lengths never reads them)
template <bool LEN>
__global__ __launch_bounds__(BLK) void emd_keep_kernel(int j, int n, int m, const float *__restrict__ ws_c, float *__restrict__ levels,
                                                       const int *__restrict__ len1, const int *__restrict__ len2) {
    int nl, ml;
    emd_counts<LEN>(len1, len2, blockIdx.y, n, m, nl, ml);
    const EmdWs w = ws_of(const_cast<float *>(ws_c), blockIdx.y, n, m);
    float *dst = levels + ((size_t)blockIdx.y * MCP_EMD_LEVELS + j) * ((size_t)n + m);
    const int i = blockIdx.x * BLK + threadIdx.x;
    if (i < nl) dst[i] = w.ratioL[i];
    if (i < ml) dst[n + i] = w.ratioR[i];
}

// the level loop of mcp_emd; levels != NULL also keeps each level's ratios (one copy launch per level, after pass 3).
// LEN: the same launches over the padded n / m (the host reads no length), the kernels bound themselves.
template <bool LEN>
int emd_run(int b, int n, int m, const float *xyz1, const float *xyz2, const int *len1, const int *len2, float *match, float *cost,
            float *workspace, float *levels, hipStream_t s) {
    float multiL, multiR;  // emd_kernel.cu:32-38 (integer division)
    if (n >= m) { multiL = 1.f; multiR = (float)(n / m); } else { multiL = (float)(m / n); multiR = 1.f; }
    if (match) {
        hipError_t e = hipMemsetAsync(match, 0, sizeof(float) * (size_t)b * n * m, s);
        if (e != hipSuccess) return (int)e;
    }
    const int big = n > m ? n : m;
    hipLaunchKernelGGL(emd_init_kernel<LEN>, dim3(mcp_divup(big, BLK), b), dim3(BLK), 0, s, n, m, multiL, multiR, workspace, len1, len2);
    for (int j = 7; j >= -2; --j) {
        float level = -powf(4.0f, (float)j);
        if (j == -2) level = 0.f;
        hipLaunchKernelGGL((emd_left_kernel<1, LEN>), dim3(mcp_divup(n, BLK), b), dim3(BLK), 0, s, level, n, m, xyz1, xyz2, workspace,
                           (float *)nullptr, len1, len2);
        hipLaunchKernelGGL(emd_right_kernel<LEN>, dim3(mcp_divup(m, BLK), b), dim3(BLK), 0, s, level, n, m, xyz1, xyz2, workspace, len1,
                           len2);
        hipLaunchKernelGGL((emd_left_kernel<3, LEN>), dim3(mcp_divup(n, BLK), b), dim3(BLK), 0, s, level, n, m, xyz1, xyz2, workspace,
                           match, len1, len2);
        if (levels)
            hipLaunchKernelGGL(emd_keep_kernel<LEN>, dim3(mcp_divup(big, BLK), b), dim3(BLK), 0, s, 7 - j, n, m, workspace, levels, len1,
                               len2);
    }
    hipLaunchKernelGGL(emd_reduce_kernel<LEN>, dim3(b), dim3(BLK), 0, s, n, m, workspace, cost, len1, len2);
    return mcp_launch_status();
}

}  // namespace

MCP_EXPORT int mcp_emd(int b, int n, int m, const float *xyz1, const float *xyz2, float *match, float *cost, float *workspace,
                       mcp_stream_t stream) {
    MCP_CHECK_ARGS(b > 0 && n > 0 && m > 0 && xyz1 && xyz2 && cost && workspace);
    return emd_run<false>(b, n, m, xyz1, xyz2, nullptr, nullptr, match, cost, workspace, nullptr, (hipStream_t)stream);
}

MCP_EXPORT size_t mcp_emd_levels_floats(int b, int n, int m) {
    if (b <= 0 || n <= 0 || m <= 0) return 0;
    return (size_t)b * MCP_EMD_LEVELS * ((size_t)n + m);
}

MCP_EXPORT int mcp_emd_keep(int b, int n, int m, const float *xyz1, const float *xyz2, float *cost, float *levels, float *workspace,
                            mcp_stream_t stream) {
    MCP_CHECK_ARGS(b > 0 && n > 0 && m > 0 && xyz1 && xyz2 && cost && levels && workspace);
    return emd_run<false>(b, n, m, xyz1, xyz2, nullptr, nullptr, nullptr, cost, workspace, levels, (hipStream_t)stream);
}

MCP_EXPORT int mcp_emd_lengths(int b, int n, int m, const float *xyz1, const float *xyz2, const int *len1, const int *len2, float *match,
                               float *cost, float *workspace, mcp_stream_t stream) {
    MCP_CHECK_ARGS(b > 0 && n > 0 && m > 0 && xyz1 && xyz2 && cost && workspace);
    if (!len1 && !len2) return emd_run<false>(b, n, m, xyz1, xyz2, nullptr, nullptr, match, cost, workspace, nullptr, (hipStream_t)stream);
    return emd_run<true>(b, n, m, xyz1, xyz2, len1, len2, match, cost, workspace, nullptr, (hipStream_t)stream);
}

MCP_EXPORT int mcp_emd_keep_lengths(int b, int n, int m, const float *xyz1, const float *xyz2, const int *len1, const int *len2,
                                    float *cost, float *levels, float *workspace, mcp_stream_t stream) {
    MCP_CHECK_ARGS(b > 0 && n > 0 && m > 0 && xyz1 && xyz2 && cost && levels && workspace);
    if (!len1 && !len2) return emd_run<false>(b, n, m, xyz1, xyz2, nullptr, nullptr, nullptr, cost, workspace, levels, (hipStream_t)stream);
    return emd_run<true>(b, n, m, xyz1, xyz2, len1, len2, nullptr, cost, workspace, levels, (hipStream_t)stream);
}
