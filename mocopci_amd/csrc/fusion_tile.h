// fusion_tile.h -- fusion_split_kernel (fusion.hip), stated once for the dense unit and for fusion_lengths.hip.  The including unit
// sets the compile-time parameter, as pointconv_grad_tile.h and fusion_bn_pass.h have it: FUS_LEN 0 is fusion_split_kernel with its
// parameters as they were, FUS_LEN 1 fusion_split_lengths_kernel with `const int *len` behind them.  The text stays in the kernel (a
// forceinline body under a __global__ wrapper is optimised on its own first and comes out with another schedule); FUS_LEN 0 is the
// dense kernel, instruction for instruction (profiles/fusion_lengths_resources.txt).  FUS_LEN 1: point p of element bb is live iff
// p - bb n < min(max(len[bb], 0), n).  One wave owns one point, so the answer is wave-uniform: the length is a scalar load and a padded
// point is one scalar branch -- none of its row of p1, idx, idx2 is read, nothing is gathered, and its row of out is written as zeros
// (from not computing: the unit is built with -fno-honor-nans, so never from padding times zero).  A live point runs the software
// pipeline below unchanged; the points are dealt to workgroups and waves in padded order on the grid of b * n points.
// The host side that both entry points share (the grid, the launch) is at the end of this file.
#pragma once
#include "fusion_shared.h"
#include "mfma_split.h"

#ifndef FUS_LEN
#error "define FUS_LEN (0 or 1) before including fusion_tile.h"
#endif
#if FUS_LEN
#define FUS_KERNEL fusion_split_lengths_kernel
#define FUS_LENS_PARAM , const int *__restrict__ len
#define FUS_LENS , len
#else
#define FUS_KERNEL fusion_split_kernel
#define FUS_LENS_PARAM
#define FUS_LENS
#endif

namespace {

// ---- split-bf16 build ------------------------------------------------------------------------------------------------------
// LDS image of the split build: w1 / biases (fp32), then per layer [t_out][kstep][piece][lane] x 16 B
constexpr int SP_W1 = 0, SP_B1 = 256, SP_B2 = SP_B1 + 64, SP_B3 = SP_B2 + 64, SP_F32_FLOATS = SP_B3 + 128;  // fp32 part (floats)
constexpr int SP_W2_U4 = 2 * 4 * 3 * 64, SP_W3_U4 = 4 * 4 * 3 * 64;                                         // uint4 counts
constexpr size_t SP_LDS_BYTES = SP_F32_FLOATS * 4 + (size_t)(SP_W2_U4 + SP_W3_U4) * 16;

// running channel max over registers 4q..4q+3 of a tile, in register order (two v_max3_f32).  The empty asm keeps the value where it is
// computed: without it the compiler sinks the whole chain of a point to its one use behind the last MFMA, tiles kept alive until then.
__device__ __forceinline__ float max4(float m, const f32x16 &a, int q) {
#pragma unroll
    for (int i = 0; i < 4; ++i) m = fmaxf(m, a[4 * q + i]);
    asm volatile("" : "+v"(m));
    return m;
}
// TILES output tiles of one split-bf16 layer with 64 input channels: out[t] = bias(t) + sum over k-steps s = 0..3 of W(t, s) . X(s), the
// k-steps ascending.  wl points at this lane's entry of the layer's weight image, bias at this lane half's 16 floats of tile 0 (tiles are
// 32 floats apart).  fill(r) is the filler batch of k-step r = 4 t + s (mcp_kstep_fill), NF0 vector instructions for r < 8 and NF1 from
// there; the weight pieces of k-step r + 1 and the bias of the next tile are read while k-step r runs.
constexpr int NF_SPLIT = 26, NF_MAX = 2;  // mcp_relu_split4, max4
template <int TILES, int NF0, int NF1, class Fill>
__device__ __forceinline__ void split_layer(const uint4 *wl, const float *bias, const McpSplit3 *xs, f32x16 *out, Fill fill) {
    uint4 w1 = wl[0], w2 = wl[64], w3 = wl[128];
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = bias[i];
#pragma unroll
    for (int r = 0; r < 4 * TILES; ++r) {
        uint4 n1 = w1, n2 = w2, n3 = w3;
        f32x16 nacc = acc;
        if (r + 1 < 4 * TILES) {
            const uint4 *nx = wl + (size_t)(r + 1) * 3 * 64;
            n1 = nx[0]; n2 = nx[64]; n3 = nx[128];
            if ((r & 3) == 3) {
#pragma unroll
                for (int i = 0; i < 16; ++i) nacc[i] = bias[32 * ((r >> 2) + 1) + i];
            }
        }
        if (r < 8) acc = mcp_kstep_fill<NF0>(w1, w2, w3, xs[r & 3], acc, [&] { fill(r); });
        else acc = mcp_kstep_fill<NF1>(w1, w2, w3, xs[r & 3], acc, [&] { fill(r); });
        if ((r & 3) == 3) { out[r >> 2] = acc; acc = nacc; }
        w1 = n1; w2 = n2; w3 = n3;
    }
}

__global__ __launch_bounds__(64 * WAVES, 2) void FUS_KERNEL(long long total, int n, const float *__restrict__ p1,
                                                                  const float *__restrict__ p2, const int *__restrict__ idx, const int *__restrict__ idx2,
                                                                  const float *__restrict__ w1, const float *__restrict__ b1,
                                                                  const float *__restrict__ w2, const float *__restrict__ b2,
                                                                  const float *__restrict__ w3, const float *__restrict__ b3,
                                                                  float *__restrict__ out FUS_LENS_PARAM) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    uint4 *w2s = reinterpret_cast<uint4 *>(lds + SP_F32_FLOATS);
    uint4 *w3s = w2s + SP_W2_U4;
    const int tid = threadIdx.x;
    for (int e = tid; e < 256; e += 64 * WAVES) {  // w1 (fp32, K = 4): [t][s][lane] = W1[32t + (lane&31)][2s + (lane>>5)]
        const int lane = e & 63, s = (e >> 6) & 1, t = e >> 7;
        lds[SP_W1 + e] = w1[(32 * t + (lane & 31)) * 4 + 2 * s + (lane >> 5)];
    }
    mcp_split_weights(w2s, w2, C1, 2, tid, 64 * WAVES);
    mcp_split_weights(w3s, w3, C2, 4, tid, 64 * WAVES);
    for (int e = tid; e < 64; e += 64 * WAVES) {  // biases: [t][h][r]
        const int r = e & 15, h = (e >> 4) & 1, t = e >> 5;
        lds[SP_B1 + e] = b1[32 * t + mcp_chan_of(r, h)];
        lds[SP_B2 + e] = b2[32 * t + mcp_chan_of(r, h)];
    }
    for (int e = tid; e < 128; e += 64 * WAVES) {
        const int r = e & 15, h = (e >> 4) & 1, t = e >> 5;
        lds[SP_B3 + e] = b3[32 * t + mcp_chan_of(r, h)];
    }
    __syncthreads();

    const int lane = tid & 63, wave = tid >> 6, h = lane >> 5, col = lane & 31;
    const McpUnits units = mcp_units_by_xcd(total, WAVES);   // XCD x takes the x-th eighth of the points (common.h)
    const uint4 *w2l = w2s + lane, *w3l = w3s + lane;
    for (long long p = units.first + wave; p < units.limit; p += units.stride) {
        const long long bb = mcp_div(p, n, mcp_fits32(total));
#if FUS_LEN
        if (!fusion_live(len, p, bb, n)) {   // a padded point: nothing of it is read, its row of out is zero
            if (lane < 3) out[p * 3 + lane] = 0.f;
            continue;
        }
#endif
        const float cx = p1[p * 3 + 0], cy = p1[p * 3 + 1], cz = p1[p * 3 + 2];
        float score[2], nbx[2], nby[2], nbz[2];
        // The point's two 32-neighbour column tiles are two independent chains, A (ct = 0) and B (ct = 1).  They run as a software
        // pipeline: the ReLU + operand split (and the channel max) of one chain is the filler work under the MFMAs of the other, a
        // quarter tile (26 vector instructions) per six-MFMA k-step, and a quarter tile is first touched at least one whole k-step
        // after the MFMA that finished it.  Every accumulator still starts from its bias and takes its k-steps in ascending order.
        //   layer 1 of A and B | split A1 | A: layer 2 under it split B1 | B: layer 2, split A2 | A: layer 3, split B2 + max A | B: layer 3, max A, B
        f32x16 l1[2][2];
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
            // idx2 != NULL: the two 32-neighbour halves come as separate (B,N,32) lists (no concatenation pass by the caller)
            const int id = idx2 ? (ct ? idx2 : idx)[p * 32 + col] : idx[p * NB + 32 * ct + col];
            const float *q = p2 + ((long long)bb * n + id) * 3;
            const float x = q[0], y = q[1], z = q[2];
            nbx[ct] = x; nby[ct] = y; nbz[ct] = z;
            const float rx = x - cx, ry = y - cy, rz = z - cz;
            const float dist = sqrtf((rx * rx + ry * ry) + rz * rz);
            const float in0 = h ? ry : rx, in1 = h ? dist : rz;
            // ---- layer 1: 4 -> 64 on the f32-input MFMA (K = 4: two k-steps) ----
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                f32x16 acc;
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] = lds[SP_B1 + (t * 2 + h) * 16 + r];
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(lds[SP_W1 + (t * 2 + 0) * 64 + lane], in0, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(lds[SP_W1 + (t * 2 + 1) * 64 + lane], in1, acc, 0, 0, 0);
                l1[ct][t] = acc;
            }
        }
        McpSplit3 xa1[4], xb1[4], xa2[4], xb2[4];
        f32x16 a2[2], b2t[2], a3[4], b3t[4];
        float ma = 0.f, mb = 0.f;
#pragma unroll
        for (int u = 0; u < 8; ++u) mcp_relu_split4(l1[0][u >> 2], u & 3, xa1[u >> 1]);   // nothing to hide under yet
        __builtin_amdgcn_sched_barrier(0);
        // A layer 2 | ReLU + split of B's layer 1
        split_layer<2, NF_SPLIT, 0>(w2l, lds + SP_B2 + h * 16, xa1, a2, [&](int r) { if (r < 8) mcp_relu_split4(l1[1][r >> 2], r & 3, xb1[r >> 1]); });
        // B layer 2 | ReLU + split of A's layer 2 (its second tile was finished four k-steps before it is first read)
        split_layer<2, NF_SPLIT, 0>(w2l, lds + SP_B2 + h * 16, xb1, b2t, [&](int r) { if (r < 8) mcp_relu_split4(a2[r >> 2], r & 3, xa2[r >> 1]); });
        // A layer 3 | ReLU + split of B's layer 2, then the channel max of A's tiles 0 and 1 (max over ReLU = ReLU of max)
        split_layer<4, NF_SPLIT, NF_MAX>(w3l, lds + SP_B3 + h * 16, xa2, a3, [&](int r) {
            if (r < 8) mcp_relu_split4(b2t[r >> 2], r & 3, xb2[r >> 1]);
            else ma = max4(ma, a3[(r - 8) >> 2], (r - 8) & 3);
        });
        // B layer 3 | the channel max of A's tiles 2 and 3, then of B's tiles 0 and 1
        split_layer<4, NF_MAX, NF_MAX>(w3l, lds + SP_B3 + h * 16, xb2, b3t, [&](int r) {
            if (r < 8) ma = max4(ma, a3[2 + (r >> 2)], r & 3);
            else mb = max4(mb, b3t[(r - 8) >> 2], (r - 8) & 3);
        });
#pragma unroll
        for (int u = 0; u < 8; ++u) mb = max4(mb, b3t[2 + (u >> 2)], u & 3);
        score[0] = fmaxf(ma, __shfl_xor(ma, 32));  // the two lane halves hold the other 64 channels
        score[1] = fmaxf(mb, __shfl_xor(mb, 32));
        const float mx = wave_max(fmaxf(score[0], score[1]));
        const float e0 = expf(score[0] - mx), e1 = expf(score[1] - mx);
        const float den = wave_sum(e0 + e1);
        const float sx = wave_sum(e0 * nbx[0] + e1 * nbx[1]);
        const float sy = wave_sum(e0 * nby[0] + e1 * nby[1]);
        const float sz = wave_sum(e0 * nbz[0] + e1 * nbz[1]);
        if (lane == 0) {
            out[p * 3 + 0] = sx / den;
            out[p * 3 + 1] = sy / den;
            out[p * 3 + 2] = sz / den;
        }
    }
}

// ---- host side of mcp_fusion (FUS_LEN 0) and mcp_fusion_lengths (FUS_LEN 1): the grid from the PADDED shape, the launch ----
// 8 rounds of workgroups over the 512 resident slots rather than 2: the points are dealt out statically, so when another
// stream's kernels hold some CUs (the next step's FPS chains take 16-24 of them, workgroups that leave no room for one of
// these) a 2-round grid ends on the slowest slots -- measured 1.63 ms in the step against 1.34 ms alone; 8 rounds let the
// dispatcher rebalance (1.38 ms in the step) and cost nothing alone (the weight staging is ~1 % of a 48-point workgroup).
constexpr long long FUS_GRID_CAP = 4096;
unsigned fusion_grid(long long total, long long grid_cap) { return (unsigned)min((total + WAVES - 1) / WAVES, grid_cap); }

int fusion_split_run(long long total, int n, const float *p1, const float *p2, const int *idx, const int *idx2, const float *w1, const float *b1,
                     const float *w2, const float *b2, const float *w3, const float *b3, float *out, unsigned grid, hipStream_t s FUS_LENS_PARAM) {
    if (const int rc = mcp_allow_lds<FUS_KERNEL>()) return rc;
    hipLaunchKernelGGL(FUS_KERNEL, dim3(grid), dim3(64 * WAVES), SP_LDS_BYTES, s, total, n, p1, p2, idx, idx2, w1, b1, w2, b2, w3, b3, out FUS_LENS);
    return mcp_launch_status();
}

}  // namespace
