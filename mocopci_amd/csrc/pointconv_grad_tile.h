// pointconv_grad_tile.h -- pointconv_agg_grad_kernel (pointconv_grad.hip), stated once for the dense unit and for
// pointconv_lengths.hip.  The including unit sets the compile-time parameter, as fusion_bn_pass.h has it: PCG_LEN 0 is
// pointconv_agg_grad_kernel with its parameters as they were, PCG_LEN 1 pointconv_agg_grad_lengths_kernel with `const int *qlen`
// behind them.  (A forceinline body under a __global__ wrapper commuted 17 of the dense kernel's additions, so the text stays in
// the kernel.)  PCG_LEN 0 is the dense kernel, instruction for instruction (profiles/pointconv_lengths_resources.txt).  PCG_LEN 1: centre i of element bb is live iff
// i < min(max(qlen[bb], 0), s); a padded centre has no input read (idx row, new_xyz, gathered rows, grad_out), its rows of
// grad_new_xyz / grad_gxyz / grad_rows are exact zeros and it adds exact zeros to the 176 weight gradients -- from zeros in place of
// its loads, never from padding times zero.  The deal of centre pairs to waves and the order of every sum are the dense kernel's.
// The host side is stated once as well, under the same parameter: pcg_run at the end of this file, which both exported functions call.
#pragma once
#include "common.h"

#ifndef PCG_LEN
#error "define PCG_LEN (0 or 1) before including pointconv_grad_tile.h"
#endif
#if PCG_LEN
#define PCG_KERNEL pointconv_agg_grad_lengths_kernel
#define PCG_LENS_PARAM , const int *__restrict__ qlen
#define PCG_LENS , qlen
#define PCG_LENS_MISALIGNED || (((uintptr_t)qlen) & 3)   // host: scalar loads only
#define PCG_LOAD(inside) (valid && (inside))   // a gathered row is read for a live centre only
#else
#define PCG_KERNEL pointconv_agg_grad_kernel
#define PCG_LENS_PARAM
#define PCG_LENS
#define PCG_LENS_MISALIGNED
#define PCG_LOAD(inside) (inside)
#endif

namespace {

#ifndef MCP_POINTCONV_K_WN   // shared with pointconv_tile.h (pointconv_lengths.hip includes both)
#define MCP_POINTCONV_K_WN
constexpr int K = 32, WN = 8;
#endif
constexpr int WAVES = 4;
// weight-gradient vector: dW0 (8,3) | db0 (8) | dW1 (8,8) | db1 (8) | dW2 (8,8) | db2 (8)
constexpr int G_W0 = 0, G_B0 = 24, G_W1 = 32, G_B1 = 96, G_W2 = 104, G_B2 = 168, G_FLOATS = 176;
constexpr int MAX_D = 256;

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float half_sum(float v) {  // over the 32 lanes that share lane >> 5
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

#if PCG_LEN
// live length of element bb as the kernel sees it; centre p (of element bb) is live
__device__ __forceinline__ int pcg_len(const int *__restrict__ qlen, long long bb, int s) { return min(max(qlen[bb], 0), s); }
__device__ __forceinline__ bool pcg_live(const int *__restrict__ qlen, long long p, long long total, int s, bool f32) {
    if (p >= total) return false;
    const long long bb = mcp_div(p, s, f32);
    return p - bb * s < (long long)pcg_len(qlen, bb, s);
}
#endif

__global__ __launch_bounds__(64 * WAVES, 1) void PCG_KERNEL(long long total, int n, int s, int d, const float *__restrict__ s_xyz,
                                                                        const float *__restrict__ new_xyz, const float *__restrict__ s_points,
                                                                        const int *__restrict__ idx, const float *__restrict__ w0,
                                                                        const float *__restrict__ b0, const float *__restrict__ w1,
                                                                        const float *__restrict__ b1, const float *__restrict__ w2,
                                                                        const float *__restrict__ b2, const float *__restrict__ gout,
                                                                        float *__restrict__ d_new_xyz, float *__restrict__ d_gxyz,
                                                                        float *__restrict__ d_rows, float *__restrict__ partial PCG_LENS_PARAM) {
    extern __shared__ __attribute__((aligned(16))) float lds[];  // per wave: dL/dout of its two centres, 2 x (3 + d) x 8 floats
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, pl = lane >> 5, k = lane & 31;
    const int cin = d + 3, arow = cin * WN;  // floats per centre
    float *la = lds + (size_t)wave * 2 * arow;
    const float4 *mine = reinterpret_cast<const float4 *>(la + pl * arow);
    const bool f32 = mcp_fits32(total);
    float acc[G_FLOATS];
#pragma unroll
    for (int e = 0; e < G_FLOATS; ++e) acc[e] = 0.f;

    const long long pairs = (total + 1) >> 1;
    const McpUnits units = mcp_units_by_xcd(pairs, WAVES);   // XCD x takes the x-th eighth of the centre pairs (common.h)
    for (long long it = units.first + wave; it < units.limit; it += units.stride) {
        const long long p = 2 * it + pl;
#if PCG_LEN
        // a padded centre is a lane without a centre, and such a lane works on ZEROS: padding may hold NaN, which a zero gradient
        // would not silence.  Its rows are written as zeros; a wave without a live centre writes them and moves on.
        // (`it` is wave-uniform; said so, the two lengths are scalar loads and no lane's idx load waits behind a vector load of them)
        const long long itu = ((long long)__builtin_amdgcn_readfirstlane((int)(it >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)it);
        const bool live0 = pcg_live(qlen, 2 * itu, total, s, f32), live1 = pcg_live(qlen, 2 * itu + 1, total, s, f32);
        const bool valid = pl ? live1 : live0;
        const long long pc = p < total ? p : total - 1;
        if (!valid && p < total) {
            float4 *zrow = reinterpret_cast<float4 *>(d_rows + (p * K + k) * d);
            for (int c4 = 0; c4 < (d >> 2); ++c4) zrow[c4] = make_float4(0.f, 0.f, 0.f, 0.f);
            float *z = d_gxyz + (p * K + k) * 3;
            z[0] = 0.f; z[1] = 0.f; z[2] = 0.f;
            if (k < 3) d_new_xyz[p * 3 + k] = 0.f;
        }
        if (!live0 && !live1) continue;
#else
        const bool valid = p < total;
        const long long pc = valid ? p : total - 1;  // a lane without a centre works on the last one with a zero gradient
#endif
        __builtin_amdgcn_wave_barrier();
        for (int e = lane; e < 2 * (arow >> 2); e += 64) {
            const int half = e >= (arow >> 2), o = e - half * (arow >> 2);
            const long long pp = 2 * it + half;
#if PCG_LEN
            reinterpret_cast<float4 *>(la)[e] = (half ? live1 : live0) ? reinterpret_cast<const float4 *>(gout + pp * arow)[o] : make_float4(0.f, 0.f, 0.f, 0.f);
#else
            reinterpret_cast<float4 *>(la)[e] = pp < total ? reinterpret_cast<const float4 *>(gout + pp * arow)[o] : make_float4(0.f, 0.f, 0.f, 0.f);
#endif
        }
        __builtin_amdgcn_wave_barrier();
        const long long bb = mcp_div(pc, s, f32);
#if PCG_LEN
        const int id = valid ? idx[pc * K + k] : 0;
        const float *q = s_xyz + ((long long)bb * n + id) * 3;
        const float x0 = valid ? q[0] - new_xyz[pc * 3 + 0] : 0.f, x1 = valid ? q[1] - new_xyz[pc * 3 + 1] : 0.f, x2 = valid ? q[2] - new_xyz[pc * 3 + 2] : 0.f;
#else
        const int id = idx[pc * K + k];
        const float *q = s_xyz + ((long long)bb * n + id) * 3;
        const float x0 = q[0] - new_xyz[pc * 3 + 0], x1 = q[1] - new_xyz[pc * 3 + 1], x2 = q[2] - new_xyz[pc * 3 + 2];
#endif
        // every lane walks its own gathered row: with one wave per SIMD (176 accumulators per lane) nothing hides a load, and two loads
        // in flight (the old unroll-by-2 loop) left 65 % of the wave's time in s_waitcnt (round 5 counters).  The row is read in chunks
        // of CHUNK float4: the first chunk's loads are issued here, in front of the WeightNet arithmetic, every later chunk's while the
        // one before it is used.
        constexpr int CHUNK = 8;
        const float4 *row = reinterpret_cast<const float4 *>(s_points + ((long long)bb * n + id) * d);
        const int quads = d >> 2;
        float4 cur[CHUNK], nxt[CHUNK];
#pragma unroll
        for (int i = 0; i < CHUNK; ++i) cur[i] = PCG_LOAD(i < quads) ? row[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        // ---- the WeightNet again (pointconv_agg_kernel's fma order) ----
        float h0[WN], h1[WN], h2[WN];
#pragma unroll
        for (int j = 0; j < WN; ++j)
            h0[j] = fmaxf(__builtin_fmaf(w0[j * 3 + 2], x2, __builtin_fmaf(w0[j * 3 + 1], x1, __builtin_fmaf(w0[j * 3], x0, b0[j]))), 0.f);
#pragma unroll
        for (int j = 0; j < WN; ++j) {
            float a = b1[j];
#pragma unroll
            for (int i = 0; i < WN; ++i) a = __builtin_fmaf(w1[j * WN + i], h0[i], a);
            h1[j] = fmaxf(a, 0.f);
        }
#pragma unroll
        for (int j = 0; j < WN; ++j) {
            float a = b2[j];
#pragma unroll
            for (int i = 0; i < WN; ++i) a = __builtin_fmaf(w2[j * WN + i], h1[i], a);
            h2[j] = fmaxf(a, 0.f);
        }
        // ---- one pass over [dxyz | gathered feature row]: the pair's input gradient and dL/dw ----
        float dw[WN];
#pragma unroll
        for (int m = 0; m < WN; ++m) dw[m] = 0.f;
        auto channel = [&](float v, int c) {  // returns d v, accumulates dw
            const float4 a = mine[2 * c], b = mine[2 * c + 1];
            float g = a.x * h2[0];
            g = __builtin_fmaf(a.y, h2[1], g); g = __builtin_fmaf(a.z, h2[2], g); g = __builtin_fmaf(a.w, h2[3], g);
            g = __builtin_fmaf(b.x, h2[4], g); g = __builtin_fmaf(b.y, h2[5], g); g = __builtin_fmaf(b.z, h2[6], g); g = __builtin_fmaf(b.w, h2[7], g);
            dw[0] = __builtin_fmaf(v, a.x, dw[0]); dw[1] = __builtin_fmaf(v, a.y, dw[1]); dw[2] = __builtin_fmaf(v, a.z, dw[2]);
            dw[3] = __builtin_fmaf(v, a.w, dw[3]); dw[4] = __builtin_fmaf(v, b.x, dw[4]); dw[5] = __builtin_fmaf(v, b.y, dw[5]);
            dw[6] = __builtin_fmaf(v, b.z, dw[6]); dw[7] = __builtin_fmaf(v, b.w, dw[7]);
            return g;
        };
        float dg0 = channel(x0, 0), dg1 = channel(x1, 1), dg2 = channel(x2, 2);
        {
            float4 *orow = reinterpret_cast<float4 *>(d_rows + (pc * K + k) * d);
            for (int c0 = 0; c0 < quads; c0 += CHUNK) {
#pragma unroll
                for (int i = 0; i < CHUNK; ++i) nxt[i] = PCG_LOAD(c0 + CHUNK + i < quads) ? row[c0 + CHUNK + i] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                for (int i = 0; i < CHUNK; ++i) {
                    const int c4 = c0 + i;
                    if (c4 < quads) {   // wave-uniform
                        const float4 f = cur[i];
                        float4 o;
                        o.x = channel(f.x, 3 + 4 * c4 + 0);
                        o.y = channel(f.y, 3 + 4 * c4 + 1);
                        o.z = channel(f.z, 3 + 4 * c4 + 2);
                        o.w = channel(f.w, 3 + 4 * c4 + 3);
                        if (valid) orow[c4] = o;
                    }
                }
#pragma unroll
                for (int i = 0; i < CHUNK; ++i) cur[i] = nxt[i];
            }
        }
        // ---- back through the WeightNet ----
        float dz2[WN], dz1[WN], dz0[WN];
#pragma unroll
        for (int m = 0; m < WN; ++m) {
            dz2[m] = h2[m] > 0.f ? dw[m] : 0.f;
            acc[G_B2 + m] += dz2[m];
#pragma unroll
            for (int i = 0; i < WN; ++i) acc[G_W2 + m * WN + i] = __builtin_fmaf(dz2[m], h1[i], acc[G_W2 + m * WN + i]);
        }
#pragma unroll
        for (int i = 0; i < WN; ++i) {
            float a = w2[i] * dz2[0];
#pragma unroll
            for (int m = 1; m < WN; ++m) a = __builtin_fmaf(w2[m * WN + i], dz2[m], a);
            dz1[i] = h1[i] > 0.f ? a : 0.f;
            acc[G_B1 + i] += dz1[i];
#pragma unroll
            for (int j = 0; j < WN; ++j) acc[G_W1 + i * WN + j] = __builtin_fmaf(dz1[i], h0[j], acc[G_W1 + i * WN + j]);
        }
#pragma unroll
        for (int j = 0; j < WN; ++j) {
            float a = w1[j] * dz1[0];
#pragma unroll
            for (int i = 1; i < WN; ++i) a = __builtin_fmaf(w1[i * WN + j], dz1[i], a);
            dz0[j] = h0[j] > 0.f ? a : 0.f;
            acc[G_B0 + j] += dz0[j];
            acc[G_W0 + j * 3 + 0] = __builtin_fmaf(dz0[j], x0, acc[G_W0 + j * 3 + 0]);
            acc[G_W0 + j * 3 + 1] = __builtin_fmaf(dz0[j], x1, acc[G_W0 + j * 3 + 1]);
            acc[G_W0 + j * 3 + 2] = __builtin_fmaf(dz0[j], x2, acc[G_W0 + j * 3 + 2]);
            dg0 = __builtin_fmaf(w0[j * 3 + 0], dz0[j], dg0);
            dg1 = __builtin_fmaf(w0[j * 3 + 1], dz0[j], dg1);
            dg2 = __builtin_fmaf(w0[j * 3 + 2], dz0[j], dg2);
        }
        if (valid) {
            float *o = d_gxyz + (pc * K + k) * 3;
            o[0] = dg0; o[1] = dg1; o[2] = dg2;
        }
        const float sx = half_sum(dg0), sy = half_sum(dg1), sz = half_sum(dg2);
        if (valid && k == 0) {
            d_new_xyz[pc * 3 + 0] = -sx;
            d_new_xyz[pc * 3 + 1] = -sy;
            d_new_xyz[pc * 3 + 2] = -sz;
        }
    }
    // ---- weight gradients: butterfly per wave, waves in wave order, the workgroup's vector to the second pass ----
    __syncthreads();
    float *red = lds;  // [WAVES][176], over the staging rows (no longer needed)
#pragma unroll
    for (int e = 0; e < G_FLOATS; ++e) {
        const float v = wave_sum(acc[e]);
        if (lane == 0) red[wave * G_FLOATS + e] = v;
    }
    __syncthreads();
    if (tid < G_FLOATS) {
        float v = red[tid];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) v += red[w * G_FLOATS + tid];
        partial[(size_t)blockIdx.x * G_FLOATS + tid] = v;
    }
}

__global__ __launch_bounds__(256) void pointconv_grad_reduce_kernel(const float *__restrict__ partial, int parts, float *__restrict__ out) {
    const int e = threadIdx.x;
    if (e >= G_FLOATS) return;
    float v = 0.f;
    for (int g = 0; g < parts; ++g) v += partial[(size_t)g * G_FLOATS + e];
    out[e] = v;
}

unsigned grad_grid(long long total) {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    const long long want = (total + 2 * WAVES - 1) / (2 * WAVES), cap = cus;  // one resident workgroup per CU: 176 accumulators per lane, one wave per SIMD
    return (unsigned)(want < cap ? want : cap);
}

// ---- host side of mcp_pointconv_agg_grad (PCG_LEN 0) and mcp_pointconv_agg_grad_lengths (PCG_LEN 1), stated once: the argument
// checks, the grid and LDS size from the PADDED shape, the two launches ----
int pcg_run(int b, int n, int s, int d, int k, const float *s_xyz, const float *new_xyz, const float *s_points, const int *idx, const float *w0,
            const float *b0, const float *w1, const float *b1, const float *w2, const float *b2, const float *grad_out, float *grad_new_xyz,
            float *grad_gxyz, float *grad_rows, float *grad_weights, void *workspace, size_t workspace_bytes, hipStream_t st PCG_LENS_PARAM) {
    MCP_CHECK_ARGS(b > 0 && n > 0 && s > 0 && s_xyz && new_xyz && s_points && idx && w0 && b0 && w1 && b1 && w2 && b2 && grad_out && grad_new_xyz &&
                   grad_gxyz && grad_rows && grad_weights && workspace);
    if (k != K || d < 4 || (d & 3) || d > MAX_D) return MCP_ERR_UNSUPPORTED;
    if (((((uintptr_t)s_points) | ((uintptr_t)grad_out) | ((uintptr_t)grad_rows)) & 15) PCG_LENS_MISALIGNED) return MCP_ERR_BAD_ARG;
    const long long total = (long long)b * s;
    const unsigned grid = grad_grid(total);
    if (workspace_bytes < (size_t)grid * G_FLOATS * sizeof(float)) return MCP_ERR_BAD_ARG;
    size_t lds = (size_t)WAVES * 2 * (d + 3) * WN * sizeof(float);
    if (lds < (size_t)WAVES * G_FLOATS * sizeof(float)) lds = (size_t)WAVES * G_FLOATS * sizeof(float);
    if (const int rc = mcp_allow_lds<PCG_KERNEL>()) return rc;
    mcp_prof_begin(MCP_KERNEL_POINTCONV, st);
    hipLaunchKernelGGL(PCG_KERNEL, dim3(grid), dim3(64 * WAVES), lds, st, total, n, s, d, s_xyz, new_xyz, s_points, idx, w0, b0, w1, b1, w2, b2, grad_out,
                       grad_new_xyz, grad_gxyz, grad_rows, static_cast<float *>(workspace) PCG_LENS);
    hipLaunchKernelGGL(pointconv_grad_reduce_kernel, dim3(1), dim3(256), 0, st, static_cast<const float *>(workspace), (int)grid, grad_weights);
    mcp_prof_end(MCP_KERNEL_POINTCONV, st);
    return mcp_launch_status();
}

}  // namespace
