// fp_mlp.hip -- fused feature-propagation layer of pointnet2 (PointnetFPModule, pointnet2_modules.py:116-156; FeaturePropagation of
// models/layers.py:150-178) for gfx950: three-neighbour blend + skip concatenation + shared per-point MLP in one kernel.
//
// Reference formulation: three_interpolate writes (B, C2, n), torch.cat writes (B, C2 + C1, n), then up to three Conv2d(1x1) +
// BatchNorm2d + ReLU passes each write (B, C, n) -- at the largest point count of the network.  Here only the (B, n, C_out) row
// leaves registers.
//
// Contract (mcp_fp_mlp).  Channel-last known_feats (B, m, C2), skip (B, n, C1) or NULL with C1 = 0, idx (B, n, 3) int32, dist
// (B, n, 3) as three_nn returns it (square roots), w3 (B, n, 3) for rule 0, ulen (B) or NULL.  For a live row p of element bb:
//   * weights by `rule`:  0: w = w3 as given, dist is not read;
//                         1 (pointnet2_modules.py:139-142): r_j = 1 / (dist_j + 1e-8), w_j = r_j / ((r_0 + r_1) + r_2);
//                         2 (layers.py:162-169): d_j = dist_j * dist_j raised to at least 1e-10, r_j = 1 / d_j, same normalisation;
//   * under rules 1 and 2 a slot whose dist is +inf (three_nn over fewer than three known points) has weight exactly 0 and its
//     row of known_feats is not read; three infinite slots give an interpolated part of exact zeros.  No NaN is formed on the way
//     (the unit is built with -fno-honor-nans);
//   * x = [(w0 f[i0] + w1 f[i1]) + w2 f[i2] (C2 values) | skip[bb,p] (C1 values)]: rounded fp32 products, that sum order;
//   * h1 = ReLU(W1 x + b1), ..., out[bb,p] = ReLU(WL h(L-1) + bL) for 1 .. 3 layers; W_l is (widths[l], cin_l) row-major with
//     eval-mode BatchNorm already folded in by the caller;
//   * ulen as the query lengths elsewhere: device int32 array, clamped to [0, n] in the kernel, NULL = every row live; a row at or
//     beyond ulen[bb] writes zeros and none of its inputs (idx, dist, w3, skip) is read;
//   * every output element is written; indices are trusted; no allocation, no environment variable, no host read of a length;
//   * supported: C2 a multiple of 4 in 4 .. 512; C1 in 0 .. 512 (any value: a skip row that is no multiple of 16 bytes is read
//     dword by dword); C1 + C2 <= 768; 1 .. 3 layers of width 32, 64, 128 or 256; anything else MCP_ERR_UNSUPPORTED, nothing
//     launched.
//
// Tiling.  One wave owns 32 points, the MFMA column; four waves per workgroup, one workgroup per 128 rows of the flattened (B * n)
// list (a tile may straddle two elements).  Two banks of TMAX accumulator tiles (TMAX = 2, 4, 8: the widest layer / 32).  Layer 1
// walks its input k-steps (16 channels each: ceil(C2 / 16) of the blend, then ceil(C1 / 16) of the skip row; the raw rows of the next
// k-step are in flight while this one is multiplied) and accumulates into every output tile of bank A.  Each later layer walks the
// previous bank tile by tile -- ReLU, mcp_split_kstep twice -- and accumulates into every output tile of the other bank.  The last
// bank is stored through its ReLU.  All loops over tiles are fully unrolled, absent tiles are skipped by wave-uniform branches: no
// accumulator or operand array is indexed with a runtime value.
//
// Weights.  mcp_fp_mlp_pack writes the image slab by slab in the order the kernel consumes it: layer by layer, k-step by k-step,
// and inside a slab [output tile][piece][lane] x 16 B (mcp_split_weights' operand layout), then the biases in accumulator order.
// fp_weights_in_lds(shape) is the one dispatch predicate: an image of at most 64 KB is staged whole in LDS; a larger one (up to 1.5 MB)
// is streamed as mlp.hip streams its chunks -- the workgroup holds two slabs in LDS and fetches slab q + 1 while slab q is multiplied,
// one barrier per slab.
//
// The row, the gather, the slab sequence and the tile helpers are fp_mlp_tile.h's, shared with fp_mlp_grad.hip and fp_mlp_bn.hip.
#include "fp_mlp_tile.h"

namespace {

// One layer of the image: slab s (k-step s of the layer's input) holds, for every output tile t, the three pieces of the 8 values
// per lane W[32t + (lane&31)][column of (s, i, lane>>5)].  Input k-steps 0 .. ksa-1 cover columns 0 .. va-1 (zero beyond), the next
// cover columns va .. va+vb-1 (layer 1: the skip part after the blend part, each padded to whole k-steps).  Bias: [t][h][r].
__global__ __launch_bounds__(256) void fp_mlp_pack_kernel(const float *__restrict__ w, const float *__restrict__ b, int ld, int ksa, int va, int vb,
                                                          int ks, int tiles, uint4 *__restrict__ dstw, float *__restrict__ dstb) {
    const int first = blockIdx.x * 256 + threadIdx.x, stride = gridDim.x * 256;
    for (int e = first; e < tiles * ks * 64; e += stride) {
        const int lane = e & 63, t = (e >> 6) % tiles, s = (e >> 6) / tiles;
        const bool second = s >= ksa;
        const int sl = second ? s - ksa : s, valid = second ? vb : va, col0 = second ? va : 0;
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int ch = 32 * (sl >> 1) + mcp_chan_of(8 * (sl & 1) + i, lane >> 5);
            v[i] = ch < valid ? w[(size_t)(32 * t + (lane & 31)) * ld + col0 + ch] : 0.f;
        }
        const McpSplit3 sp = mcp_split8(v);
        uint4 *o = dstw + (size_t)(s * tiles + t) * TILE_U4 + lane;
        o[0] = sp.p1;
        o[64] = sp.p2;
        o[128] = sp.p3;
    }
    for (int e = first; e < tiles * 32; e += stride) {
        const int r = e & 15, h = (e >> 4) & 1, t = e >> 5;
        dstb[e] = b[32 * t + mcp_chan_of(r, h)];
    }
}

struct FpArgs {
    long long total;  // B * n rows
    int n, m, c2, c1, rule, layers;
    int ksb, ks0;                // k-steps of the blend, and of all of layer 1's input
    int t0, t1, t2, b0, b1, b2;  // per layer: output tiles, bias offset (named: never indexed at run time)
    int w_u4, small_floats;
};

template <int TMAX, bool STREAM>
__global__ __launch_bounds__(THREADS, TMAX == 8 ? 1 : 2) void fp_mlp_kernel(const FpArgs a, const float *__restrict__ known_feats, const float *__restrict__ skip,
                                                                         const int *__restrict__ idx, const float *__restrict__ dist,
                                                                         const float *__restrict__ w3, const int *__restrict__ ulen,
                                                                         const float *__restrict__ packed, float *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *small = lds;                                               // biases, then the whole image or two slab buffers
    const int tid = threadIdx.x, h = (tid & 63) >> 5;
    FpSlabs<TMAX, STREAM> slabs;
    {
        const float4 *src = reinterpret_cast<const float4 *>(packed) + a.w_u4;
        for (int e = tid; e < a.small_floats / 4; e += THREADS) reinterpret_cast<float4 *>(small)[e] = src[e];
        slabs.begin(reinterpret_cast<u32x4 *>(lds + a.small_floats), reinterpret_cast<const u32x4 *>(packed), a.t0, a.w_u4);
    }
    __syncthreads();

    const FpRow row(a.total, a.n, ulen);
    FpGather g;
    g.begin(row, a.m, a.c2, a.c1, a.rule, a.ksb, known_feats, skip, idx, dist, w3);

    auto bias_bank = [&](f32x16(&bank)[TMAX], int boff, int tiles) {
#pragma unroll
        for (int o = 0; o < TMAX; ++o) fp_bias_tile(bank[o], o, tiles, small + boff);
    };
    // layer l >= 1: the previous bank tile by tile through ReLU and the operand split into every output tile of the other bank;
    // `after`: the output tiles of the layer behind this one (0: none)
    auto next_layer = [&](f32x16(&src)[TMAX], f32x16(&dst)[TMAX], int tin, int tout, int boff, int after) {
        bias_bank(dst, boff, tout);
#pragma unroll
        for (int t = 0; t < TMAX; ++t) {
            if (t < tin) {
                f32x16 r = src[t];
#pragma unroll
                for (int i = 0; i < 16; ++i) r[i] = fmaxf(r[i], 0.f);
                slabs.into(dst, tout, mcp_split_kstep(r, 0), tout);
                slabs.into(dst, tout, mcp_split_kstep(r, 1), t + 1 == tin ? after : tout);
            }
        }
    };
    auto store_bank = [&](f32x16(&bank)[TMAX], int tiles) {
        if (!row.inr) return;
        const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
        float *orow = out + row.p * (tiles * 32) + 4 * h;
#pragma unroll
        for (int o = 0; o < TMAX; ++o) {
            if (o < tiles) {
#pragma unroll
                for (int g4 = 0; g4 < 4; ++g4) {
                    float4 v = make_float4(fmaxf(bank[o][4 * g4 + 0], 0.f), fmaxf(bank[o][4 * g4 + 1], 0.f), fmaxf(bank[o][4 * g4 + 2], 0.f),
                                           fmaxf(bank[o][4 * g4 + 3], 0.f));
                    if (!row.live) v = z4;
                    *reinterpret_cast<float4 *>(orow + 32 * o + 8 * g4) = v;
                }
            }
        }
    };

    f32x16 bank_a[TMAX], bank_b[TMAX];
    // ---- layer 1: input k-steps from memory ----
    bias_bank(bank_a, a.b0, a.t0);
    fp_ksteps(a.ks0, [&](int s) { return g.fetch(s); },
              [&](const FpGatherRaw &now, int s, bool last) { slabs.into(bank_a, a.t0, g.finish(now, s, nullptr, 0), last ? a.t1 : a.t0); });
    if (a.layers == 1) {
        store_bank(bank_a, a.t0);
    } else {
        next_layer(bank_a, bank_b, a.t0, a.t1, a.b1, a.t2);
        if (a.layers == 2) {
            store_bank(bank_b, a.t1);
        } else {
            next_layer(bank_b, bank_a, a.t1, a.t2, a.b2, 0);
            store_bank(bank_a, a.t2);
        }
    }
}

}  // namespace

MCP_EXPORT int mcp_fp_mlp_packed_floats(int c2, int c1, int layers, const int *widths) {
    FpShape sh;
    if (!fp_shape(c2, c1, layers, widths, &sh)) return 0;
    return sh.w_u4 * 4 + sh.small_floats;
}

MCP_EXPORT int mcp_fp_mlp_pack(int c2, int c1, int layers, const int *widths, const float *const *w, const float *const *b, float *packed,
                               mcp_stream_t stream) {
    MCP_CHECK_ARGS(widths && w && b && packed);
    FpShape sh;
    if (!fp_shape(c2, c1, layers, widths, &sh)) return MCP_ERR_UNSUPPORTED;
    for (int l = 0; l < layers; ++l) MCP_CHECK_ARGS(w[l] && b[l]);
    if (((uintptr_t)packed) & 15) return MCP_ERR_BAD_ARG;
    hipStream_t s = (hipStream_t)stream;
    uint4 *pw = reinterpret_cast<uint4 *>(packed);
    float *small = packed + (size_t)sh.w_u4 * 4;
    for (int l = 0; l < layers; ++l) {
        const int ld = l == 0 ? c2 + c1 : widths[l - 1];
        const int ksa = l == 0 ? sh.ksb : sh.ks[l], va = l == 0 ? c2 : ld, vb = l == 0 ? c1 : 0;
        const int work = sh.tiles[l] * sh.ks[l] * 64;
        hipLaunchKernelGGL(fp_mlp_pack_kernel, dim3((work + 255) / 256), dim3(256), 0, s, w[l], b[l], ld, ksa, va, vb, sh.ks[l], sh.tiles[l], pw,
                           small + sh.boff[l]);
        const int rc = mcp_launch_status();
        if (rc != MCP_OK) return rc;
        pw += (size_t)sh.tiles[l] * sh.ks[l] * TILE_U4;
    }
    return MCP_OK;
}

MCP_EXPORT int mcp_fp_mlp(int b, int n, int m, int c2, int c1, int rule, int layers, const int *widths, const float *known_feats, const float *skip,
                          const int *idx, const float *dist, const float *w3, const int *ulen, const float *packed, float *out,
                          mcp_stream_t stream) {
    MCP_CHECK_ARGS(b > 0 && n > 0 && m > 0 && widths && known_feats && idx && packed && out && rule >= 0 && rule <= 2);
    MCP_CHECK_ARGS((c1 <= 0 || skip) && (rule == 0 ? w3 != nullptr : dist != nullptr));
    FpShape sh;
    if (!fp_shape(c2, c1, layers, widths, &sh)) return MCP_ERR_UNSUPPORTED;
    if ((((uintptr_t)known_feats) | ((uintptr_t)out) | ((uintptr_t)packed) | ((c1 & 3) == 0 ? (uintptr_t)skip : 0)) & 15) return MCP_ERR_BAD_ARG;
    FpArgs a;
    a.total = (long long)b * n;
    a.n = n; a.m = m; a.c2 = c2; a.c1 = c1; a.rule = rule; a.layers = layers;
    a.ksb = sh.ksb; a.ks0 = sh.ks[0];
    a.t0 = sh.tiles[0]; a.t1 = sh.tiles[1]; a.t2 = sh.tiles[2];
    a.b0 = sh.boff[0]; a.b1 = sh.boff[1]; a.b2 = sh.boff[2];
    a.w_u4 = sh.w_u4;
    a.small_floats = sh.small_floats;
    return fp_dispatch(sh.tmax, !fp_weights_in_lds(sh), [&](auto tmax, auto stream_w) {
        constexpr int T = decltype(tmax)::value;
        constexpr bool S = decltype(stream_w)::value;
        return fp_launch<fp_mlp_kernel<T, S>, T, S>(a.total, a.small_floats, a.w_u4, (hipStream_t)stream, a, known_feats, skip, idx, dist, w3, ulen,
                                                    packed, out);
    });
}
