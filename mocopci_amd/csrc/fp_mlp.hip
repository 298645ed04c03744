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
#include <math.h>

#include "common.h"
#include "mfma_split.h"
#include "fp_mlp_shape.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

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
    int ksb, kss;
    int ks0, ks1, ks2, t0, t1, t2, b0, b1, b2;  // per layer: k-steps, output tiles, bias offset (named: never indexed at run time)
    int w_u4, small_floats;
};

struct FpRaw {  // what one input k-step of layer 1 reads: the two float4 of each of the three known rows, or of the skip row (in a*)
    float4 a0, a1, b0, b1, c0, c1;
};

template <int TMAX, bool STREAM>
__global__ __launch_bounds__(THREADS, TMAX == 8 ? 1 : 2) void fp_mlp_kernel(const FpArgs a, const float *__restrict__ known_feats, const float *__restrict__ skip,
                                                                         const int *__restrict__ idx, const float *__restrict__ dist,
                                                                         const float *__restrict__ w3, const int *__restrict__ ulen,
                                                                         const float *__restrict__ packed, float *__restrict__ out) {
    constexpr int LOADS = (TMAX * TILE_U4 + THREADS - 1) / THREADS;
    constexpr int BUF = LOADS * THREADS;  // uint4 of one LDS slab buffer: the widest slab rounded up to whole passes of the workgroup
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *small = lds;                                               // biases
    u32x4 *wl = reinterpret_cast<u32x4 *>(lds + a.small_floats);      // whole image, or [2][BUF]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, col = lane & 31;
    const u32x4 *gimg = reinterpret_cast<const u32x4 *>(packed);

    auto tiles_of = [&](int l) { return l == 0 ? a.t0 : l == 1 ? a.t1 : l == 2 ? a.t2 : 0; };
    auto ks_of = [&](int l) { return l == 0 ? a.ks0 : l == 1 ? a.ks1 : l == 2 ? a.ks2 : 0; };

    // ---- the slab sequence: begin_slab(l) gives this lane's entry of the next slab (a slab of layer l), end_slab() releases it ----
    u32x4 pre[LOADS];                 // staging registers of the slab after the one being multiplied
    const u32x4 *nxt_src = gimg;      // streamed: where the next slab to fetch starts, its layer, and that layer's slabs still to fetch
    int nxt_layer = 0, nxt_left = a.ks0, cur = 0;
    const u32x4 *wcur = wl;           // staged whole: the next slab in LDS
#pragma unroll
    for (int u = 0; u < LOADS; ++u) pre[u] = u32x4{0u, 0u, 0u, 0u};
    auto fetch_slab = [&]() {
        if (nxt_layer < a.layers) {
            const int n4 = tiles_of(nxt_layer) * TILE_U4;
#pragma unroll
            for (int u = 0; u < LOADS; ++u) pre[u] = nxt_src[min(tid + u * THREADS, n4 - 1)];  // entries past the slab repeat its last one, never used
            nxt_src += n4;
            if (--nxt_left == 0) {
                ++nxt_layer;
                nxt_left = ks_of(nxt_layer);
            }
        }
    };
    auto stash = [&](int buf) {
#pragma unroll
        for (int u = 0; u < LOADS; ++u) wl[buf * BUF + tid + u * THREADS] = pre[u];
    };
    auto begin_slab = [&](int l) -> const uint4 * {
        if constexpr (STREAM) {
            fetch_slab();
            __syncthreads();  // the slab is complete in buffer cur; nobody reads buffer cur ^ 1 any more
            return reinterpret_cast<const uint4 *>(wl + cur * BUF) + lane;
        } else {
            const u32x4 *w = wcur;
            wcur += tiles_of(l) * TILE_U4;
            return reinterpret_cast<const uint4 *>(w) + lane;
        }
    };
    auto end_slab = [&]() {
        if constexpr (STREAM) {
            stash(cur ^ 1);
            cur ^= 1;
        }
    };

    {
        const float4 *src = reinterpret_cast<const float4 *>(packed) + a.w_u4;
        for (int e = tid; e < a.small_floats / 4; e += THREADS) reinterpret_cast<float4 *>(small)[e] = src[e];
        if constexpr (STREAM) {
            fetch_slab();
            stash(0);
        } else {
            for (int e = tid; e < a.w_u4; e += THREADS) wl[e] = gimg[e];
        }
    }
    __syncthreads();

    // ---- this column's row: liveness, the three weights, the three known rows ----
    const long long p = ((long long)blockIdx.x * WAVES + wave) * 32 + col;
    const bool inr = p < a.total;
    const long long bb = inr ? mcp_div(p, a.n, mcp_fits32(a.total)) : 0;
    bool live = inr;
    if (inr && ulen) {
        const int ul = min(max(ulen[bb], 0), a.n);
        live = (int)(p - bb * a.n) < ul;
    }
    float w0 = 0.f, w1 = 0.f, w2 = 0.f;
    bool u0 = false, u1 = false, u2 = false;  // the slot's row is read
    const float *f0 = known_feats, *f1 = known_feats, *f2 = known_feats;
    const float *srow = skip;
    if (live) {
        const int *ip = idx + p * 3;
        const long long base = bb * a.m;
        f0 = known_feats + (base + ip[0]) * a.c2;
        f1 = known_feats + (base + ip[1]) * a.c2;
        f2 = known_feats + (base + ip[2]) * a.c2;
        if (a.c1) srow = skip + p * a.c1;
        if (a.rule == 0) {
            w0 = w3[p * 3 + 0]; w1 = w3[p * 3 + 1]; w2 = w3[p * 3 + 2];
            u0 = u1 = u2 = true;
        } else {
            float d0 = dist[p * 3 + 0], d1 = dist[p * 3 + 1], d2 = dist[p * 3 + 2];
            u0 = d0 < INFINITY; u1 = d1 < INFINITY; u2 = d2 < INFINITY;
            if (a.rule == 1) {
                d0 = d0 + 1e-8f; d1 = d1 + 1e-8f; d2 = d2 + 1e-8f;
            } else {
                d0 = d0 * d0; d1 = d1 * d1; d2 = d2 * d2;
                d0 = d0 < 1e-10f ? 1e-10f : d0; d1 = d1 < 1e-10f ? 1e-10f : d1; d2 = d2 < 1e-10f ? 1e-10f : d2;
            }
            const float r0 = u0 ? 1.0f / d0 : 0.f, r1 = u1 ? 1.0f / d1 : 0.f, r2 = u2 ? 1.0f / d2 : 0.f;
            const float sum = (r0 + r1) + r2;
            const bool any = sum > 0.f;  // false: no known point at all -- zeros, not 0 / 0
            w0 = any ? r0 / sum : 0.f; w1 = any ? r1 / sum : 0.f; w2 = any ? r2 / sum : 0.f;
        }
    }
    const bool skip_q = (a.c1 & 3) == 0;  // skip rows are 16-byte aligned

    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    auto fetch = [&](int s) {
        FpRaw r{z4, z4, z4, z4, z4, z4};
        if (s < a.ksb) {
            const int ch0 = 16 * s + 4 * h, ch1 = ch0 + 8;
            if (ch0 < a.c2) {
                if (u0) r.a0 = *reinterpret_cast<const float4 *>(f0 + ch0);
                if (u1) r.b0 = *reinterpret_cast<const float4 *>(f1 + ch0);
                if (u2) r.c0 = *reinterpret_cast<const float4 *>(f2 + ch0);
            }
            if (ch1 < a.c2) {
                if (u0) r.a1 = *reinterpret_cast<const float4 *>(f0 + ch1);
                if (u1) r.b1 = *reinterpret_cast<const float4 *>(f1 + ch1);
                if (u2) r.c1 = *reinterpret_cast<const float4 *>(f2 + ch1);
            }
        } else if (live) {
            const int ch0 = 16 * (s - a.ksb) + 4 * h, ch1 = ch0 + 8;
            if (skip_q) {
                if (ch0 < a.c1) r.a0 = *reinterpret_cast<const float4 *>(srow + ch0);
                if (ch1 < a.c1) r.a1 = *reinterpret_cast<const float4 *>(srow + ch1);
            } else {
                if (ch0 + 0 < a.c1) r.a0.x = srow[ch0 + 0];
                if (ch0 + 1 < a.c1) r.a0.y = srow[ch0 + 1];
                if (ch0 + 2 < a.c1) r.a0.z = srow[ch0 + 2];
                if (ch0 + 3 < a.c1) r.a0.w = srow[ch0 + 3];
                if (ch1 + 0 < a.c1) r.a1.x = srow[ch1 + 0];
                if (ch1 + 1 < a.c1) r.a1.y = srow[ch1 + 1];
                if (ch1 + 2 < a.c1) r.a1.z = srow[ch1 + 2];
                if (ch1 + 3 < a.c1) r.a1.w = srow[ch1 + 3];
            }
        }
        return r;
    };
    auto blend = [&](float fa, float fb, float fc) { return (w0 * fa + w1 * fb) + w2 * fc; };
    auto finish = [&](const FpRaw &r, int s) {
        float v[8];
        if (s < a.ksb) {
            v[0] = blend(r.a0.x, r.b0.x, r.c0.x); v[1] = blend(r.a0.y, r.b0.y, r.c0.y);
            v[2] = blend(r.a0.z, r.b0.z, r.c0.z); v[3] = blend(r.a0.w, r.b0.w, r.c0.w);
            v[4] = blend(r.a1.x, r.b1.x, r.c1.x); v[5] = blend(r.a1.y, r.b1.y, r.c1.y);
            v[6] = blend(r.a1.z, r.b1.z, r.c1.z); v[7] = blend(r.a1.w, r.b1.w, r.c1.w);
        } else {
            v[0] = r.a0.x; v[1] = r.a0.y; v[2] = r.a0.z; v[3] = r.a0.w;
            v[4] = r.a1.x; v[5] = r.a1.y; v[6] = r.a1.z; v[7] = r.a1.w;
        }
        return mcp_split8(v);
    };

    auto bias_bank = [&](f32x16(&bank)[TMAX], int boff, int tiles) {
#pragma unroll
        for (int o = 0; o < TMAX; ++o) {
#pragma unroll
            for (int r = 0; r < 16; ++r) bank[o][r] = 0.f;
            if (o < tiles) {
                const float4 *bq = reinterpret_cast<const float4 *>(small + boff + (o * 2 + h) * 16);
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const float4 v = bq[g];
                    bank[o][4 * g + 0] = v.x; bank[o][4 * g + 1] = v.y; bank[o][4 * g + 2] = v.z; bank[o][4 * g + 3] = v.w;
                }
            }
        }
    };
    // one k-step slab into every output tile of a bank
    auto slab_into = [&](f32x16(&bank)[TMAX], int l, int tiles, const McpSplit3 &xs) {
        const uint4 *w = begin_slab(l);
#pragma unroll
        for (int o = 0; o < TMAX; ++o)
            if (o < tiles) bank[o] = mcp_mfma_split(w + o * TILE_U4, xs, bank[o]);
        // The wave-uniform branches around absent tiles leave paths on which this compiler moves a finished tile between register
        // files 8 .. 11 wait states after its last MFMA (12 are needed; its hazard pass does not follow those branch chains, and
        // tools/isa_lint.py finds them).  16 idle issue slots after the slab's last MFMA cover every such path; they pass while the
        // matrix pipe is still busy with that MFMA.
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_nop 15");
        __builtin_amdgcn_sched_barrier(0);
        end_slab();
    };
    // layer l >= 1: the previous bank tile by tile through ReLU and the operand split into every output tile of the other bank
    auto next_layer = [&](f32x16(&src)[TMAX], f32x16(&dst)[TMAX], int l, int tin, int tout, int boff) {
        bias_bank(dst, boff, tout);
#pragma unroll
        for (int t = 0; t < TMAX; ++t) {
            if (t < tin) {
                f32x16 r = src[t];
#pragma unroll
                for (int i = 0; i < 16; ++i) r[i] = fmaxf(r[i], 0.f);
#pragma unroll
                for (int half = 0; half < 2; ++half) slab_into(dst, l, tout, mcp_split_kstep(r, half));
            }
        }
    };
    auto store_bank = [&](f32x16(&bank)[TMAX], int tiles) {
        if (!inr) return;
        float *orow = out + p * (tiles * 32) + 4 * h;
#pragma unroll
        for (int o = 0; o < TMAX; ++o) {
            if (o < tiles) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    float4 v = make_float4(fmaxf(bank[o][4 * g + 0], 0.f), fmaxf(bank[o][4 * g + 1], 0.f), fmaxf(bank[o][4 * g + 2], 0.f),
                                           fmaxf(bank[o][4 * g + 3], 0.f));
                    if (!live) v = z4;
                    *reinterpret_cast<float4 *>(orow + 32 * o + 8 * g) = v;
                }
            }
        }
    };

    f32x16 bank_a[TMAX], bank_b[TMAX];
    // ---- layer 1: input k-steps from memory ----
    bias_bank(bank_a, a.b0, a.t0);
    {
        FpRaw now = fetch(0);
#pragma unroll 1
        for (int s = 0; s < a.ks0; ++s) {
            const FpRaw nxt = fetch(min(s + 1, a.ks0 - 1));  // the last k-step fetches itself again: no branch in the loop body
            slab_into(bank_a, 0, a.t0, finish(now, s));
            now = nxt;
        }
    }
    if (a.layers == 1) {
        store_bank(bank_a, a.t0);
    } else {
        next_layer(bank_a, bank_b, 1, a.t0, a.t1, a.b1);
        if (a.layers == 2) {
            store_bank(bank_b, a.t1);
        } else {
            next_layer(bank_b, bank_a, 2, a.t1, a.t2, a.b2);
            store_bank(bank_a, a.t2);
        }
    }
}

template <int TMAX, bool STREAM>
int launch_fp_mlp(const FpArgs &a, const float *known_feats, const float *skip, const int *idx, const float *dist, const float *w3, const int *ulen,
                  const float *packed, float *out, hipStream_t s) {
    auto kern = fp_mlp_kernel<TMAX, STREAM>;
    static McpPerDeviceOnce attr_once;
    if (attr_once.need()) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return (int)e;
        attr_once.done();
    }
    constexpr int LOADS = (TMAX * TILE_U4 + THREADS - 1) / THREADS;
    const size_t lds = (size_t)a.small_floats * sizeof(float) + (STREAM ? (size_t)2 * LOADS * THREADS * 16 : (size_t)a.w_u4 * 16);
    const long long grid = (a.total + 32 * WAVES - 1) / (32 * WAVES);
    if (grid > 0x7FFFFFFFLL) return MCP_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(THREADS), lds, s, a, known_feats, skip, idx, dist, w3, ulen, packed, out);
    return mcp_launch_status();
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
    a.ksb = sh.ksb; a.kss = sh.kss;
    a.ks0 = sh.ks[0]; a.ks1 = sh.ks[1]; a.ks2 = sh.ks[2];
    a.t0 = sh.tiles[0]; a.t1 = sh.tiles[1]; a.t2 = sh.tiles[2];
    a.b0 = sh.boff[0]; a.b1 = sh.boff[1]; a.b2 = sh.boff[2];
    a.w_u4 = sh.w_u4;
    a.small_floats = sh.small_floats;
    hipStream_t s = (hipStream_t)stream;
    const bool whole = fp_weights_in_lds(sh);
#define FP_LAUNCH(T)                                                                                                       \
    return whole ? launch_fp_mlp<T, false>(a, known_feats, skip, idx, dist, w3, ulen, packed, out, s)                      \
                 : launch_fp_mlp<T, true>(a, known_feats, skip, idx, dist, w3, ulen, packed, out, s)
    if (sh.tmax == 2) FP_LAUNCH(2);
    if (sh.tmax == 4) FP_LAUNCH(4);
    FP_LAUNCH(8);
#undef FP_LAUNCH
}
