// group_mlp.hip -- fused set-abstraction layer of pointnet2 (PointnetSAModule[MSG], pointnet2_modules.py; SetConv and
// FlowEmbedding of models/layers.py) for gfx950: grouped gather + shared per-pair MLP + pool over the neighbours in one kernel.
//
// Reference formulation: QueryAndGroup writes (B, 3+C, M, nsample), up to three Conv2d(1x1) + BatchNorm2d + ReLU passes run over
// it, then a max (or mean) over the nsample axis.  Here nothing but the pooled (B, M, C_out) row leaves registers.
//
// Contract (mcp_group_mlp).  For a live centre p of element bb, with k_j = idx[bb,p,j], j = 0 .. nsample-1:
//     x_j  = [xyz[bb,k_j] - new_xyz[bb,p] (if use_xyz) | features[bb,k_j]]
//     h1_j = ReLU(W1 x_j + b1 (+ row_bias[bb,p]))          hl_j = ReLU(Wl h(l-1)_j + bl)
//     out[bb,p] = max_j hL_j (pool 0)  or  (sum_j hL_j) / nsample (pool 1)
//   * every slot counts, repeated indices included (the ball query's "repeat the first hit" padding needs no count);
//   * W_l is (widths[l], cin_l) row-major with eval-mode BatchNorm already folded in by the caller;
//   * qlen as in mcp_ball_query_lengths: device array, clamped to [0, m] in the kernel, NULL = every centre live; a centre at or
//     beyond qlen[bb] writes zeros and none of its rows (new_xyz, idx, row_bias) is read;
//   * supported: 1 <= nsample <= 64; c a multiple of 4 in 0 .. 128 (c = 0 needs use_xyz); 1 .. 3 layers; hidden widths in
//     {32, 64, 128}, last width in {32, 64, 128, 256}; anything else MCP_ERR_UNSUPPORTED, nothing launched;
//   * indices are trusted; no allocation, no environment variable, no host read of a length.
//
// Tiling.  One wave owns one 32-column MFMA tile at a time (persistent loop over tiles, four waves per workgroup, tiles dealt by
// XCD as in fusion.hip).  Neighbours sit on the MFMA column; a centre takes a group of P = 8, 16 or 32 columns (the next power of
// two >= nsample), so a tile carries 4, 2 or 1 centres of the flattened (B * M) centre list -- a tile may straddle two batch
// elements, and its last groups may lie beyond the list.  nsample > 32 is two tiles of one centre whose pooled rows meet in a
// wave-private LDS row.  Columns beyond nsample inside a group repeat slot 0 (harmless for the max) and are zeroed before the sum
// of the mean, which divides by nsample.
//
// Operands.  Gathered feature rows are loaded straight into the k-step layout of mfma_split.h with two 16-byte loads per lane and
// k-step (k-step s of lane half h holds channels 16s + 4h .. +3 and 16s + 8 + 4h .. +3); loads at or beyond c are not issued, the
// weight image holds zeros there.  The feature k-steps of layer 1 are rounded up to 1, 2, 4 or 8 (c = 68 .. 128 all run 8).  The
// three relative coordinates enter through the f32-input MFMA with K = 4 as in cross_kernel's position term: two
// v_mfma_f32_32x32x2_f32 per 32-channel tile (128 matrix cycles, no vector instruction) against 48 v_fma_f32 plus 48 LDS broadcasts
// per tile for fma chains.  Bias (and row_bias) is the accumulator's initial value.
//
// Arithmetic.  Every layer is mcp_tile_split on the accumulator-as-operand chain: ReLU and mcp_split_kstep apply where the
// accumulator leaves the values; the last layer is consumed one 32-channel tile at a time into the pool, a butterfly of DPP steps
// (and one cross-row shuffle for P = 32) inside the column group.
//
// Weights.  mcp_group_mlp_pack writes, per layer, the image of mcp_split_weights ([t_out][k-step][piece][lane] x 16 B), then the
// K = 4 position columns and the biases in accumulator order.  gm_weights_in_lds(c, widths) is the one dispatch predicate: an image
// of at most 64 KB is staged in LDS once per workgroup (two workgroups per CU still fit); a larger one is read through L2 tile by
// tile, as cross_grad_kernel<128> reads its image.  Register classes: KMAX = 4 (c <= 64 and hidden widths <= 64; two waves per
// SIMD) and KMAX = 8 (one wave per SIMD).
#include "common.h"
#include "mfma_split.h"
#include "group_mlp_shape.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr int WAVES = 4;
constexpr int POOL_ROW = 256;                 // floats of a wave's pooled row (the widest last layer)

// One layer of the image.  Pieces: mcp_split_weights' layout over the columns col0 .. col0 + cvalid - 1 of w (tiles * 32, ld),
// zero beyond cvalid up to 16 * ks.  pos (layer 1 only): [t][s][lane] = w[32t + (lane&31)][2s + (lane>>5)] for the three coordinate
// columns, 0 for the fourth.  Bias: [t][h][r].
__global__ __launch_bounds__(256) void group_mlp_pack_kernel(const float *__restrict__ w, const float *__restrict__ b, int ld, int col0, int cvalid,
                                                             int ks, int tiles, int use_xyz, uint4 *__restrict__ dstw, float *__restrict__ dstpos,
                                                             float *__restrict__ dstb) {
    const int first = blockIdx.x * 256 + threadIdx.x, stride = gridDim.x * 256;
    for (int e = first; e < tiles * ks * 64; e += stride) {
        const int lane = e & 63, s = (e >> 6) % ks, t = (e >> 6) / ks;
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int ch = 32 * (s >> 1) + mcp_chan_of(8 * (s & 1) + i, lane >> 5);
            v[i] = ch < cvalid ? w[(size_t)(32 * t + (lane & 31)) * ld + col0 + ch] : 0.f;
        }
        const McpSplit3 sp = mcp_split8(v);
        uint4 *o = dstw + (size_t)(t * ks + s) * 3 * 64 + lane;
        o[0] = sp.p1;
        o[64] = sp.p2;
        o[128] = sp.p3;
    }
    if (dstpos)
        for (int e = first; e < tiles * 128; e += stride) {
            const int lane = e & 63, s = (e >> 6) & 1, t = e >> 7, cc = 2 * s + (lane >> 5);
            dstpos[e] = (use_xyz && cc < 3) ? w[(size_t)(32 * t + (lane & 31)) * ld + cc] : 0.f;
        }
    for (int e = first; e < tiles * 32; e += stride) {
        const int r = e & 15, h = (e >> 4) & 1, t = e >> 5;
        dstb[e] = b[32 * t + mcp_chan_of(r, h)];
    }
}

struct GmArgs {
    long long total;  // B * M centres
    int n, m, c, nsample, use_xyz, pool, layers;
    int logp;         // log2 of the column group of a centre (3, 4, 5)
    int ctiles;       // column tiles per centre: 2 when nsample > 32
    int ks[MAX_LAYERS], tiles[MAX_LAYERS], woff[MAX_LAYERS], boff[MAX_LAYERS];
    int w_u4, small_floats;
};

template <int KMAX>
__device__ __forceinline__ f32x16 gm_tile_dyn(const uint4 *ws, const McpSplit3 *xs, int ks, f32x16 acc) {
    if constexpr (KMAX >= 8) {
        if (ks == 8) return mcp_tile_split<8>(ws, xs, acc);
    }
    if (ks == 4) return mcp_tile_split<4>(ws, xs, acc);
    if (ks == 2) return mcp_tile_split<2>(ws, xs, acc);
    return mcp_tile_split<1>(ws, xs, acc);
}

template <int KMAX, bool LDSW>
__global__ __launch_bounds__(64 * WAVES, KMAX == 4 ? 2 : 1) void group_mlp_kernel(const GmArgs a, const float *__restrict__ xyz, const float *__restrict__ new_xyz,
                                                                               const float *__restrict__ features, const int *__restrict__ idx,
                                                                               const int *__restrict__ qlen, const float *__restrict__ row_bias,
                                                                               const float *__restrict__ packed, float *__restrict__ out) {
    constexpr int HT = KMAX / 2;  // most output tiles of a hidden layer
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *small = lds;                                   // position columns | biases
    float *prow_all = lds + a.small_floats;               // [WAVES][POOL_ROW]
    uint4 *wlds = reinterpret_cast<uint4 *>(prow_all + WAVES * POOL_ROW);
    const int tid = threadIdx.x;
    {
        const float4 *src = reinterpret_cast<const float4 *>(packed) + a.w_u4;
        for (int e = tid; e < a.small_floats / 4; e += 64 * WAVES) reinterpret_cast<float4 *>(small)[e] = src[e];
        if (LDSW)
            for (int e = tid; e < a.w_u4; e += 64 * WAVES) wlds[e] = reinterpret_cast<const uint4 *>(packed)[e];
    }
    __syncthreads();
    const uint4 *wimg = LDSW ? wlds : reinterpret_cast<const uint4 *>(packed);

    const int lane = tid & 63, wave = tid >> 6, h = lane >> 5, col = lane & 31;
    float *prow = prow_all + wave * POOL_ROW;
    const int P = 1 << a.logp, G = 32 >> a.logp, slot = col & (P - 1);
    const int wfirst = a.tiles[0] * 32, wlast = a.tiles[a.layers - 1] * 32;
    const bool fits32 = mcp_fits32(a.total);
    const float fn = (float)a.nsample;

    auto bias_tile = [&](int l, int t, int hh) {
        f32x16 acc;
        const float4 *bq = reinterpret_cast<const float4 *>(small + a.boff[l] + (t * 2 + hh) * 16);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 v = bq[g];
            acc[4 * g + 0] = v.x; acc[4 * g + 1] = v.y; acc[4 * g + 2] = v.z; acc[4 * g + 3] = v.w;
        }
        return acc;
    };
    auto relu_tile = [&](f32x16 acc) {
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = fmaxf(acc[r], 0.f);
        return acc;
    };

    const long long units = (a.total + G - 1) / G;
    const McpUnits deal = mcp_units_by_xcd(units, WAVES);
    for (long long unit = deal.first + wave; unit < deal.limit; unit += deal.stride) {
        const long long p = unit * G + (col >> a.logp);  // this column's centre
        const bool inr = p < a.total;
        const long long bb = inr ? mcp_div(p, a.m, fits32) : 0;
        bool live = inr;
        if (inr && qlen) {
            const int ql = min(max(qlen[bb], 0), a.m);
            live = (int)(p - bb * a.m) < ql;
        }
        float cx = 0.f, cy = 0.f, cz = 0.f;
        if (live && a.use_xyz) { cx = new_xyz[p * 3 + 0]; cy = new_xyz[p * 3 + 1]; cz = new_xyz[p * 3 + 2]; }

        for (int ct = 0; ct < a.ctiles; ++ct) {
            // The lane's offset into the weight image, the position columns and the biases, opaque to the compiler once per tile: every
            // such address and bias value is invariant over the persistent loop, and hoisted out of it they cost hundreds of registers.
            int ll = lane, hl = h;
            asm volatile("" : "+v"(ll), "+v"(hl));
            const int j = ct * 32 + slot;
            const bool valid = j < a.nsample;
            const int k = live ? idx[p * a.nsample + (valid ? j : 0)] : 0;
            const long long row = bb * a.n + k;
            float in0 = 0.f, in1 = 0.f;
            if (live && a.use_xyz) {
                const float *q = xyz + row * 3;
                const float dx = q[0] - cx, dy = q[1] - cy, dz = q[2] - cz;
                in0 = h ? dy : dx;   // k-step 0: (dx, dy); k-step 1: (dz, 0)
                in1 = h ? 0.f : dz;
            }
            McpSplit3 xs0[KMAX];
#pragma unroll
            for (int s = 0; s < KMAX; ++s) {
                if (s < a.ks[0]) {
                    float v[8];
#pragma unroll
                    for (int g2 = 0; g2 < 2; ++g2) {
                        const int ch = 16 * s + 8 * g2 + 4 * h;
                        float4 f = make_float4(0.f, 0.f, 0.f, 0.f);
                        if (live && ch < a.c) f = *reinterpret_cast<const float4 *>(features + row * a.c + ch);
                        v[4 * g2 + 0] = f.x; v[4 * g2 + 1] = f.y; v[4 * g2 + 2] = f.z; v[4 * g2 + 3] = f.w;
                    }
                    xs0[s] = mcp_split8(v);
                }
            }

            // output tile t of layer 1, after its ReLU
            auto first_tile = [&](int t) {
                f32x16 acc = bias_tile(0, t, hl);
                if (row_bias) {
                    if (live) {
                        const float4 *rb = reinterpret_cast<const float4 *>(row_bias + p * wfirst + 32 * t + 4 * h);
#pragma unroll
                        for (int g = 0; g < 4; ++g) {
                            const float4 v = rb[2 * g];
                            acc[4 * g + 0] += v.x; acc[4 * g + 1] += v.y; acc[4 * g + 2] += v.z; acc[4 * g + 3] += v.w;
                        }
                    }
                }
                if (a.use_xyz) {
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(small[(t * 2 + 0) * 64 + ll], in0, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(small[(t * 2 + 1) * 64 + ll], in1, acc, 0, 0, 0);
                }
                if (a.ks[0]) acc = gm_tile_dyn<KMAX>(wimg + a.woff[0] + (size_t)t * a.ks[0] * 3 * 64 + ll, xs0, a.ks[0], acc);
                return relu_tile(acc);
            };
            // output tile t of layer l >= 1 from the previous layer's split activations
            auto next_tile = [&](int l, int t, const McpSplit3 *xs) {
                f32x16 acc = bias_tile(l, t, hl);
                acc = gm_tile_dyn<KMAX>(wimg + a.woff[l] + (size_t)t * a.ks[l] * 3 * 64 + ll, xs, a.ks[l], acc);
                return relu_tile(acc);
            };
            // pool of one tile of the last layer over each column group, and the store of the groups' rows
            auto pool_tile = [&](int t, f32x16 acc) {
                if (a.pool) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        float v = valid ? acc[r] : 0.f;
                        v += __uint_as_float(mcp_dpp<0xB1>(__float_as_uint(v)));    // quad_perm [1,0,3,2]
                        v += __uint_as_float(mcp_dpp<0x4E>(__float_as_uint(v)));    // quad_perm [2,3,0,1]
                        v += __uint_as_float(mcp_dpp<0x141>(__float_as_uint(v)));   // row_half_mirror: the other quad of the 8
                        if (a.logp >= 4) v += __uint_as_float(mcp_dpp<0x140>(__float_as_uint(v)));  // row_mirror: the other 8 of the row
                        if (a.logp == 5) v += __shfl_xor(v, 16);
                        acc[r] = v;
                    }
                } else {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        float v = acc[r];
                        v = fmaxf(v, __uint_as_float(mcp_dpp<0xB1>(__float_as_uint(v))));
                        v = fmaxf(v, __uint_as_float(mcp_dpp<0x4E>(__float_as_uint(v))));
                        v = fmaxf(v, __uint_as_float(mcp_dpp<0x141>(__float_as_uint(v))));
                        if (a.logp >= 4) v = fmaxf(v, __uint_as_float(mcp_dpp<0x140>(__float_as_uint(v))));
                        if (a.logp == 5) v = fmaxf(v, __shfl_xor(v, 16));
                        acc[r] = v;
                    }
                }
                if (slot == 0 && inr) {
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int ch = 32 * t + 8 * g + 4 * h;
                        float4 o = make_float4(acc[4 * g + 0], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]);
                        if (a.ctiles == 2) {  // the running pool of a centre's two tiles
                            float4 *pr = reinterpret_cast<float4 *>(prow + ch);
                            if (ct == 0) { *pr = o; continue; }
                            const float4 q = *pr;
                            if (a.pool) { o.x = q.x + o.x; o.y = q.y + o.y; o.z = q.z + o.z; o.w = q.w + o.w; }
                            else { o.x = fmaxf(q.x, o.x); o.y = fmaxf(q.y, o.y); o.z = fmaxf(q.z, o.z); o.w = fmaxf(q.w, o.w); }
                        }
                        if (a.pool) { o.x = o.x / fn; o.y = o.y / fn; o.z = o.z / fn; o.w = o.w / fn; }
                        if (!live) o = make_float4(0.f, 0.f, 0.f, 0.f);
                        *reinterpret_cast<float4 *>(out + p * wlast + ch) = o;
                    }
                }
            };

            if (a.layers == 1) {
#pragma unroll 1
                for (int t = 0; t < a.tiles[0]; ++t) pool_tile(t, first_tile(t));
            } else {
                McpSplit3 xa[KMAX];
#pragma unroll
                for (int t = 0; t < HT; ++t) {
                    if (t < a.tiles[0]) {
                        const f32x16 acc = first_tile(t);
                        xa[2 * t + 0] = mcp_split_kstep(acc, 0);
                        xa[2 * t + 1] = mcp_split_kstep(acc, 1);
                    }
                }
                if (a.layers == 2) {
#pragma unroll 1
                    for (int t = 0; t < a.tiles[1]; ++t) pool_tile(t, next_tile(1, t, xa));
                } else {
                    McpSplit3 xb[KMAX];
#pragma unroll
                    for (int t = 0; t < HT; ++t) {
                        if (t < a.tiles[1]) {
                            const f32x16 acc = next_tile(1, t, xa);
                            xb[2 * t + 0] = mcp_split_kstep(acc, 0);
                            xb[2 * t + 1] = mcp_split_kstep(acc, 1);
                        }
                    }
#pragma unroll 1
                    for (int t = 0; t < a.tiles[2]; ++t) pool_tile(t, next_tile(2, t, xb));
                }
            }
        }
    }
}

template <int KMAX, bool LDSW>
int launch_group_mlp(const GmArgs &a, const float *xyz, const float *new_xyz, const float *features, const int *idx, const int *qlen,
                     const float *row_bias, const float *packed, float *out, hipStream_t s) {
    auto kern = group_mlp_kernel<KMAX, LDSW>;
    static McpPerDeviceOnce attr_once;
    if (attr_once.need()) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return (int)e;
        attr_once.done();
    }
    const size_t lds = (size_t)(a.small_floats + WAVES * POOL_ROW) * sizeof(float) + (LDSW ? (size_t)a.w_u4 * 16 : 0);
    const int G = 32 >> a.logp;
    const long long units = (a.total + G - 1) / G;
    // persistent grid: the resident slots (256 CUs x 2 or 1 workgroups, see __launch_bounds__)
    const long long want = (units + WAVES - 1) / WAVES, cap = KMAX == 4 ? 512 : 256;
    const unsigned grid = (unsigned)max(1LL, min(want, cap));
    hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * WAVES), lds, s, a, xyz, new_xyz, features, idx, qlen, row_bias, packed, out);
    return mcp_launch_status();
}

}  // namespace

MCP_EXPORT int mcp_group_mlp_packed_floats(int c, int layers, const int *widths) {
    GmShape sh;
    if (!gm_shape(c, layers, widths, &sh)) return 0;
    return sh.w_u4 * 4 + sh.small_floats;
}

MCP_EXPORT int mcp_group_mlp_pack(int c, int use_xyz, int layers, const int *widths, const float *const *w, const float *const *b, float *packed,
                                  mcp_stream_t stream) {
    MCP_CHECK_ARGS(widths && w && b && packed);
    GmShape sh;
    if (!gm_shape(c, layers, widths, &sh) || (c == 0 && !use_xyz)) return MCP_ERR_UNSUPPORTED;
    for (int l = 0; l < layers; ++l) MCP_CHECK_ARGS(w[l] && b[l]);
    if (((uintptr_t)packed) & 15) return MCP_ERR_BAD_ARG;
    hipStream_t s = (hipStream_t)stream;
    uint4 *pw = reinterpret_cast<uint4 *>(packed);
    float *small = packed + (size_t)sh.w_u4 * 4;
    for (int l = 0; l < layers; ++l) {
        const int col0 = (l == 0 && use_xyz) ? 3 : 0;
        const int cvalid = l == 0 ? c : widths[l - 1], ld = col0 + cvalid;
        const int work = max(sh.tiles[l] * sh.ks[l] * 64, sh.tiles[l] * 128);
        hipLaunchKernelGGL(group_mlp_pack_kernel, dim3((work + 255) / 256), dim3(256), 0, s, w[l], b[l], ld, col0, cvalid, sh.ks[l], sh.tiles[l], use_xyz,
                           pw + sh.woff[l], l == 0 ? small : nullptr, small + sh.boff[l]);
        const int rc = mcp_launch_status();
        if (rc != MCP_OK) return rc;
    }
    return MCP_OK;
}

MCP_EXPORT int mcp_group_mlp(int b, int n, int m, int c, int nsample, int use_xyz, int pool, int layers, const int *widths, const float *xyz,
                             const float *new_xyz, const float *features, const int *idx, const int *qlen, const float *row_bias, const float *packed,
                             float *out, mcp_stream_t stream) {
    MCP_CHECK_ARGS(b > 0 && n > 0 && m > 0 && widths && idx && packed && out && (pool == 0 || pool == 1));
    MCP_CHECK_ARGS((!use_xyz || (xyz && new_xyz)) && (c <= 0 || features));
    GmShape sh;
    if (!gm_shape(c, layers, widths, &sh) || nsample < 1 || nsample > 64 || (c == 0 && !use_xyz)) return MCP_ERR_UNSUPPORTED;
    if ((((uintptr_t)features) | ((uintptr_t)row_bias) | ((uintptr_t)out) | ((uintptr_t)packed)) & 15) return MCP_ERR_BAD_ARG;
    GmArgs a;
    a.total = (long long)b * m;
    a.n = n; a.m = m; a.c = c; a.nsample = nsample; a.use_xyz = use_xyz ? 1 : 0; a.pool = pool; a.layers = layers;
    a.logp = nsample <= 8 ? 3 : nsample <= 16 ? 4 : 5;
    a.ctiles = nsample > 32 ? 2 : 1;
    for (int l = 0; l < MAX_LAYERS; ++l) { a.ks[l] = sh.ks[l]; a.tiles[l] = sh.tiles[l]; a.woff[l] = sh.woff[l]; a.boff[l] = sh.boff[l]; }
    a.w_u4 = sh.w_u4;
    a.small_floats = sh.small_floats;
    hipStream_t s = (hipStream_t)stream;
    const bool in_lds = gm_weights_in_lds(sh);
    if (sh.kmax == 4)
        return in_lds ? launch_group_mlp<4, true>(a, xyz, new_xyz, features, idx, qlen, row_bias, packed, out, s)
                      : launch_group_mlp<4, false>(a, xyz, new_xyz, features, idx, qlen, row_bias, packed, out, s);
    return in_lds ? launch_group_mlp<8, true>(a, xyz, new_xyz, features, idx, qlen, row_bias, packed, out, s)
                  : launch_group_mlp<8, false>(a, xyz, new_xyz, features, idx, qlen, row_bias, packed, out, s);
}
