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
//
// The column's centre, the position operand, the head of a layer-1 tile, the butterflies, the pack kernel and the launch are
// group_mlp_tile.h's, shared with group_mlp_grad.hip and group_mlp_bn.hip.
#include <type_traits>

#include "group_mlp_tile.h"

namespace {

constexpr int WAVES = 4;
constexpr int POOL_ROW = 256;                 // floats of a wave's pooled row (the widest last layer)

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
    const float fn = (float)a.nsample;

    auto relu_tile = [&](f32x16 acc) {
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = fmaxf(acc[r], 0.f);
        return acc;
    };

    const long long units = (a.total + G - 1) / G;
    const McpUnits deal = mcp_units_by_xcd(units, WAVES);
    for (long long unit = deal.first + wave; unit < deal.limit; unit += deal.stride) {
        const GmCentre me(unit, col, a.logp, a.total, a.m, qlen);   // this column's centre
        const long long p = me.p, bb = me.bb;
        const bool inr = me.inr, live = me.live;

        for (int ct = 0; ct < a.ctiles; ++ct) {
            // The lane's offset into the weight image, the position columns and the biases, opaque to the compiler once per tile: every
            // such address and bias value is invariant over the persistent loop, and hoisted out of it they cost hundreds of registers.
            int ll = lane, hl = h;
            asm volatile("" : "+v"(ll), "+v"(hl));
            const int j = ct * 32 + slot;
            const bool valid = j < a.nsample;
            const int k = live ? idx[p * a.nsample + (valid ? j : 0)] : 0;
            const long long row = bb * a.n + k;
            const GmPos pos = gm_position(xyz + row * 3, new_xyz + p * 3, live && a.use_xyz, h);
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
                f32x16 acc = gm_layer1_head(small, a.boff[0], t, hl, ll, row_bias, p, wfirst, live, a.use_xyz, pos);
                if (a.ks[0]) acc = gm_tile_dyn<KMAX>(wimg + a.woff[0] + (size_t)t * a.ks[0] * 3 * 64 + ll, xs0, a.ks[0], acc);
                return relu_tile(acc);
            };
            // output tile t of layer l >= 1 from the previous layer's split activations
            auto next_tile = [&](int l, int t, const McpSplit3 *xs) {
                f32x16 acc = gm_bias_tile(small + a.boff[l], t, hl);
                acc = gm_tile_dyn<KMAX>(wimg + a.woff[l] + (size_t)t * a.ks[l] * 3 * 64 + ll, xs, a.ks[l], acc);
                return relu_tile(acc);
            };
            // pool of one tile of the last layer over each column group, and the store of the groups' rows
            auto pool_tile = [&](int t, f32x16 acc) {
                if (a.pool) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[r] = gm_group_sum(valid ? acc[r] : 0.f, a.logp);
                } else {
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[r] = gm_group_max(acc[r], a.logp);
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

}  // namespace

MCP_EXPORT int mcp_group_mlp_packed_floats(int c, int layers, const int *widths) {
    GmShape sh;
    if (!gm_shape(c, 1, layers, widths, &sh)) return 0;   // the image's size does not depend on use_xyz
    return sh.w_u4 * 4 + sh.small_floats;
}

MCP_EXPORT int mcp_group_mlp_pack(int c, int use_xyz, int layers, const int *widths, const float *const *w, const float *const *b, float *packed,
                                  mcp_stream_t stream) {
    MCP_CHECK_ARGS(widths && w && b && packed);
    GmShape sh;
    if (!gm_shape(c, use_xyz, layers, widths, &sh)) return MCP_ERR_UNSUPPORTED;
    for (int l = 0; l < layers; ++l) MCP_CHECK_ARGS(w[l] && b[l]);
    if (((uintptr_t)packed) & 15) return MCP_ERR_BAD_ARG;
    uint4 *pw = reinterpret_cast<uint4 *>(packed);
    float *small = packed + (size_t)sh.w_u4 * 4;
    for (int l = 0; l < layers; ++l) {   // entries [t][s]; layer 1's position columns go to the small part, not behind the features
        const int col0 = l == 0 ? sh.x.px : 0, cvalid = l == 0 ? c : widths[l - 1];
        const int rc = gm_pack_fwd((hipStream_t)stream, w[l], b[l], col0 + cvalid, col0, cvalid, 0, sh.ks[l], sh.tiles[l], sh.ks[l], 1, pw + sh.woff[l],
                                   l == 0 ? small : nullptr, small + sh.boff[l]);
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
    if (!gm_shape(c, use_xyz, layers, widths, &sh) || nsample < 1 || nsample > 64) return MCP_ERR_UNSUPPORTED;
    if ((((uintptr_t)features) | ((uintptr_t)row_bias) | ((uintptr_t)out) | ((uintptr_t)packed)) & 15) return MCP_ERR_BAD_ARG;
    GmArgs a;
    a.total = (long long)b * m;
    a.n = n; a.m = m; a.c = c; a.nsample = nsample; a.use_xyz = use_xyz ? 1 : 0; a.pool = pool; a.layers = layers;
    const GmUnits u = gm_units(a.total, nsample);
    a.logp = u.logp;
    a.ctiles = u.ctiles;
    for (int l = 0; l < MAX_LAYERS; ++l) { a.ks[l] = sh.ks[l]; a.tiles[l] = sh.tiles[l]; a.woff[l] = sh.woff[l]; a.boff[l] = sh.boff[l]; }
    a.w_u4 = sh.w_u4;
    a.small_floats = sh.small_floats;
    const bool in_lds = gm_weights_in_lds(sh);
    const size_t lds = (size_t)(a.small_floats + WAVES * POOL_ROW) * sizeof(float) + (in_lds ? (size_t)a.w_u4 * 16 : 0);
    // persistent grid: the resident slots (256 CUs x 2 or 1 workgroups, see __launch_bounds__)
    auto go = [&](auto kmax, auto ldsw) {
        constexpr int K = decltype(kmax)::value;
        return gm_launch<group_mlp_kernel<K, decltype(ldsw)::value>>(u.units, WAVES, K == 4 ? 512 : 256, lds, (hipStream_t)stream, a, xyz, new_xyz, features,
                                                                     idx, qlen, row_bias, packed, out);
    };
    using std::integral_constant;
    if (sh.kmax == 4) return in_lds ? go(integral_constant<int, 4>{}, std::true_type{}) : go(integral_constant<int, 4>{}, std::false_type{});
    return in_lds ? go(integral_constant<int, 8>{}, std::true_type{}) : go(integral_constant<int, 8>{}, std::false_type{});
}
