// group_mlp_grad.hip -- backward of the fused set-abstraction layer (mcp_group_mlp, group_mlp.hip) for gfx950.
//
// The layer, for a live centre p, slots j < nsample, k_j = idx[p, j]:
//     x_j = [xyz[k_j] - new_xyz[p] (use_xyz) | features[k_j]],  z_(l,j) = W_l h_(l-1,j) + b_l (+ row_bias[p] for l = 1),  h_(l,j) = ReLU(z_(l,j)),
//     h_(0,j) = x_j,  out[p] = max_j h_(L,j)  or  (sum_j h_(L,j)) / nsample.
// Given g = dL/dout (B, M, C_out):
//     max:   gy_j[ch] = g[p, ch] for the LOWEST j < nsample with h_(L,j)[ch] == out[p, ch], 0 for every other slot (F.max_pool2d's rule);
//     mean:  gy_j = g[p] / nsample for every j < nsample;
//     gz_L = gy . [h_L > 0],  gz_l = (W_(l+1)^T gz_(l+1)) . [h_l > 0],  dx_j = W_1^T gz_(1,j),
//     grad_features[k_j] += dx_j[3:],  grad_xyz[k_j] += dx_j[:3],  grad_new_xyz[p] = -sum_j dx_j[:3],  grad_row_bias[p] = sum_j gz_(1,j),
//     dW_l = sum_pairs gz_l h_(l-1)^T,  db_l = sum_pairs gz_l   (dW_1 covers the position columns when use_xyz).
//
// Contract (mcp_group_mlp_grad).  Shapes, use_xyz, pool, row_bias, qlen and the supported set are mcp_group_mlp's (gm_shape is not
// narrowed: the kernel has ONE register class, see below).  In addition:
//   * idx gets no gradient; a pooled value of 0 sends nothing (the ReLU mask removes it);
//   * the columns of a group beyond nsample, which repeat slot 0 in the forward, take part in no sum here;
//   * a padded centre (at or beyond qlen[bb]) has none of its float inputs read, grad_out included; it writes zeros to its rows of
//     grad_new_xyz, grad_row_bias and to its pair rows of dx, and adds nothing anywhere else (its gz rows are exact zeros).  Its row
//     of idx must be readable: the caller's mcp_scatter_segments and the scatter walk every position;
//   * rows of features / xyz that no slot gathers get exact zeros (the scatter writes every row);
//   * no atomics: the scatters are mcp_group_rows_grad_sorted over the caller's (order, seg) = mcp_scatter_segments of idx viewed as
//     (B, M nsample) with n = N, the weight sums are mcp_linear_wgrad's fixed-order partial sums.  Two calls give identical bits;
//   * every output may be NULL and is then not computed (grad_w / grad_b: the arrays are required, as in mcp_fp_mlp_grad);
//   * the optional `out` is the forward's result again, bit for bit: every output tile of the recompute receives the forward's
//     sequence of matrix instructions on the forward's own image -- the head of a layer-1 tile (bias, row bias, the two K = 4
//     position products) is gm_layer1_head of group_mlp_tile.h, the one function both kernels call, then the k-steps in ascending
//     order with mcp_mfma_split's six-product order --, the pool is gm_group_sum / gm_group_max of the same header, which the
//     forward calls too, and ReLU as a selection has the bits of fmaxf for every finite value;
//   * no allocation, no environment variable, no host read of a length; the caller owns the workspace
//     (mcp_group_mlp_grad_workspace_bytes) and the operand image (mcp_group_mlp_grad_pack, mcp_group_mlp_grad_packed_floats floats).
//
// One kernel does the per-pair part in the forward's tiling: neighbours on the MFMA column, a centre takes a group of P = 8, 16 or
// 32 columns, a wave owns a unit of 32 / P centres (one centre and two column tiles when nsample > 32), persistent loop over the
// units dealt by XCD.  It keeps the one-bank lesson of fp_mlp_grad to its end: ONE accumulator tile is live.  The workspace has to
// receive x, every hidden h_l, every gz_l and dx anyway (the weight sums and the scatters read them), so every finished 32-channel
// tile is written to its pair row at once, and the next product reads its k-steps back from that row -- k-step s of an
// accumulator-layout row is the two quads at 16 s and 16 s + 8, written by this very lane, so no barrier lies between the store and
// the read; the next k-step's quads are in flight while this one is multiplied.  The price is that a k-step is split into its bf16
// pieces once per output tile instead of once; the gain is one register class for every supported shape (eight waves per workgroup,
// two per SIMD) and no scratch.
//   Phase 1 is the forward, tile by tile; x and the h_l go to the workspace, h_L into the slot of gz_L.
//   Phase 2, per 32-channel tile of the last layer: h_L of the centre's one or two column tiles is read back, pooled with the
//   butterfly of group_mlp_tile.h (the optional `out` is written here), and the winner slot of a channel is the minimum, over the group and
//   over both tiles, of "j where h_(L,j) == pooled, else 64" -- so the two tiles of nsample > 32 agree through this FIRST POOLING
//   PASS over recomputed values, the forward's `out` is not read.  gz_L replaces h_L in place.  Then, layer by layer, the k-steps of
//   gz_l meet the image of W_l^T, the product is selected by [h_(l-1) > 0] with h_(l-1) read back from the workspace (no mask lives in
//   a register) and written as gz_(l-1); dx = W_1^T gz_1 is produced tile by tile the same way.  Sums over a group (grad_row_bias,
//   grad_new_xyz) are the same butterfly, the two tiles of nsample > 32 added in order.
// The workspace is the dense per-pair intermediate that the forward avoids: 4 (ldx + 2 sum(widths) - widths[L-1] + c + 3) bytes per
// (centre, slot) pair.  An in-kernel accumulation of the weight gradients would remove it; that is not done here.
//
// Image (mcp_group_mlp_grad_pack): [mcp_group_mlp_pack's image: forward pieces | position columns, biases] [transposed pieces], the
// latter in mcp_split_weights_transposed's operand layout ([output tile][k-step][piece][lane] x 16 B): for l = L .. 2 the k-steps of
// gz_l (two per tile) with the tiles of layer l - 1 as outputs, then the k-steps of gz_1 with the tiles of dx as outputs.  dx is laid
// out [features (c) | position (3)], so that every feature quad of a pair row is 16-byte aligned; rows of W_1^T beyond c + 3 are
// zeros.  gg_weights_in_lds(c, use_xyz, widths) is the one staging predicate: when the two parts together are at most 128 KB both are
// staged in LDS once per workgroup; otherwise both are read through L2.
//
// Built WITHOUT -fno-honor-nans: the masks and the ReLU are comparisons and selections, and a training kernel should not be compiled
// under the assumption that no NaN arrives (a diverged run must show its NaN, not hide it).
//
// The column's centre, the position operand, the head of a layer-1 tile, the butterflies, the pack kernels, the launch, the
// workspace's parts and the tail of the entry point are group_mlp_tile.h's, shared with group_mlp.hip and group_mlp_bn.hip.
#include "group_mlp_tile.h"

namespace {

constexpr int WAVES = 8;
constexpr int THREADS = 64 * WAVES;
constexpr int GRAD_LDS_IMAGE_BYTES = 128 * 1024;      // largest (forward + transposed) image staged in LDS
constexpr int MAX_GRID = 256;                         // persistent grid: one workgroup per CU

struct GgShape {
    GmShape f;
    int boff[MAX_LAYERS];// uint4 offset, inside the transposed part, of the pieces that take gz_l (l = 0: into dx, else into layer l - 1)
    int bwd_u4;
};

inline bool gg_shape(int c, int use_xyz, int layers, const int *widths, GgShape *s) {
    if (!gm_shape(c, use_xyz, layers, widths, &s->f)) return false;
    int u4 = 0;
    for (int l = 0; l < MAX_LAYERS; ++l) s->boff[l] = 0;
    for (int l = layers - 1; l >= 1; --l) {
        s->boff[l] = u4;
        u4 += s->f.tiles[l - 1] * 2 * s->f.tiles[l] * TILE_U4;
    }
    s->boff[0] = u4;
    u4 += s->f.x.dxt * 2 * s->f.tiles[0] * TILE_U4;
    s->bwd_u4 = u4;
    return true;
}
// the staging predicate, a function of (c, use_xyz, widths) alone (ops.group_mlp_grad_weights_in_lds mirrors it)
inline bool gg_weights_in_lds(const GgShape &s) { return ((size_t)s.f.w_u4 + s.bwd_u4) * 16 <= (size_t)GRAD_LDS_IMAGE_BYTES; }
inline size_t gg_image_floats(const GgShape &s) { return ((size_t)s.f.w_u4 + s.bwd_u4) * 4 + s.f.small_floats; }

struct GgArgs {
    long long total;  // B * M centres
    int n, m, c, nsample, use_xyz, pool, layers;
    int logp, ctiles;
    int ks0;                                    // feature k-steps of layer 1 in the forward image
    int tiles[MAX_LAYERS], woff[MAX_LAYERS], bias[MAX_LAYERS], boff[MAX_LAYERS];
    int tlast;                                  // tiles[layers - 1]: no array of the arguments is indexed with a run-time value
    int w_u4, small_floats, bwd_u4, dxt, ldx, want_dx;
};
struct GgIn {
    const float *xyz, *new_xyz, *features, *row_bias, *packed, *grad_out;
    const int *idx, *qlen;
};
struct GgOut {
    float *x, *hid[2], *gz[MAX_LAYERS], *gzl, *dxf, *dxp, *grad_new_xyz, *grad_row_bias, *out;   // gzl = gz[layers - 1]
};

template <bool LDSW>
__global__ __launch_bounds__(THREADS, 1) void group_mlp_grad_kernel(const GgArgs a, const GgIn in, const GgOut o) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *small = lds;                                                   // position columns | biases
    uint4 *wlds = reinterpret_cast<uint4 *>(lds + a.small_floats);        // forward pieces | transposed pieces
    const int tid = threadIdx.x;
    const uint4 *gimg = reinterpret_cast<const uint4 *>(in.packed);
    const int small_u4 = a.small_floats / 4;
    {
        const float4 *src = reinterpret_cast<const float4 *>(in.packed) + a.w_u4;
        for (int e = tid; e < small_u4; e += THREADS) reinterpret_cast<float4 *>(small)[e] = src[e];
        if (LDSW) {
            for (int e = tid; e < a.w_u4; e += THREADS) wlds[e] = gimg[e];
            for (int e = tid; e < a.bwd_u4; e += THREADS) wlds[a.w_u4 + e] = gimg[a.w_u4 + small_u4 + e];
        }
    }
    __syncthreads();
    const uint4 *wfwd = LDSW ? wlds : gimg;
    const uint4 *wbwd = LDSW ? wlds + a.w_u4 : gimg + a.w_u4 + small_u4;

    const int lane = tid & 63, wave = tid >> 6, h = lane >> 5, col = lane & 31;
    const int P = 1 << a.logp, G = 32 >> a.logp, slot = col & (P - 1);
    const int L = a.layers;
    const int wfirst = a.tiles[0] * 32, wlast = a.tlast * 32;
    const float fn = (float)a.nsample;

    // the two quads of k-step s of a row (`row` points at channel 4 h of it); quads at or beyond `lim` channels, and every quad of a
    // column that is not `ok`, are zeros and are not loaded
    auto load_kstep = [&](const float *row, int s, bool ok, int lim, float4 &q0, float4 &q1) {
        q0 = make_float4(0.f, 0.f, 0.f, 0.f); q1 = q0;
        const int ch = 16 * s + 4 * h;
        if (ok && ch < lim) q0 = *reinterpret_cast<const float4 *>(row + 16 * s);
        if (ok && ch + 8 < lim) q1 = *reinterpret_cast<const float4 *>(row + 16 * s + 8);
    };
    // acc += sum_s W(s) . row(s) over ks k-steps; w points at this lane's entry of (k-step 0, piece 1) of the output tile
    auto tile_from_row = [&](f32x16 acc, const uint4 *w, const float *row, int ks, bool ok, int lim) {
        float4 n0, n1;
        load_kstep(row, 0, ok, lim, n0, n1);
#pragma unroll 1
        for (int s = 0; s < ks; ++s) {
            float4 m0, m1;
            load_kstep(row, min(s + 1, ks - 1), ok, lim, m0, m1);   // the last k-step fetches itself again: no branch in the loop body
            const float v[8] = {n0.x, n0.y, n0.z, n0.w, n1.x, n1.y, n1.z, n1.w};
            acc = mcp_mfma_split(w + (size_t)s * TILE_U4, mcp_split8(v), acc);
            n0 = m0; n1 = m1;
        }
        return acc;
    };
    auto zero_tile = [&]() {
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        return acc;
    };
    // Rows in accumulator order: register 4 g + i of tile t is channel 32 t + 8 g + 4 h + i (`row` points at channel 4 h).
    auto store_tile = [&](float *row, int t, const f32x16 &v) {
#pragma unroll
        for (int g = 0; g < 4; ++g) *reinterpret_cast<float4 *>(row + 32 * t + 8 * g) = make_float4(v[4 * g + 0], v[4 * g + 1], v[4 * g + 2], v[4 * g + 3]);
    };
    auto load_tile = [&](const float *row, int t, bool ok) {
        f32x16 v;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
            if (ok) q = *reinterpret_cast<const float4 *>(row + 32 * t + 8 * g);
            v[4 * g + 0] = q.x; v[4 * g + 1] = q.y; v[4 * g + 2] = q.z; v[4 * g + 3] = q.w;
        }
        return v;
    };

    const long long units = (a.total + G - 1) / G;
    const McpUnits deal = mcp_units_by_xcd(units, WAVES);
    for (long long unit = deal.first + wave; unit < deal.limit; unit += deal.stride) {
        const GmCentre me(unit, col, a.logp, a.total, a.m, in.qlen);   // this column's centre
        const long long p = me.p, bb = me.bb;
        const bool inr = me.inr, live = me.live;
        // the pair row of this column in column tile ct; a column at or beyond nsample owns none
        auto pair_row = [&](int ct, bool &valid) {
            const int j = ct * 32 + slot;
            valid = inr && j < a.nsample;
            long long q = valid ? p * a.nsample + j : 0;
            asm volatile("" : "+v"(q));   // addresses are formed where they are used, not hoisted out of the loops
            return q;
        };

        // ---- phase 1: the forward, tile by tile ----
        for (int ct = 0; ct < a.ctiles; ++ct) {
            bool valid;
            const long long pr = pair_row(ct, valid);
            const int j = ct * 32 + slot;
            const int k = live ? in.idx[p * a.nsample + (j < a.nsample ? j : 0)] : 0;
            const long long src = bb * a.n + k;
            const GmPos pos = gm_position(in.xyz + src * 3, in.new_xyz + p * 3, live && a.use_xyz, h);
            if (a.use_xyz && valid && h == 0) *reinterpret_cast<float4 *>(o.x + pr * a.ldx + a.c) = make_float4(pos.dx, pos.dy, pos.dz, 0.f);
            const float *frow = in.features + src * a.c + 4 * h;   // formed, not read, when c = 0 or the centre is padded
            if (valid) {   // the feature part of x
                float *xr = o.x + pr * a.ldx + 4 * h;
                for (int ch = 0; ch + 4 * h < a.c; ch += 8) {
                    float4 f = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (live) f = *reinterpret_cast<const float4 *>(frow + ch);
                    *reinterpret_cast<float4 *>(xr + ch) = f;
                }
            }
            // layer 1
            float *h1row = (L == 1 ? o.gz[0] : o.hid[0]) + pr * wfirst + 4 * h;
#pragma unroll 1
            for (int t = 0; t < a.tiles[0]; ++t) {
                f32x16 acc = gm_layer1_head(small, a.bias[0], t, h, lane, in.row_bias, p, wfirst, live, a.use_xyz, pos);
                if (a.ks0) {
                    acc = tile_from_row(acc, wfwd + a.woff[0] + (size_t)t * a.ks0 * TILE_U4 + lane, frow, a.ks0, live, a.c);
                } else {
                    // c = 0: the ReLU reads the K = 4 position product itself.  Behind this wave-uniform branch the compiler left 13-17
                    // wait states between that 16-pass MFMA and the first v_max where 18 are needed (tools/isa_lint.py): 18 idle slots here.
                    __builtin_amdgcn_sched_barrier(0);
                    asm volatile("s_nop 15\n\ts_nop 1");
                    __builtin_amdgcn_sched_barrier(0);
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] = acc[r] > 0.f ? acc[r] : 0.f;
                if (valid) store_tile(h1row, t, acc);
            }
            // layers 2 .. L from the rows just written; h_L goes into the slot of gz_L
#pragma unroll
            for (int l = 1; l < MAX_LAYERS; ++l) {
                if (l >= L) break;
                const int win = a.tiles[l - 1] * 32, wout = a.tiles[l] * 32;
                const float *hin = o.hid[l - 1] + pr * win + 4 * h;
                float *hout = (l == 1 && L > 2 ? o.hid[1] : o.gz[l]) + pr * wout + 4 * h;
#pragma unroll 1
                for (int t = 0; t < a.tiles[l]; ++t) {
                    f32x16 acc = gm_bias_tile(small + a.bias[l], t, h);
                    acc = tile_from_row(acc, wfwd + a.woff[l] + (size_t)t * (2 * a.tiles[l - 1]) * TILE_U4 + lane, hin, 2 * a.tiles[l - 1], valid, win);
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[r] = acc[r] > 0.f ? acc[r] : 0.f;
                    if (valid) store_tile(hout, t, acc);
                }
            }
        }

        bool valid0, valid1 = false;
        const long long pr0 = pair_row(0, valid0);
        long long pr1 = 0;
        if (a.ctiles == 2) pr1 = pair_row(1, valid1);
        const bool head = inr && slot == 0;   // the lane that writes the centre's rows

        // ---- phase 2: pool, winner, gz_L in place of h_L ----
        {
            float *g0row = o.gzl + pr0 * wlast + 4 * h, *g1row = o.gzl + pr1 * wlast + 4 * h;
#pragma unroll 1
            for (int t = 0; t < a.tlast; ++t) {
                const f32x16 ha = load_tile(g0row, t, valid0), hb = load_tile(g1row, t, valid1);
                f32x16 gv = zero_tile();
                if (live) gv = load_tile(in.grad_out + p * wlast + 4 * h, t, true);
                f32x16 ga, gb, pooled;
                if (a.pool) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        float s = gm_group_sum(ha[r], a.logp);   // a column beyond nsample holds 0
                        if (a.ctiles == 2) s = s + gm_group_sum(hb[r], a.logp);
                        pooled[r] = s / fn;
                        const float gy = gv[r] / fn;
                        ga[r] = (valid0 && ha[r] > 0.f) ? gy : 0.f;
                        gb[r] = (valid1 && hb[r] > 0.f) ? gy : 0.f;
                    }
                } else {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        float mx = gm_group_max(ha[r], a.logp);  // h >= 0: the zeros of the columns beyond nsample change no maximum
                        if (a.ctiles == 2) mx = fmaxf(mx, gm_group_max(hb[r], a.logp));
                        pooled[r] = mx;
                        int win = gm_group_min((valid0 && ha[r] == mx) ? slot : 64, a.logp);
                        if (a.ctiles == 2) win = min(win, gm_group_min((valid1 && hb[r] == mx) ? 32 + slot : 64, a.logp));
                        ga[r] = (valid0 && slot == win && ha[r] > 0.f) ? gv[r] : 0.f;
                        gb[r] = (valid1 && 32 + slot == win && hb[r] > 0.f) ? gv[r] : 0.f;
                    }
                }
                if (valid0) store_tile(g0row, t, ga);
                if (valid1) store_tile(g1row, t, gb);
                if (o.out && head) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) pooled[r] = live ? pooled[r] : 0.f;
                    store_tile(o.out + p * wlast + 4 * h, t, pooled);
                }
                if (L == 1 && o.grad_row_bias) {
                    f32x16 sum;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        float s = gm_group_sum(ga[r], a.logp);
                        if (a.ctiles == 2) s = s + gm_group_sum(gb[r], a.logp);
                        sum[r] = s;
                    }
                    if (head) store_tile(o.grad_row_bias + p * wfirst + 4 * h, t, sum);
                }
            }
        }

        // ---- gz_(l-1) = (W_l^T gz_l) . [h_(l-1) > 0] ----
#pragma unroll
        for (int l = MAX_LAYERS - 1; l >= 1; --l) {
            if (l >= L) continue;
            const int win = a.tiles[l] * 32, wout = a.tiles[l - 1] * 32, ks = 2 * a.tiles[l];
#pragma unroll 1
            for (int t = 0; t < a.tiles[l - 1]; ++t) {
                f32x16 sum = zero_tile();
                for (int ct = 0; ct < a.ctiles; ++ct) {
                    const bool valid = ct ? valid1 : valid0;
                    const long long pr = ct ? pr1 : pr0;
                    f32x16 acc = tile_from_row(zero_tile(), wbwd + a.boff[l] + (size_t)t * ks * TILE_U4 + lane, o.gz[l] + pr * win + 4 * h, ks, valid, win);
                    const f32x16 hv = load_tile(o.hid[l - 1] + pr * wout + 4 * h, t, valid);
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[r] = hv[r] > 0.f ? acc[r] : 0.f;   // a column beyond nsample: hv = 0
                    if (valid) store_tile(o.gz[l - 1] + pr * wout + 4 * h, t, acc);
                    if (l == 1 && o.grad_row_bias) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const float s = gm_group_sum(acc[r], a.logp);
                            sum[r] = ct ? sum[r] + s : s;
                        }
                    }
                }
                if (l == 1 && o.grad_row_bias && head) store_tile(o.grad_row_bias + p * wfirst + 4 * h, t, sum);
            }
        }

        // ---- dx = W_1^T gz_1, laid out [features | position] ----
        if (a.want_dx) {
            const int ks = 2 * a.tiles[0];
#pragma unroll 1
            for (int t = 0; t < a.dxt; ++t) {
                float sx = 0.f, sy = 0.f, sz = 0.f;
                const bool pos_tile = a.use_xyz && t == (a.c >> 5);   // the tile that holds channels c .. c + 2
                for (int ct = 0; ct < a.ctiles; ++ct) {
                    const bool valid = ct ? valid1 : valid0;
                    const long long pr = ct ? pr1 : pr0;
                    const f32x16 acc = tile_from_row(zero_tile(), wbwd + a.boff[0] + (size_t)t * ks * TILE_U4 + lane, o.gz[0] + pr * wfirst + 4 * h, ks, valid, wfirst);
                    float px = 0.f, py = 0.f, pz = 0.f;
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int ch = 32 * t + 8 * g + 4 * h;
                        if (ch < a.c) {   // c is a multiple of 4: a quad lies on one side
                            if (valid) *reinterpret_cast<float4 *>(o.dxf + pr * a.c + ch) = make_float4(acc[4 * g + 0], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]);
                        } else if (ch == a.c) {
                            px = acc[4 * g + 0]; py = acc[4 * g + 1]; pz = acc[4 * g + 2];
                        }
                    }
                    if (pos_tile) {
                        const bool mine = valid && 4 * h == (a.c & 4);   // the lane half that holds the position quad
                        px = mine ? px : 0.f; py = mine ? py : 0.f; pz = mine ? pz : 0.f;
                        if (mine) {
                            float *d = o.dxp + pr * 3;
                            d[0] = px; d[1] = py; d[2] = pz;
                        }
                        if (o.grad_new_xyz) {
                            const float tx = gm_group_sum(px, a.logp), ty = gm_group_sum(py, a.logp), tz = gm_group_sum(pz, a.logp);
                            sx = ct ? sx + tx : tx; sy = ct ? sy + ty : ty; sz = ct ? sz + tz : tz;
                        }
                    }
                }
                if (pos_tile && o.grad_new_xyz && head && 4 * h == (a.c & 4)) {
                    float *d = o.grad_new_xyz + p * 3;
                    d[0] = 0.f - sx; d[1] = 0.f - sy; d[2] = 0.f - sz;
                }
            }
        }
    }
}

}  // namespace

MCP_EXPORT int mcp_group_mlp_grad_packed_floats(int c, int use_xyz, int layers, const int *widths) {
    GgShape sh;
    if (!gg_shape(c, use_xyz, layers, widths, &sh)) return 0;
    return (int)gg_image_floats(sh);
}

MCP_EXPORT int mcp_group_mlp_grad_pack(int c, int use_xyz, int layers, const int *widths, const float *const *w, const float *const *b, float *packed,
                                       mcp_stream_t stream) {
    MCP_CHECK_ARGS(widths && w && b && packed);
    GgShape sh;
    if (!gg_shape(c, use_xyz, layers, widths, &sh)) return MCP_ERR_UNSUPPORTED;
    int rc = mcp_group_mlp_pack(c, use_xyz, layers, widths, w, b, packed, stream);   // [forward pieces | position columns, biases]
    if (rc != MCP_OK) return rc;
    const GmShape &f = sh.f;
    hipStream_t s = (hipStream_t)stream;
    uint4 *pw = reinterpret_cast<uint4 *>(packed + (size_t)f.w_u4 * 4 + f.small_floats);   // the transposed pieces in the order of boff, entries [t][s]
    for (int l = layers - 1; l >= 1; --l)
        if ((rc = gm_pack_bwd(s, w[l], widths[l - 1], widths[l - 1], 0, 0, f.tiles[l - 1], 2 * f.tiles[l], 2 * f.tiles[l], 1, pw)) != MCP_OK) return rc;
    return gm_pack_bwd(s, w[0], f.x.cin, c, f.x.px, 0, f.x.dxt, 2 * f.tiles[0], 2 * f.tiles[0], 1, pw);
}

MCP_EXPORT size_t mcp_group_mlp_grad_workspace_bytes(int b, int m, int c, int nsample, int use_xyz, int layers, const int *widths) {
    GgShape sh;
    if (b <= 0 || m <= 0 || nsample < 1 || nsample > 64 || !gg_shape(c, use_xyz, layers, widths, &sh)) return 0;
    FpTake take;
    GmBack lay;
    return gm_back_layout(take, (long long)b * m * nsample, sh.f.x, layers, widths, &lay) ? take.at : 0;
}

MCP_EXPORT int mcp_group_mlp_grad(int b, int n, int m, int c, int nsample, int use_xyz, int pool, int layers, const int *widths, const float *xyz,
                                  const float *new_xyz, const float *features, const int *idx, const int *qlen, const float *row_bias,
                                  const float *packed, const float *grad_out, const int *order, const int *seg, float *grad_features, float *grad_xyz,
                                  float *grad_new_xyz, float *grad_row_bias, float *const *grad_w, float *const *grad_b, float *out, void *workspace,
                                  size_t workspace_bytes, mcp_stream_t stream) {
    MCP_CHECK_ARGS(b > 0 && n > 0 && m > 0 && widths && idx && packed && grad_out && grad_w && grad_b && workspace && (pool == 0 || pool == 1));
    MCP_CHECK_ARGS((!use_xyz || (xyz && new_xyz)) && (c <= 0 || features) && (!(grad_features || grad_xyz) || (order && seg)));
    MCP_CHECK_ARGS((!grad_row_bias || row_bias) && (!grad_features || c > 0) && (!(grad_xyz || grad_new_xyz) || use_xyz));
    GgShape sh;
    if (!gg_shape(c, use_xyz, layers, widths, &sh) || nsample < 1 || nsample > 64) return MCP_ERR_UNSUPPORTED;
    for (int l = 0; l < layers; ++l) MCP_CHECK_ARGS(grad_w[l] && grad_b[l]);
    const uintptr_t quads = (uintptr_t)features | (uintptr_t)row_bias | (uintptr_t)packed | (uintptr_t)grad_out | (uintptr_t)out |
                            (uintptr_t)grad_row_bias | (uintptr_t)grad_features | (uintptr_t)workspace;
    if (quads & 15) return MCP_ERR_BAD_ARG;
    const long long total = (long long)b * m;
    if ((long long)m * nsample > 0x7FFFFFFFLL) return MCP_ERR_UNSUPPORTED;
    const GmShape &f = sh.f;
    FpTake take;   // the workspace is the backward-only parts and nothing else
    GmBack lay;
    if (!gm_back_layout(take, total * nsample, f.x, layers, widths, &lay)) return MCP_ERR_UNSUPPORTED;
    if (workspace_bytes < take.at) return MCP_ERR_BAD_ARG;
    char *ws = reinterpret_cast<char *>(workspace);
    auto part = [&](size_t off) { return reinterpret_cast<float *>(ws + off); };

    const GmUnits u = gm_units(total, nsample);
    GgArgs a;
    a.total = total;
    a.n = n; a.m = m; a.c = c; a.nsample = nsample; a.use_xyz = use_xyz ? 1 : 0; a.pool = pool; a.layers = layers;
    a.logp = u.logp;
    a.ctiles = u.ctiles;
    a.ks0 = f.ks[0];
    for (int l = 0; l < MAX_LAYERS; ++l) { a.tiles[l] = f.tiles[l]; a.woff[l] = f.woff[l]; a.bias[l] = f.boff[l]; a.boff[l] = sh.boff[l]; }
    a.tlast = f.tiles[layers - 1];
    a.w_u4 = f.w_u4; a.small_floats = f.small_floats; a.bwd_u4 = sh.bwd_u4; a.dxt = f.x.dxt; a.ldx = f.x.ldx;
    a.want_dx = (grad_features || grad_xyz || grad_new_xyz) ? 1 : 0;
    const GgIn in{xyz, new_xyz, features, row_bias, packed, grad_out, idx, qlen};
    const GgOut o{part(lay.x), {part(lay.hid[0]), part(lay.hid[1])}, {part(lay.gz[0]), part(lay.gz[1]), part(lay.gz[2])}, part(lay.gz[layers - 1]),
                  part(lay.dxf), part(lay.dxp), grad_new_xyz, grad_row_bias, out};
    const bool in_lds = gg_weights_in_lds(sh);
    const size_t lds = (size_t)a.small_floats * sizeof(float) + (in_lds ? ((size_t)a.w_u4 + a.bwd_u4) * 16 : 0);
    hipStream_t s = (hipStream_t)stream;
    const int rc = in_lds ? gm_launch<group_mlp_grad_kernel<true>>(u.units, WAVES, MAX_GRID, lds, s, a, in, o)
                          : gm_launch<group_mlp_grad_kernel<false>>(u.units, WAVES, MAX_GRID, lds, s, a, in, o);
    if (rc != MCP_OK) return rc;
    return gm_backward_tail(b, n, m, nsample, f.x, layers, widths, ws, lay, order, seg, grad_features, grad_xyz, grad_w, grad_b, stream);
}
