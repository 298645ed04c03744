// fp_mlp_grad.hip -- backward of the fused feature-propagation layer (mcp_fp_mlp, fp_mlp.hip) for gfx950.
//
// The layer, for a live row p:  x = [(w0 f[i0] + w1 f[i1]) + w2 f[i2] | skip],  z_l = W_l h_(l-1) + b_l,  h_l = ReLU(z_l),  h_0 = x,
// out = h_L.  Given g = dL/dout (B, n, C_out):
//     gz_L = g . [out > 0],   gz_(l-1) = (W_l^T gz_l) . [h_(l-1) > 0]  (l = L .. 2),   dx = W_1^T gz_1,
//     grad_skip = dx[C2:],  grad_blend = dx[:C2],  grad_known_feats[i_j] += w_j grad_blend,  dW_l = sum_p gz_l h_(l-1)^T,  db_l = sum_p gz_l.
//
// Contract (mcp_fp_mlp_grad).  Shapes, rules, ulen and infinite slots as the forward's header (fp_mlp.hip).  In addition:
//   * dist, w3 and the coordinates get NO gradient, as in the reference (its ThreeNN and ThreeInterpolate return none for them);
//   * a padded row (at or beyond ulen[bb]) has none of its float inputs read, grad_out included; it writes zeros to grad_skip and adds
//     nothing to grad_known_feats, the weight or the bias gradients (its gz rows are exact zeros).  Its row of idx must be readable:
//     the caller's mcp_scatter_segments and the scatter walk every position of idx (out-of-range values are left out; in-range ones
//     add w_used x grad_blend = 0 x 0);
//   * rows of known_feats that no live slot with a non-zero weight gathers get exactly zero; a slot whose dist is +inf carries the
//     weight exactly 0 (selected, never computed from the infinity);
//   * no atomics: the scatter of the blend is mcp_interp3_apply_grad_sorted over the caller's (order, seg) = mcp_scatter_segments of
//     idx viewed as (B, 3n); the weight sums are mcp_linear_wgrad's fixed-order partial sums.  Two calls give identical bits;
//   * the optional `out` is the forward's result again, bit for bit: the recompute walks the forward's slabs of the same image in the
//     same order with the same six-product split (and ReLU as a selection, which has the bits of fmaxf for every finite value);
//   * no allocation, no environment variable, no host read of a length; the caller owns the workspace
//     (mcp_fp_mlp_grad_workspace_bytes) and the operand image (mcp_fp_mlp_grad_pack, mcp_fp_mlp_grad_packed_floats floats);
//   * supported: everything mcp_fp_mlp supports; anything else MCP_ERR_UNSUPPORTED, nothing launched.
//
// One kernel does the per-row part, in the forward's tiling: a wave owns 32 rows, the MFMA column; four waves per workgroup.  Unlike
// the forward it holds ONE bank of TMAX accumulator tiles.  The workspace has to receive x, every hidden h_l and every gz_l anyway (the
// weight sums read them), so a finished bank is written out tile by tile and the next layer reads its k-steps back: k-step s of an
// accumulator-layout row is the two quads at 16 s and 16 s + 8, which this very lane wrote, so no barrier lies between the store and
// the read.  Every layer is therefore the layer-1 loop again (layer_from_rows): a rolled loop over k-steps, the next k-step's two
// quads in flight while this one is multiplied.
//   Phase 1 is the forward: layer 1 from the gathered rows (x written on the way), then per layer ReLU(bank) -> h_l, biases into the
//   bank, the k-steps of h_l back in.  Same image, same slab order, same six-product split as the forward (fp_mlp.hip).
//   Phase 2: gz_L = g selected by [out > 0] in place of the last bank (the recomputed out written on the way); per layer the bank is
//   zeroed, the k-steps of gz_l are multiplied with the image of W_l^T, and the result is selected by [h_(l-1) > 0] with h_(l-1) read
//   back from the workspace -- no mask is kept in registers -- and written as gz_(l-1).  dx = W_1^T gz_1 has up to 24 output tiles:
//   they are produced in chunks of TMAX tiles in the same bank, each chunk from the k-steps of gz_1 again, and stored chunk by chunk
//   (grad_blend, grad_skip), never held together.
// w_used (B, n, 3) holds the weights the blend used (0 in an infinite slot, three zeros in a padded row).  No scatter and no weight
// sum in this kernel; all tile loops are unrolled, absent tiles are skipped by wave-uniform branches, no register array is indexed
// with a run-time value.
//
// Image (mcp_fp_mlp_grad_pack): [mcp_fp_mlp_pack's image: forward slabs | biases] [backward slabs], every slab in the order it is
// consumed, the backward ones in mcp_split_weights_transposed's operand layout: for l = L .. 2 the k-steps of gz_l (two per tile)
// with the tiles of layer l - 1 as outputs; then, chunk by chunk, the k-steps of gz_1 with that chunk's tiles of dx as outputs (rows
// of W_1^T beyond C2 + C1 are zeros).  fg_whole(shape) is the one staging predicate: when both halves are at most 64 KB each is staged
// whole in LDS for its phase; otherwise the whole sequence is streamed through two LDS slab buffers, one barrier per slab, as in
// the forward.
//
// Built WITHOUT -fno-honor-nans: the masks and the ReLU are comparisons and selections, which need no canonicalisation, and a training
// kernel should not be compiled under the assumption that no NaN arrives (a diverged run must show its NaN, not hide it).
//
// The row, the gather, the slab sequence, the tile helpers and the dx epilogue are fp_mlp_tile.h's, shared with fp_mlp.hip and
// fp_mlp_bn.hip.
#include "fp_mlp_tile.h"

namespace {

inline size_t fg_image_floats(const FgShape &s) { return ((size_t)s.f.w_u4 + s.bwd_u4) * 4 + s.f.small_floats; }

// Slabs of A = W^T for output tiles tile0 .. tile0 + tiles - 1 (32 rows m of A each) over the ks k-steps of W's rows: entry
// ((s * tiles + t) * 3 + piece) * 64 + lane holds the 8 bf16 pieces of A[32 (tile0 + t) + (lane & 31)][k] = w[k * ld + m],
// k = 32 (s >> 1) + chan_of(8 (s & 1) + i, lane >> 5); rows m >= ld are zeros.
__global__ __launch_bounds__(256) void fp_mlp_grad_pack_kernel(const float *__restrict__ w, int ld, int tile0, int tiles, int ks, uint4 *__restrict__ dst) {
    const int first = blockIdx.x * 256 + threadIdx.x, stride = gridDim.x * 256;
    for (int e = first; e < tiles * ks * 64; e += stride) {
        const int lane = e & 63, t = (e >> 6) % tiles, s = (e >> 6) / tiles;
        const int mrow = 32 * (tile0 + t) + (lane & 31);
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int k = 32 * (s >> 1) + mcp_chan_of(8 * (s & 1) + i, lane >> 5);
            v[i] = mrow < ld ? w[(size_t)k * ld + mrow] : 0.f;
        }
        const McpSplit3 sp = mcp_split8(v);
        uint4 *o = dst + (size_t)(s * tiles + t) * TILE_U4 + lane;
        o[0] = sp.p1;
        o[64] = sp.p2;
        o[128] = sp.p3;
    }
}

struct FgArgs {
    long long total;  // B * n rows
    int n, m, c2, c1, rule, layers;
    int ksb, ks0;
    int t0, t1, t2, b1, b2;                // per layer: output tiles, bias offset (named: never indexed at run time)
    int w_u4, small_floats, bwd_u4, dxt;
};
struct FgIn {
    const float *known_feats, *skip, *dist, *w3, *packed, *grad_out;
    const int *idx, *ulen;
};
struct FgOut {
    float *x, *h1, *h2, *gz1, *gz2, *gz3, *grad_blend, *w_used, *grad_skip, *out;
};

template <int TMAX, bool STREAM>
__global__ __launch_bounds__(THREADS, 1) void fp_mlp_grad_kernel(const FgArgs a, const FgIn in, const FgOut o) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *small = lds;                                               // biases, then one phase's slabs or two slab buffers
    const int tid = threadIdx.x, h = (tid & 63) >> 5;
    const u32x4 *gimg = reinterpret_cast<const u32x4 *>(in.packed);
    const int small_u4 = a.small_floats / 4;   // the biases lie between the forward and the backward slabs
    FpSlabs<TMAX, STREAM> slabs;
    {
        const float4 *src = reinterpret_cast<const float4 *>(in.packed) + a.w_u4;
        for (int e = tid; e < small_u4; e += THREADS) reinterpret_cast<float4 *>(small)[e] = src[e];
        slabs.begin(reinterpret_cast<u32x4 *>(lds + a.small_floats), gimg, a.t0, a.w_u4);
    }
    __syncthreads();

    const FpRow me(a.total, a.n, in.ulen);
    const long long p = me.p;
    const bool inr = me.inr, live = me.live;
    FpGather g;
    g.begin(me, a.m, a.c2, a.c1, a.rule, a.ksb, in.known_feats, in.skip, in.idx, in.dist, in.w3);
    g.store_w_used(o.w_used, p);
    // The row index behind a compiler barrier: an address formed from it is formed where it is used.  Without it the compiler
    // forms the 64-bit row addresses of all eleven arrays at the top of the kernel and keeps them beside the bank.
    auto row = [&]() {
        long long q = p;
        asm volatile("" : "+v"(q));
        return q;
    };

    // bank += W . rows over `ks` k-steps of the lane's own row of a workspace array (h_l or gz_l, just written by this lane): the
    // layer-1 loop again.  Only one bank is ever live.  `after`, `skip_u4`: the slab behind the last one of this product.
    auto layer_from_rows = [&](f32x16(&bank)[TMAX], const float *rows, int ks, int tiles, int after, int skip_u4) {
        fp_ksteps(ks, [&](int s) { return fp_row_kstep(rows, s, inr); },
                  [&](const FpQuads &n, int, bool last) {
                      const float v[8] = {n.a0.x, n.a0.y, n.a0.z, n.a0.w, n.a1.x, n.a1.y, n.a1.z, n.a1.w};
                      slabs.into(bank, tiles, mcp_split8(v), last ? after : tiles, last ? skip_u4 : 0);
                  });
    };
    // forward layer l >= 2: h_(l-1) = ReLU(bank) to the workspace, then the bank is the next layer's
    auto next_layer = [&](f32x16(&bank)[TMAX], int tin, int tout, int boff, float *hl, int after, bool last_forward) {
        float *hrow = hl + row() * (tin * 32) + 4 * h;
#pragma unroll
        for (int t = 0; t < TMAX; ++t) {
            if (t < tin && inr) {
                f32x16 r = bank[t];
#pragma unroll
                for (int i = 0; i < 16; ++i) r[i] = r[i] > 0.f ? r[i] : 0.f;
                fp_store_tile(hrow, t, r);
            }
        }
#pragma unroll
        for (int t = 0; t < TMAX; ++t) fp_bias_tile(bank[t], t, tout, small + boff);
        layer_from_rows(bank, hrow, 2 * tin, tout, after, last_forward ? small_u4 : 0);
    };
    // gz_L = g selected by [out > 0], written to the workspace; the recomputed out on the way
    auto grad_last = [&](f32x16(&bank)[TMAX], int tiles, float *gz) {
        const long long at = row() * (tiles * 32) + 4 * h;
#pragma unroll
        for (int t = 0; t < TMAX; ++t) {
            if (t < tiles && inr) {
                f32x16 outv, gzv;
#pragma unroll
                for (int g4 = 0; g4 < 4; ++g4) {
                    float4 gv = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (live) gv = *reinterpret_cast<const float4 *>(in.grad_out + at + 32 * t + 8 * g4);
                    const float gq[4] = {gv.x, gv.y, gv.z, gv.w};
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float v = bank[t][4 * g4 + j];
                        const bool pos = v > 0.f;
                        outv[4 * g4 + j] = (pos && live) ? v : 0.f;
                        gzv[4 * g4 + j] = pos ? gq[j] : 0.f;
                    }
                }
                fp_store_tile(gz + at, t, gzv);
                if (o.out) fp_store_tile(o.out + at, t, outv);
                __builtin_amdgcn_sched_barrier(0);   // one tile's rows of g in flight, not the whole bank's
            }
        }
    };
    // gz_(l-1) = (W_l^T gz_l) selected by [h_(l-1) > 0] (h_(l-1) read back from the workspace), written to the workspace
    auto back_layer = [&](f32x16(&bank)[TMAX], const float *gz_in, int tin, int tout, const float *hl, float *gz_out, int after) {
        fp_zero_bank(bank);
        layer_from_rows(bank, gz_in + row() * (tin * 32) + 4 * h, 2 * tin, tout, after, 0);
        const long long at = row() * (tout * 32) + 4 * h;
#pragma unroll
        for (int t = 0; t < TMAX; ++t) {
            if (t < tout && inr) {
                f32x16 v = bank[t];
#pragma unroll
                for (int g4 = 0; g4 < 4; ++g4) {
                    const float4 hv = *reinterpret_cast<const float4 *>(hl + at + 32 * t + 8 * g4);
                    v[4 * g4 + 0] = hv.x > 0.f ? v[4 * g4 + 0] : 0.f;
                    v[4 * g4 + 1] = hv.y > 0.f ? v[4 * g4 + 1] : 0.f;
                    v[4 * g4 + 2] = hv.z > 0.f ? v[4 * g4 + 2] : 0.f;
                    v[4 * g4 + 3] = hv.w > 0.f ? v[4 * g4 + 3] : 0.f;
                }
                fp_store_tile(gz_out + at, t, v);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    };

    f32x16 bank[TMAX];
    // ---- phase 1, layer 1: input k-steps from memory, x written to the workspace on the way ----
    const int dx_first = min(TMAX, a.dxt);   // output tiles of the first chunk of dx
    const int after1 = a.layers == 1 ? dx_first : a.t1;
#pragma unroll
    for (int t = 0; t < TMAX; ++t) fp_bias_tile(bank[t], t, a.t0, small);
    fp_ksteps(a.ks0, [&](int s) { return g.fetch(s); },
              [&](const FpGatherRaw &now, int s, bool last) {
                  slabs.into(bank, a.t0, g.finish(now, s, o.x, row()), last ? after1 : a.t0, last && a.layers == 1 ? small_u4 : 0);
              });
    // the backward slabs take the forward slabs' place
    auto phase_two = [&]() { slabs.restage(gimg + a.w_u4 + small_u4, a.bwd_u4); };
    // ---- the rest of phase 1, then phase 2: gz_L, back through the layers to gz_1 ----
    if (a.layers == 1) {
        phase_two();
        grad_last(bank, a.t0, o.gz1);
    } else {
        next_layer(bank, a.t0, a.t1, a.b1, o.h1, a.layers == 2 ? a.t0 : a.t2, a.layers == 2);
        if (a.layers == 2) {
            phase_two();
            grad_last(bank, a.t1, o.gz2);
        } else {
            next_layer(bank, a.t1, a.t2, a.b2, o.h2, a.t1, true);
            phase_two();
            grad_last(bank, a.t2, o.gz3);
            back_layer(bank, o.gz3, a.t2, a.t1, o.h2, o.gz2, a.t0);
        }
        back_layer(bank, o.gz2, a.t1, a.t0, o.h1, o.gz1, dx_first);
    }

    // ---- dx = W_1^T gz_1 in chunks of TMAX output tiles, each from the k-steps of gz_1 again ----
    const float *g1row = o.gz1 + row() * (a.t0 * 32) + 4 * h;
#pragma unroll 1
    for (int c0 = 0; c0 < a.dxt; c0 += TMAX) {
        const int tc = min(TMAX, a.dxt - c0);
        fp_zero_bank(bank);
        layer_from_rows(bank, g1row, 2 * a.t0, tc, min(TMAX, a.dxt - c0 - TMAX), 0);
        if (inr) fp_store_dx(bank, c0, tc, row(), a.c2, a.c1, o.grad_blend, o.grad_skip);
    }
}

// The caller-owned workspace: byte offsets of its parts, each 256-byte aligned.
struct FgLayout {
    size_t x, h1, h2, gz[MAX_LAYERS], grad_blend, w_used, dw_slice, wgrad, wgrad_bytes, bytes;
};
// false: mcp_linear_wgrad does not take one of the layers' products
inline bool fg_layout(long long total, const FgShape &s, const int *widths, FgLayout *l) {
    FpTake take;
    const size_t rows = (size_t)total;
    l->x = take(rows * s.cin);
    l->h1 = take(s.f.layers >= 2 ? rows * widths[0] : 0);
    l->h2 = take(s.f.layers >= 3 ? rows * widths[1] : 0);
    for (int i = 0; i < MAX_LAYERS; ++i) l->gz[i] = take(i < s.f.layers ? rows * widths[i] : 0);
    l->grad_blend = take(rows * s.f.c2);
    l->w_used = take(rows * 3);
    l->dw_slice = take(s.cin > WGRAD_COLS ? (size_t)widths[0] * WGRAD_COLS : 0);
    if (!fp_wgrad_bytes(total, s, widths, &l->wgrad_bytes)) return false;
    l->wgrad = take.at;
    l->bytes = take.at + FpTake::up(l->wgrad_bytes);
    return true;
}

}  // namespace

MCP_EXPORT int mcp_fp_mlp_grad_packed_floats(int c2, int c1, int layers, const int *widths) {
    FgShape sh;
    if (!fg_shape(c2, c1, layers, widths, &sh)) return 0;
    return (int)fg_image_floats(sh);
}

MCP_EXPORT int mcp_fp_mlp_grad_pack(int c2, int c1, int layers, const int *widths, const float *const *w, const float *const *b, float *packed,
                                    mcp_stream_t stream) {
    MCP_CHECK_ARGS(widths && w && b && packed);
    FgShape sh;
    if (!fg_shape(c2, c1, layers, widths, &sh)) return MCP_ERR_UNSUPPORTED;
    int rc = mcp_fp_mlp_pack(c2, c1, layers, widths, w, b, packed, stream);   // [forward slabs | biases]
    if (rc != MCP_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    uint4 *pw = reinterpret_cast<uint4 *>(packed + (size_t)sh.f.w_u4 * 4 + sh.f.small_floats);
    auto go = [&](const float *wl, int ld, int tile0, int tiles, int ks) {
        const int work = tiles * ks * 64;
        hipLaunchKernelGGL(fp_mlp_grad_pack_kernel, dim3((work + 255) / 256), dim3(256), 0, s, wl, ld, tile0, tiles, ks, pw);
        pw += (size_t)tiles * ks * TILE_U4;
        return mcp_launch_status();
    };
    for (int l = layers - 1; l >= 1; --l)
        if ((rc = go(w[l], widths[l - 1], 0, sh.f.tiles[l - 1], 2 * sh.f.tiles[l])) != MCP_OK) return rc;
    for (int c0 = 0; c0 < sh.dxt; c0 += sh.f.tmax) {
        const int tc = sh.dxt - c0 < sh.f.tmax ? sh.dxt - c0 : sh.f.tmax;
        if ((rc = go(w[0], sh.cin, c0, tc, 2 * sh.f.tiles[0])) != MCP_OK) return rc;
    }
    return MCP_OK;
}

MCP_EXPORT size_t mcp_fp_mlp_grad_workspace_bytes(int b, int n, int c2, int c1, int layers, const int *widths) {
    FgShape sh;
    if (b <= 0 || n <= 0 || !fg_shape(c2, c1, layers, widths, &sh)) return 0;
    FgLayout lay;
    return fg_layout((long long)b * n, sh, widths, &lay) ? lay.bytes : 0;
}

MCP_EXPORT int mcp_fp_mlp_grad(int b, int n, int m, int c2, int c1, int rule, int layers, const int *widths, const float *known_feats,
                               const float *skip, const int *idx, const float *dist, const float *w3, const int *ulen, const float *packed,
                               const float *grad_out, const int *order, const int *seg, float *grad_known_feats, float *grad_skip,
                               float *const *grad_w, float *const *grad_b, float *out, void *workspace, size_t workspace_bytes,
                               mcp_stream_t stream) {
    MCP_CHECK_ARGS(b > 0 && n > 0 && m > 0 && widths && known_feats && idx && packed && grad_out && grad_w && grad_b && workspace && rule >= 0 && rule <= 2);
    MCP_CHECK_ARGS((c1 <= 0 || (skip && grad_skip)) && (rule == 0 ? w3 != nullptr : dist != nullptr) && (!grad_known_feats || (order && seg)));
    FgShape sh;
    if (!fg_shape(c2, c1, layers, widths, &sh)) return MCP_ERR_UNSUPPORTED;
    for (int l = 0; l < layers; ++l) MCP_CHECK_ARGS(grad_w[l] && grad_b[l]);
    const uintptr_t quads = (uintptr_t)known_feats | (uintptr_t)packed | (uintptr_t)grad_out | (uintptr_t)out | (uintptr_t)workspace |
                            ((c1 & 3) == 0 ? (uintptr_t)skip | (uintptr_t)grad_skip : 0);
    if (quads & 15) return MCP_ERR_BAD_ARG;
    const long long total = (long long)b * n;
    FgLayout lay;
    if (!fg_layout(total, sh, widths, &lay)) return MCP_ERR_UNSUPPORTED;
    if (workspace_bytes < lay.bytes) return MCP_ERR_BAD_ARG;
    if ((total + 32 * WAVES - 1) / (32 * WAVES) > 0x7FFFFFFFLL) return MCP_ERR_UNSUPPORTED;
    char *ws = reinterpret_cast<char *>(workspace);
    auto part = [&](size_t off) { return reinterpret_cast<float *>(ws + off); };
    float *x = part(lay.x), *hid[2] = {part(lay.h1), part(lay.h2)}, *gz[MAX_LAYERS] = {part(lay.gz[0]), part(lay.gz[1]), part(lay.gz[2])};
    float *grad_blend = part(lay.grad_blend), *w_used = part(lay.w_used);

    const FpShape &f = sh.f;
    FgArgs a;
    a.total = total;
    a.n = n; a.m = m; a.c2 = c2; a.c1 = c1; a.rule = rule; a.layers = layers;
    a.ksb = f.ksb; a.ks0 = f.ks[0];
    a.t0 = f.tiles[0]; a.t1 = f.tiles[1]; a.t2 = f.tiles[2];
    a.b1 = f.boff[1]; a.b2 = f.boff[2];
    a.w_u4 = f.w_u4; a.small_floats = f.small_floats; a.bwd_u4 = sh.bwd_u4; a.dxt = sh.dxt;
    const FgIn in{known_feats, skip, dist, w3, packed, grad_out, idx, ulen};
    const FgOut o{x, hid[0], hid[1], gz[0], gz[1], gz[2], grad_blend, w_used, grad_skip, out};
    hipStream_t s = (hipStream_t)stream;
    int rc = fp_dispatch(f.tmax, !fg_whole(sh), [&](auto tmax, auto stream_w) {
        constexpr int T = decltype(tmax)::value;
        constexpr bool S = decltype(stream_w)::value;
        return fp_launch<fp_mlp_grad_kernel<T, S>, T, S>(total, a.small_floats, a.w_u4 > a.bwd_u4 ? a.w_u4 : a.bwd_u4, s, a, in, o);
    });
    if (rc != MCP_OK) return rc;

    // the blend's scatter: every destination row's addends in ascending position 3 p + j
    if (grad_known_feats) {
        rc = mcp_interp3_apply_grad_sorted(b, n, m, c2, nullptr, idx, w_used, grad_blend, order, seg, grad_known_feats, nullptr, stream);
        if (rc != MCP_OK) return rc;
    }
    // dW_l = gz_l^T h_(l-1), db_l = column sums of gz_l
    void *wws = ws + lay.wgrad;
    for (int l = layers - 1; l >= 1; --l) {
        rc = mcp_linear_wgrad(total, widths[l], widths[l - 1], gz[l], widths[l], hid[l - 1], widths[l - 1], grad_w[l], grad_b[l], wws, lay.wgrad_bytes,
                              stream);
        if (rc != MCP_OK) return rc;
    }
    if (sh.cin <= WGRAD_COLS) return mcp_linear_wgrad(total, widths[0], sh.cin, gz[0], widths[0], x, sh.cin, grad_w[0], grad_b[0], wws, lay.wgrad_bytes, stream);
    float *slice = part(lay.dw_slice);
    for (int c0 = 0; c0 < sh.cin; c0 += WGRAD_COLS) {   // columns c0 .. c0 + kb - 1 of x through the row stride; the dense (width, kb) block is then laid into dW_1
        const int kb = sh.cin - c0 < WGRAD_COLS ? sh.cin - c0 : WGRAD_COLS;
        rc = mcp_linear_wgrad(total, widths[0], kb, gz[0], widths[0], x + c0, sh.cin, slice, c0 == 0 ? grad_b[0] : nullptr, wws, lay.wgrad_bytes, stream);
        if (rc != MCP_OK) return rc;
        const hipError_t e = hipMemcpy2DAsync(grad_w[0] + c0, (size_t)sh.cin * sizeof(float), slice, (size_t)kb * sizeof(float), (size_t)kb * sizeof(float),
                                              (size_t)widths[0], hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) return (int)e;
    }
    return MCP_OK;
}
