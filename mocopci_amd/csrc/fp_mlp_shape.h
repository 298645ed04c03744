// fp_mlp_shape.h -- the shape arithmetic of the fused feature-propagation layer, shared by its forward (fp_mlp.hip), its backward
// (fp_mlp_grad.hip) and its training-mode BatchNorm form (fp_mlp_bn.hip): which shapes are built, the k-steps and output tiles of
// every layer, the size of the forward weight image, the register class, and how a caller-owned workspace is laid out.  Host code
// only; the device code and the launch code the three units share are in fp_mlp_tile.h, which includes this header.  MAX_LAYERS,
// TILE_U4, LDS_IMAGE_BYTES and FpTake are also the set-abstraction layer's (group_mlp_shape.h includes this header), so nothing
// here names a workgroup's size: WAVES and THREADS are fp_mlp_tile.h's.
#pragma once
#include "common.h"

namespace {

constexpr int MAX_LAYERS = 3;
constexpr int TILE_U4 = 3 * 64;               // uint4 of one (output tile, k-step): three pieces of 64 lanes
constexpr int LDS_IMAGE_BYTES = 64 * 1024;    // largest weight image staged whole

struct FpShape {
    int layers, c2, c1;
    int ksb, kss;           // k-steps of the blend and of the skip row in layer 1
    int ks[MAX_LAYERS];     // k-steps of layer l (ks[0] = ksb + kss)
    int tiles[MAX_LAYERS];  // 32-channel output tiles of layer l
    int boff[MAX_LAYERS];   // float offset of layer l's bias in the small part
    int w_u4, small_floats; // image: [w_u4 uint4 | small_floats floats]
    int tmax;               // register class: 2, 4 or 8
};

// false: outside the supported shapes
inline bool fp_shape(int c2, int c1, int layers, const int *widths, FpShape *s) {
    if (layers < 1 || layers > MAX_LAYERS || !widths || c2 < 4 || c2 > 512 || (c2 & 3) || c1 < 0 || c1 > 512 || c1 + c2 > 768) return false;
    for (int l = 0; l < layers; ++l) {
        const int w = widths[l];
        if (!(w == 32 || w == 64 || w == 128 || w == 256)) return false;
    }
    s->layers = layers;
    s->c2 = c2;
    s->c1 = c1;
    s->ksb = (c2 + 15) / 16;
    s->kss = (c1 + 15) / 16;
    int u4 = 0, fl = 0, widest = 0;
    for (int l = 0; l < MAX_LAYERS; ++l) {
        if (l >= layers) { s->ks[l] = s->tiles[l] = s->boff[l] = 0; continue; }
        s->ks[l] = l == 0 ? s->ksb + s->kss : widths[l - 1] / 16;
        s->tiles[l] = widths[l] / 32;
        s->boff[l] = fl;
        u4 += s->tiles[l] * s->ks[l] * TILE_U4;
        fl += widths[l];
        if (widths[l] > widest) widest = widths[l];
    }
    s->w_u4 = u4;
    s->small_floats = fl;
    s->tmax = widest <= 64 ? 2 : widest <= 128 ? 4 : 8;
    return true;
}

// the staging predicate, a function of (c2, c1, widths) alone (ops.fp_mlp_weights_in_lds mirrors it)
inline bool fp_weights_in_lds(const FpShape &s) { return (size_t)s.w_u4 * 16 <= (size_t)LDS_IMAGE_BYTES; }

// ---- the backward: the forward's shape with the slabs of the transposed weights ----
struct FgShape {
    FpShape f;
    int cin, dxt;        // C2 + C1 and its 32-channel tiles
    int bwd_u4;          // uint4 of the backward slabs
};

inline bool fg_shape(int c2, int c1, int layers, const int *widths, FgShape *s) {
    if (!fp_shape(c2, c1, layers, widths, &s->f)) return false;
    const FpShape &f = s->f;
    s->cin = c2 + c1;
    s->dxt = (s->cin + 31) / 32;
    int u4 = 0;
    for (int l = layers - 1; l >= 1; --l) u4 += 2 * f.tiles[l] * f.tiles[l - 1] * TILE_U4;   // gz_l (two k-steps per tile) into the tiles of layer l - 1
    u4 += s->dxt * 2 * f.tiles[0] * TILE_U4;                                                 // gz_1 into the tiles of dx
    s->bwd_u4 = u4;
    return true;
}
// the staging predicate, a function of (c2, c1, widths) alone (ops.fp_mlp_grad_weights_in_lds mirrors it)
inline bool fg_whole(const FgShape &s) {
    return (size_t)s.f.w_u4 * 16 <= (size_t)LDS_IMAGE_BYTES && (size_t)s.bwd_u4 * 16 <= (size_t)LDS_IMAGE_BYTES;
}

// ---- the caller-owned workspace of the training entry points: take(floats) gives the byte offset of the next part, each part
// 256-byte aligned; `at` is the offset behind the parts taken so far ----
struct FpTake {
    size_t at = 0;
    static size_t up(size_t v) { return (v + 255) & ~(size_t)255; }
    size_t operator()(size_t floats) {
        const size_t here = at;
        at += up(floats * sizeof(float));
        return here;
    }
};
constexpr int WGRAD_COLS = 256;   // mcp_linear_wgrad takes at most 256 x 256 outputs: layer 1 goes in column slices of x
// the largest workspace mcp_linear_wgrad asks for over the layers' products; false: it does not take one of them
inline bool fp_wgrad_bytes(long long total, const FgShape &s, const int *widths, size_t *bytes) {
    size_t need = 0;
    for (int i = 0; i < s.f.layers; ++i) {
        const int k = i == 0 ? (s.cin < WGRAD_COLS ? s.cin : WGRAD_COLS) : widths[i - 1];
        const size_t b = mcp_linear_wgrad_workspace_bytes(total, widths[i], k);
        if (b == 0) return false;
        if (b > need) need = b;
    }
    if (s.cin > WGRAD_COLS && s.cin % WGRAD_COLS && !mcp_linear_wgrad_workspace_bytes(total, widths[0], s.cin % WGRAD_COLS)) return false;
    *bytes = need;
    return true;
}
}  // namespace
