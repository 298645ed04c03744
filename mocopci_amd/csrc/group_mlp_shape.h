// group_mlp_shape.h -- the shape arithmetic of the fused set-abstraction layer, shared by its forward (group_mlp.hip), its backward
// (group_mlp_grad.hip) and its training-mode BatchNorm form (group_mlp_bn.hip): which shapes are built, a pair's input row, the
// k-steps and output tiles of every layer, the layout of the forward weight image and the register class of the forward.  Host code
// only; the device code and the rest of the host code the three units share are in group_mlp_tile.h, which includes this header.
// MAX_LAYERS, TILE_U4, LDS_IMAGE_BYTES and FpTake are fp_mlp_shape.h's: the two families build the same kind of image.
#pragma once
#include "fp_mlp_shape.h"

namespace {

// a (centre, slot) pair's row of x as the training units lay it out: [features (c) | position (px)]
struct GmRow {
    int c;
    int px;              // 3 with use_xyz, else 0
    int cin, ldx;        // c + px; floats of a row of x (cin rounded up to whole quads)
    int dxt;             // 32-channel tiles of dx
};

struct GmShape {
    int layers;
    GmRow x;
    int ks[MAX_LAYERS];     // k-steps (16 input channels each) of layer l's split product; ks[0] covers the features only
    int tiles[MAX_LAYERS];  // 32-channel output tiles of layer l
    int woff[MAX_LAYERS];   // uint4 offset of layer l's pieces in the image
    int boff[MAX_LAYERS];   // float offset of layer l's bias in the small part (the position columns come first, at 0)
    int w_u4, small_floats; // image: [w_u4 uint4 | small_floats floats]
    int kmax;               // register class: 4 or 8
};

__host__ __device__ inline int gm_pow2_up(int v) { int p = 1; while (p < v) p <<= 1; return v <= 0 ? 0 : p; }

// The one statement of the supported shapes (mcp_group_mlp's header lists them; nsample is the entry points' own check).
// false: outside them
inline bool gm_supported(int c, int use_xyz, int layers, const int *widths, GmRow *x) {
    if (layers < 1 || layers > MAX_LAYERS || !widths || c < 0 || c > 128 || (c & 3) || (c == 0 && !use_xyz)) return false;
    for (int l = 0; l < layers; ++l) {
        const int w = widths[l];
        const bool ok = w == 32 || w == 64 || w == 128 || (l == layers - 1 && w == 256);
        if (!ok) return false;
    }
    x->c = c;
    x->px = use_xyz ? 3 : 0;
    x->cin = c + x->px;
    x->ldx = (x->cin + 3) & ~3;
    x->dxt = (x->cin + 31) / 32;
    return true;
}

// false: outside the supported shapes
inline bool gm_shape(int c, int use_xyz, int layers, const int *widths, GmShape *s) {
    if (!gm_supported(c, use_xyz, layers, widths, &s->x)) return false;
    s->layers = layers;
    int u4 = 0, fl = widths[0] / 32 * 128, kmax = 4;
    for (int l = 0; l < MAX_LAYERS; ++l) {
        if (l >= layers) { s->ks[l] = s->tiles[l] = s->woff[l] = s->boff[l] = 0; continue; }
        s->ks[l] = l == 0 ? gm_pow2_up((c + 15) / 16) : widths[l - 1] / 16;
        s->tiles[l] = widths[l] / 32;
        s->woff[l] = u4;
        s->boff[l] = fl;
        u4 += s->tiles[l] * s->ks[l] * TILE_U4;
        fl += widths[l];
        if (s->ks[l] > 4) kmax = 8;
    }
    s->w_u4 = u4;
    s->small_floats = fl;
    s->kmax = kmax;
    return true;
}
// the LDS / L2 dispatch predicate, a function of (c, widths) alone (ops.group_mlp_weights_in_lds mirrors it)
inline bool gm_weights_in_lds(const GmShape &s) { return (size_t)s.w_u4 * 16 <= (size_t)LDS_IMAGE_BYTES; }

// the column groups of a call: a centre takes P = 1 << logp columns of a 32-column tile, a wave's unit is 32 / P centres
struct GmUnits {
    int logp;          // log2 of the column group of a centre (3, 4, 5)
    int ctiles;        // column tiles per centre: 2 when nsample > 32
    long long units;
};
inline GmUnits gm_units(long long total, int nsample) {
    GmUnits u;
    u.logp = nsample <= 8 ? 3 : nsample <= 16 ? 4 : 5;
    u.ctiles = nsample > 32 ? 2 : 1;
    const int G = 32 >> u.logp;
    u.units = (total + G - 1) / G;
    return u;
}

}  // namespace
