// fp_mlp_shape.h -- the shape arithmetic of the fused feature-propagation layer, shared by its forward (fp_mlp.hip) and its backward
// (fp_mlp_grad.hip): which shapes are built, the k-steps and output tiles of every layer, the size of the forward weight image and
// the register class.  Host code only.
#pragma once

namespace {

constexpr int WAVES = 4;
constexpr int THREADS = 64 * WAVES;
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

}  // namespace
