// group_mlp_shape.h -- the shape arithmetic of the fused set-abstraction layer, shared by its forward (group_mlp.hip) and its backward
// (group_mlp_grad.hip): which shapes are built, the k-steps and output tiles of every layer, the layout of the forward weight image
// and the register class of the forward.  Host code only.
#pragma once

namespace {

constexpr int MAX_LAYERS = 3;
constexpr int LDS_IMAGE_BYTES = 64 * 1024;    // largest weight image staged in LDS

struct GmShape {
    int layers, c;
    int ks[MAX_LAYERS];     // k-steps (16 input channels each) of layer l's split product; ks[0] covers the features only
    int tiles[MAX_LAYERS];  // 32-channel output tiles of layer l
    int woff[MAX_LAYERS];   // uint4 offset of layer l's pieces in the image
    int boff[MAX_LAYERS];   // float offset of layer l's bias in the small part (the position columns come first, at 0)
    int w_u4, small_floats; // image: [w_u4 uint4 | small_floats floats]
    int kmax;               // register class: 4 or 8
};

__host__ __device__ inline int gm_pow2_up(int v) { int p = 1; while (p < v) p <<= 1; return v <= 0 ? 0 : p; }

// false: outside the supported shapes
inline bool gm_shape(int c, int layers, const int *widths, GmShape *s) {
    if (layers < 1 || layers > MAX_LAYERS || !widths || c < 0 || c > 128 || (c & 3)) return false;
    for (int l = 0; l < layers; ++l) {
        const int w = widths[l];
        const bool ok = w == 32 || w == 64 || w == 128 || (l == layers - 1 && w == 256);
        if (!ok) return false;
    }
    s->layers = layers;
    s->c = c;
    int u4 = 0, fl = widths[0] / 32 * 128, kmax = 4;
    for (int l = 0; l < MAX_LAYERS; ++l) {
        if (l >= layers) { s->ks[l] = s->tiles[l] = s->woff[l] = s->boff[l] = 0; continue; }
        s->ks[l] = l == 0 ? gm_pow2_up((c + 15) / 16) : widths[l - 1] / 16;
        s->tiles[l] = widths[l] / 32;
        s->woff[l] = u4;
        s->boff[l] = fl;
        u4 += s->tiles[l] * s->ks[l] * 3 * 64;
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

}  // namespace
