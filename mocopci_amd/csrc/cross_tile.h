// cross_tile.h -- what the three units of the fused cost volume share: the forward (cross.hip), its backward at D = 64 / 128
// (cross_grad.hip) and at D = 256 (cross256_grad.hip).  Both backward paths recompute z as the forward computes it, bit for bit, and
// place dz at the forward's arg-max.  Stated here once: the constants and the layout of the packed image, a lane's neighbour, the
// layer-1 tile and the arg-max winner of the two backward kernels, the D = 256 streaming constants, the backward entry checks.
// The forward kernels keep their own text of the layer-1 tile and of the D = 256 weight-streaming walk (pass Z keeps its copy of the
// walk): called through a helper they compile to another instruction stream ("The cost volume's shared code"), and
// their schedules are not to move.  The units also keep what they do not share: the neighbour max (scatter_max), the per-point
// pipelines and grids, passes W and DX, the backward's roles.
#pragma once
#include "mfma_split.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr int KNB = 32;
constexpr float SLOPE = 0.1f;  // pointconv_util.py:10
// LeakyReLU with 0 < slope < 1 is max(v, slope*v): two instructions, same value for every finite v (and for +-0)
__device__ __forceinline__ float leaky(float v) { return mcp_max_raw(v, v * SLOPE); }

// ---- the image mcp_cross_pack writes (floats): split Wmlp [t_out][k-step = 2T][piece = 3][lane] x uint4 | pos | bias ----
template <int D>
struct CrossLds {
    static constexpr int T = D / 32;
    static constexpr int W_FLOATS = T * (2 * T) * 3 * 64 * 4;  // 1.5 D*D
    static constexpr int POS_FLOATS = T * 2 * 64;               // [t][kstep][lane]
    static constexpr int B_FLOATS = T * 2 * 16;                 // [t][half][r]
    static constexpr int OFF_W = 0, OFF_POS = W_FLOATS, OFF_B = OFF_POS + POS_FLOATS;
    static constexpr int FLOATS = OFF_B + B_FLOATS;
};
// float4 number of channels 32t + 8g + 4h .. +3 of a feature row: registers 4g .. 4g+3 of lane half h in accumulator tile t
__device__ __forceinline__ int cross_at(int t, int g, int h) { return (32 * t + 8 * g + 4 * h) >> 2; }

// Neighbour `col` of flat point p: one (B,N1,32) list, or -- idx2 != NULL -- the 16 feature-space and the 16 coordinate-space
// neighbours as two (B,N1,16) lists.  ps() is p's row in the first list: p itself, except under the forward's batch map, whose
// lookup is made only on the two-list path (hence a callable).  Written as cross_kernel had it: its stream does not change.
template <class PS>
__device__ __forceinline__ int cross_nbr(const int *idx, const int *idx2, long long p, PS ps, int col) {
    if (!idx2) return idx[p * KNB + col];
    const long long s = ps();
    return col >= 16 ? idx2[p * 16 + col - 16] : idx[s * 16 + col];
}
__device__ __forceinline__ int cross_nbr(const int *idx, const int *idx2, long long p, int col) {
    return cross_nbr(idx, idx2, p, [p] { return p; }, col);
}

// Layer 1 of one 32-channel tile, the arithmetic only: x = LeakyReLU(points2[idx] + points1 + [Wpos | bpos] [dx,dy,dz,1]).  The
// points1 row initialises the accumulator (broadcast over the neighbours), the positional term is two K = 2 MFMAs with this lane's
// two entries of tile t of the position image `pos`, the gathered row is added in accumulator layout.  own(g) / gathered(g) give float4
// cross_at(t, g, h) of the two rows from wherever the caller has them (an LDS row, prefetched registers, global memory) and are
// called in that order per g; xsink(g, acc) sees registers 4g .. 4g+3 as soon as they are final.
template <class Own, class Gathered, class XSink>
__device__ __forceinline__ f32x16 cross_layer1(const float *pos, int t, int lane, float in0, float in1, Own own, Gathered gathered, XSink xsink) {
    f32x16 acc;
    float4 rg[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const float4 a = own(g);
        rg[g] = gathered(g);
        acc[4 * g + 0] = a.x; acc[4 * g + 1] = a.y; acc[4 * g + 2] = a.z; acc[4 * g + 3] = a.w;
    }
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(pos[(t * 2 + 0) * 64 + lane], in0, acc, 0, 0, 0);   // k-step 0: (dx,dy)
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(pos[(t * 2 + 1) * 64 + lane], in1, acc, 0, 0, 0);  // k-step 1: (dz,1)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        acc[4 * g + 0] = leaky(acc[4 * g + 0] + rg[g].x);
        acc[4 * g + 1] = leaky(acc[4 * g + 1] + rg[g].y);
        acc[4 * g + 2] = leaky(acc[4 * g + 2] + rg[g].z);
        acc[4 * g + 3] = leaky(acc[4 * g + 3] + rg[g].w);
        xsink(g, acc);
    }
    return acc;
}
struct CrossNoXSink {  // x is not stored
    __device__ __forceinline__ void operator()(int, const f32x16 &) const {}
};

// ---- the arg-max neighbour of a channel, as the backward places dz ----
template <int CTRL>
__device__ __forceinline__ uint32_t max_dpp(uint32_t v) {
    const uint32_t o = mcp_dpp<CTRL>(v);
    return v > o ? v : o;
}
// maximum over the 32 lanes that share lane >> 5, in every lane
__device__ __forceinline__ uint32_t half_max_u32(uint32_t v) {
    v = max_dpp<0xB1>(v);   // quad_perm [1,0,3,2]
    v = max_dpp<0x4E>(v);   // quad_perm [2,3,0,1]
    v = max_dpp<0x141>(v);  // row_half_mirror
    v = max_dpp<0x140>(v);  // row_mirror
    const auto sw = __builtin_amdgcn_permlane16_swap(v, v, false, false);  // odd rows of one copy <-> even rows of the other
    return sw[0] > sw[1] ? sw[0] : sw[1];
}
// Is this lane's neighbour the arg-max of zv over the 32 lanes of its half?  An all-reduce max on order-preserving keys; among equal
// maxima the lowest list position wins (the two 16-neighbour lists overlap, so exact ties are common), found with the comparison's
// own lane mask: lower_lanes = (1 << col) - 1.  Exactly one lane of a half wins.
__device__ __forceinline__ bool cross_winner(float zv, int h, uint32_t lower_lanes) {
    const uint32_t key = mcp_ord(zv);
    const bool top = key == half_max_u32(key);
    const unsigned long long mask = __builtin_amdgcn_ballot_w64(top);
    const uint32_t mine = h ? (uint32_t)(mask >> 32) : (uint32_t)mask;
    return top && (mine & lower_lanes) == 0u;
}

// ---- D = 256 (cross3, pointconv_util.py:783-791): the shape of the weight-streaming walk of cross256_stream_kernel (cross.hip) and of
// pass Z (cross256_grad.hip), derived from the packed image: eight 32-channel output tiles of 16 k-steps x 3 pieces x 64 lanes ----
constexpr int X256_T = CrossLds<256>::T, X256_KS = 2 * X256_T, X256_TILE_U4 = X256_KS * 3 * 64, X256_WAVES = 4;
constexpr int X256_SMALL = CrossLds<256>::POS_FLOATS + CrossLds<256>::B_FLOATS;
// LDS of the walk (floats): two weight tiles | pos + bias | one points1 row per wave; the forward's batch map comes behind it
constexpr int X256_LDS_FLOATS = 2 * X256_TILE_U4 * 4 + X256_SMALL + X256_WAVES * 256;
static_assert(X256_T * X256_TILE_U4 * 4 == CrossLds<256>::W_FLOATS, "the tiles are the packed image's weight part");
static_assert((size_t)X256_LDS_FLOATS * sizeof(float) <= 160 * 1024, "LDS budget");

// ---- the argument and alignment checks of the two backward entry points (d_ok: the unit supports this D) ----
inline int cross_grad_check(int b, int n1, int n2, bool d_ok, int k, const float *xyz1, const float *xyz2, const float *points1, const float *points2,
                            const int *idx, const float *wpos, const float *bpos, const float *wmlp, const float *bmlp, const float *grad_out,
                            const float *grad_xyz1, const float *grad_dir, const float *grad_points1, const float *grad_rows, const float *grad_weights,
                            const void *workspace) {
    MCP_CHECK_ARGS(b > 0 && n1 > 0 && n2 > 0 && xyz1 && xyz2 && points1 && points2 && idx && wpos && bpos && wmlp && bmlp && grad_out && grad_xyz1 &&
                   grad_dir && grad_points1 && grad_rows && grad_weights && workspace);
    if (k != KNB || !d_ok) return MCP_ERR_UNSUPPORTED;
    if ((((uintptr_t)points1) | ((uintptr_t)points2) | ((uintptr_t)grad_out) | ((uintptr_t)grad_rows) | ((uintptr_t)workspace)) & 15) return MCP_ERR_BAD_ARG;
    return MCP_OK;
}

}  // namespace
