// group_mlp_tile.h -- the device code and the host code that the three units of the fused set-abstraction layer share: the forward
// (group_mlp.hip), its backward (group_mlp_grad.hip) and the training-mode BatchNorm form (group_mlp_bn.hip).  group_mlp_shape.h holds
// the shape arithmetic; this header holds what a wave does with one column of the MFMA in the two persistent kernels -- the column's
// centre (GmCentre), the position operand (gm_position), the head of a layer-1 output tile (gm_layer1_head), the bias tile, the
// column-group butterflies -- the two pack kernels of the three images, and on the host the launch of the persistent kernels, the
// backward-only parts of the workspace and the tail of the two backward entry points.  Every unit keeps its argument structs, its
// control flow, its phases, its ReLU and its epilogues.
//
// Rules the callers rely on: nothing here depends on -fno-honor-nans (the forward is built with it, the two training units without:
// the code below holds no ReLU and no selection on a possibly-NaN value; the fmaxf of gm_group_max meets values >= 0 only); no
// function branches on which unit calls it -- what differs between the units (the pinned lane copies of the forward, the entry
// order of an image) arrives as data.
#pragma once
#include "common.h"
#include "mfma_split.h"
#include "group_mlp_shape.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---- this column's centre of the flattened (B * M) list: unit `unit` holds 32 >> logp centres of 1 << logp columns each.  A centre at
// or beyond the list is not in range; one at or beyond the clamped qlen[bb] is in range but not live: it writes zeros and none of its
// rows (new_xyz, idx, row_bias, grad_out) is read. ----
// the one statement of "which centres are live": centre p of element bb, qlen NULL = every centre
__device__ __forceinline__ bool gm_centre_live(long long p, long long bb, int m, const int *__restrict__ qlen) {
    return !qlen || (int)(p - bb * m) < min(max(qlen[bb], 0), m);
}
struct GmCentre {
    long long p, bb;
    bool inr, live;
    __device__ __forceinline__ GmCentre(long long unit, int col, int logp, long long total, int m, const int *__restrict__ qlen) {
        p = unit * (32 >> logp) + (col >> logp);
        inr = p < total;
        bb = inr ? mcp_div(p, m, mcp_fits32(total)) : 0;
        live = inr && gm_centre_live(p, bb, m, qlen);
    }
};

// ---- the position operand: q = xyz[k], ctr = new_xyz[p], neither read unless `live`.  The three relative coordinates are the K = 4
// input of two v_mfma_f32_32x32x2_f32: lane half h of k-step 0 holds (dx, dy), of k-step 1 (dz, 0). ----
struct GmPos {
    float dx, dy, dz;   // xyz[k] - new_xyz[p], zeros when not live (the backward stores them into x)
    float in0, in1;     // this lane's input of k-step 0 and of k-step 1
};
__device__ __forceinline__ GmPos gm_position(const float *__restrict__ q, const float *__restrict__ ctr, bool live, int h) {
    GmPos r{0.f, 0.f, 0.f, 0.f, 0.f};
    if (live) { r.dx = q[0] - ctr[0]; r.dy = q[1] - ctr[1]; r.dz = q[2] - ctr[2]; }
    r.in0 = h ? r.dy : r.dx;   // k-step 0: (dx, dy); k-step 1: (dz, 0)
    r.in1 = h ? 0.f : r.dz;
    return r;
}

// ---- tiles.  `small` is the small part of the forward image in LDS: the K = 4 position columns [t][s][lane], then every layer's bias
// in accumulator order [t][h][r]. ----
// tile t = its bias; `bias` is the layer's
__device__ __forceinline__ f32x16 gm_bias_tile(const float *bias, int t, int h) {
    f32x16 acc;
    const float4 *bq = reinterpret_cast<const float4 *>(bias + (t * 2 + h) * 16);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const float4 v = bq[g];
        acc[4 * g + 0] = v.x; acc[4 * g + 1] = v.y; acc[4 * g + 2] = v.z; acc[4 * g + 3] = v.w;
    }
    return acc;
}
// The head of output tile t of layer 1, before the feature k-steps: bias, + row_bias[p] for a live centre (row_bias NULL: none), then
// the two K = 4 position products.  mcp_group_mlp_grad's `out` is the forward's bit for bit because both kernels run THIS sequence.
// (h, lane) are the caller's: the forward passes its per-tile pinned copies.  wfirst = floats of a row of row_bias.
__device__ __forceinline__ f32x16 gm_layer1_head(const float *small, int bias_at, int t, int h, int lane, const float *__restrict__ row_bias, long long p,
                                                 int wfirst, bool live, int use_xyz, const GmPos &pos) {
    f32x16 acc = gm_bias_tile(small + bias_at, t, h);
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
    if (use_xyz) {
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(small[(t * 2 + 0) * 64 + lane], pos.in0, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(small[(t * 2 + 1) * 64 + lane], pos.in1, acc, 0, 0, 0);
    }
    return acc;
}

// ---- sum / max / min over each column group of P = 8, 16, 32 lanes, the result in every lane of the group: a butterfly of DPP steps
// and, for P = 32, one cross-row shuffle ----
__device__ __forceinline__ float gm_group_sum(float v, int logp) {
    v += __uint_as_float(mcp_dpp<0xB1>(__float_as_uint(v)));    // quad_perm [1,0,3,2]
    v += __uint_as_float(mcp_dpp<0x4E>(__float_as_uint(v)));    // quad_perm [2,3,0,1]
    v += __uint_as_float(mcp_dpp<0x141>(__float_as_uint(v)));   // row_half_mirror: the other quad of the 8
    if (logp >= 4) v += __uint_as_float(mcp_dpp<0x140>(__float_as_uint(v)));  // row_mirror: the other 8 of the row
    if (logp == 5) v += __shfl_xor(v, 16);
    return v;
}
__device__ __forceinline__ float gm_group_max(float v, int logp) {
    v = fmaxf(v, __uint_as_float(mcp_dpp<0xB1>(__float_as_uint(v))));
    v = fmaxf(v, __uint_as_float(mcp_dpp<0x4E>(__float_as_uint(v))));
    v = fmaxf(v, __uint_as_float(mcp_dpp<0x141>(__float_as_uint(v))));
    if (logp >= 4) v = fmaxf(v, __uint_as_float(mcp_dpp<0x140>(__float_as_uint(v))));
    if (logp == 5) v = fmaxf(v, __shfl_xor(v, 16));
    return v;
}
__device__ __forceinline__ int gm_group_min(int v, int logp) {
    v = min(v, (int)mcp_dpp<0xB1>((uint32_t)v));
    v = min(v, (int)mcp_dpp<0x4E>((uint32_t)v));
    v = min(v, (int)mcp_dpp<0x141>((uint32_t)v));
    if (logp >= 4) v = min(v, (int)mcp_dpp<0x140>((uint32_t)v));
    if (logp == 5) v = min(v, __shfl_xor(v, 16));
    return v;
}

// ---- the images.  Input column j of a layer, as the kernels count it, is column gm_col(j) of the caller's W: the cfeat feature columns
// start at col0 (behind the module's position columns of layer 1), npos position columns follow them (the training units' row is
// [features | position]; the forward takes its position through `dstpos`, npos = 0); -1: zeros.  Entry (t, s) of an image -- output
// tile t, k-step s, three pieces of 64 lanes -- lies at (t * st + s * ss) * TILE_U4: (ks, 1) is [t][s], (1, tiles) is [s][t]. ----
__device__ __forceinline__ int gm_col(int j, int col0, int cfeat, int npos) { return j < cfeat ? col0 + j : j < cfeat + npos ? j - cfeat : -1; }

// One layer's forward pieces, mcp_split_weights' layout per entry: W[32 t + (lane & 31)][col(k)] over the 8 values k of (s, lane >> 5).
// pos (NULL: not written): [t][s][lane] = w[32 t + (lane & 31)][2 s + (lane >> 5)] for the columns in front of col0, 0 beyond.
// Bias: [t][h][r].
__global__ __launch_bounds__(256) void gm_pack_fwd_kernel(const float *__restrict__ w, const float *__restrict__ b, int ld, int col0, int cfeat, int npos,
                                                          int ks, int tiles, int st, int ss, uint4 *__restrict__ dstw, float *__restrict__ dstpos,
                                                          float *__restrict__ dstb) {
    const int first = blockIdx.x * 256 + threadIdx.x, stride = gridDim.x * 256;
    for (int e = first; e < tiles * ks * 64; e += stride) {
        const int lane = e & 63, s = (e >> 6) % ks, t = (e >> 6) / ks;
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int col = gm_col(32 * (s >> 1) + mcp_chan_of(8 * (s & 1) + i, lane >> 5), col0, cfeat, npos);
            v[i] = col >= 0 ? w[(size_t)(32 * t + (lane & 31)) * ld + col] : 0.f;
        }
        const McpSplit3 sp = mcp_split8(v);
        uint4 *o = dstw + (size_t)(t * st + s * ss) * TILE_U4 + lane;
        o[0] = sp.p1;
        o[64] = sp.p2;
        o[128] = sp.p3;
    }
    if (dstpos)
        for (int e = first; e < tiles * 128; e += stride) {
            const int lane = e & 63, s = (e >> 6) & 1, t = e >> 7, cc = 2 * s + (lane >> 5);
            dstpos[e] = cc < col0 ? w[(size_t)(32 * t + (lane & 31)) * ld + cc] : 0.f;
        }
    for (int e = first; e < tiles * 32; e += stride) {
        const int r = e & 15, h = (e >> 4) & 1, t = e >> 5;
        dstb[e] = b[32 * t + mcp_chan_of(r, h)];
    }
}
// Pieces of A = W^T for the output tiles tile0 .. tile0 + tiles - 1 (32 rows m of A each) over the ks k-steps of W's rows, in
// mcp_split_weights_transposed's operand layout per entry: A[m][k] = w[k * ld + col(m)], k = 32 (s >> 1) + chan_of(8 (s & 1) + i,
// lane >> 5); the position columns stand in front of the features in W (col0 = npos).
__global__ __launch_bounds__(256) void gm_pack_bwd_kernel(const float *__restrict__ w, int ld, int cfeat, int npos, int tile0, int tiles, int ks, int st,
                                                          int ss, uint4 *__restrict__ dst) {
    const int first = blockIdx.x * 256 + threadIdx.x, stride = gridDim.x * 256;
    for (int e = first; e < tiles * ks * 64; e += stride) {
        const int lane = e & 63, s = (e >> 6) % ks, t = (e >> 6) / ks;
        const int col = gm_col(32 * (tile0 + t) + (lane & 31), npos, cfeat, npos);
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int k = 32 * (s >> 1) + mcp_chan_of(8 * (s & 1) + i, lane >> 5);
            v[i] = col >= 0 ? w[(size_t)k * ld + col] : 0.f;
        }
        const McpSplit3 sp = mcp_split8(v);
        uint4 *o = dst + (size_t)(t * st + s * ss) * TILE_U4 + lane;
        o[0] = sp.p1;
        o[64] = sp.p2;
        o[128] = sp.p3;
    }
}
// the launches; the transposed pieces of an image follow one another, so gm_pack_bwd moves `dst` past what it wrote
inline int gm_pack_fwd(hipStream_t s, const float *w, const float *b, int ld, int col0, int cfeat, int npos, int ks, int tiles, int st, int ss, uint4 *dstw,
                       float *dstpos, float *dstb) {
    const int work = max(tiles * ks * 64, tiles * 128);
    hipLaunchKernelGGL(gm_pack_fwd_kernel, dim3((work + 255) / 256), dim3(256), 0, s, w, b, ld, col0, cfeat, npos, ks, tiles, st, ss, dstw, dstpos, dstb);
    return mcp_launch_status();
}
inline int gm_pack_bwd(hipStream_t s, const float *w, int ld, int cfeat, int npos, int tile0, int tiles, int ks, int st, int ss, uint4 *&dst) {
    const int work = tiles * ks * 64;
    hipLaunchKernelGGL(gm_pack_bwd_kernel, dim3((work + 255) / 256), dim3(256), 0, s, w, ld, cfeat, npos, tile0, tiles, ks, st, ss, dst);
    dst += (size_t)tiles * ks * TILE_U4;
    return mcp_launch_status();
}

// ---- host side.  One launch for the two persistent kernels: KERN is an instantiation, `waves` waves per workgroup take the units in
// turn, `slots` is the resident workgroups of the device (256 CUs x what the kernel's __launch_bounds__ allows per CU); the LDS
// attribute is set once per device and instantiation. ----
template <auto KERN, class... Args>
int gm_launch(long long units, int waves, int slots, size_t lds, hipStream_t s, const Args &...args) {
    if (const int rc = mcp_allow_lds<KERN>()) return rc;
    const long long want = (units + waves - 1) / waves;
    const unsigned grid = (unsigned)max(1LL, min(want, (long long)slots));
    hipLaunchKernelGGL(KERN, dim3(grid), dim3(64 * waves), lds, s, args...);
    return mcp_launch_status();
}

// The backward-only parts of a caller-owned workspace, per (centre, slot) pair row: byte offsets, each part 256-byte aligned.
struct GmBack {
    size_t x, hid[2], gz[MAX_LAYERS], dxf, dxp, dw_slice, wgrad, wgrad_bytes;
};
// false: mcp_linear_wgrad does not take one of the layers' products
inline bool gm_back_layout(FpTake &take, long long rows_ll, const GmRow &r, int layers, const int *widths, GmBack *l) {
    const size_t rows = (size_t)rows_ll;
    l->x = take(rows * r.ldx);
    l->hid[0] = take(layers >= 2 ? rows * widths[0] : 0);
    l->hid[1] = take(layers >= 3 ? rows * widths[1] : 0);
    for (int i = 0; i < MAX_LAYERS; ++i) l->gz[i] = take(i < layers ? rows * widths[i] : 0);
    l->dxf = take(rows * r.c);
    l->dxp = take(rows * r.px);
    l->dw_slice = take(r.px && r.c ? (size_t)widths[0] * r.cin : 0);
    size_t need = 0;   // the scratch of mcp_linear_wgrad: the layer that needs most
    for (int i = 0; i < layers; ++i) {
        const size_t b = mcp_linear_wgrad_workspace_bytes(rows_ll, widths[i], i == 0 ? r.cin : widths[i - 1]);
        if (b == 0) return false;
        if (b > need) need = b;
    }
    l->wgrad = take.at;
    l->wgrad_bytes = need;
    take.at += FpTake::up(need);
    return true;
}

// The tail of a backward entry point, after its kernels have left gz_l, h_l, x and dx = (dxf | dxp) in the workspace `ws`: the two
// scatters and the weight sums.  No atomics: the scatters are mcp_group_rows_grad_sorted over the caller's (order, seg), the weight
// sums mcp_linear_wgrad's fixed-order partial sums.
inline int gm_backward_tail(int b, int n, int m, int nsample, const GmRow &r, int layers, const int *widths, char *ws, const GmBack &l, const int *order,
                            const int *seg, float *grad_features, float *grad_xyz, float *const *grad_w, float *const *grad_b, mcp_stream_t stream) {
    auto part = [&](size_t off) { return reinterpret_cast<float *>(ws + off); };
    const long long rows = (long long)b * m * nsample;
    int rc;
    // the scatters: every destination row's addends in ascending position p nsample + j
    if (grad_features) {
        rc = mcp_group_rows_grad_sorted(b, n, r.c, m * nsample, part(l.dxf), order, seg, grad_features, stream);
        if (rc != MCP_OK) return rc;
    }
    if (grad_xyz) {
        rc = mcp_group_rows_grad_sorted(b, n, 3, m * nsample, part(l.dxp), order, seg, grad_xyz, stream);
        if (rc != MCP_OK) return rc;
    }
    // dW_l = gz_l^T h_(l-1), db_l = column sums of gz_l
    void *wws = ws + l.wgrad;
    for (int i = layers - 1; i >= 1; --i) {
        rc = mcp_linear_wgrad(rows, widths[i], widths[i - 1], part(l.gz[i]), widths[i], part(l.hid[i - 1]), widths[i - 1], grad_w[i], grad_b[i], wws,
                              l.wgrad_bytes, stream);
        if (rc != MCP_OK) return rc;
    }
    const float *gz1 = part(l.gz[0]), *x = part(l.x);
    if (!(r.px && r.c)) return mcp_linear_wgrad(rows, widths[0], r.cin, gz1, widths[0], x, r.ldx, grad_w[0], grad_b[0], wws, l.wgrad_bytes, stream);
    // x holds [features | position]: the product goes to a slice and its two column blocks are laid into dW_1 = [position | features]
    float *slice = part(l.dw_slice);
    rc = mcp_linear_wgrad(rows, widths[0], r.cin, gz1, widths[0], x, r.ldx, slice, grad_b[0], wws, l.wgrad_bytes, stream);
    if (rc != MCP_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const size_t pitch = (size_t)r.cin * sizeof(float);
    hipError_t e = hipMemcpy2DAsync(grad_w[0] + 3, pitch, slice, pitch, (size_t)r.c * sizeof(float), (size_t)widths[0], hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess) return (int)e;
    e = hipMemcpy2DAsync(grad_w[0], pitch, slice + r.c, pitch, 3 * sizeof(float), (size_t)widths[0], hipMemcpyDeviceToDevice, s);
    return e == hipSuccess ? MCP_OK : (int)e;
}

}  // namespace
