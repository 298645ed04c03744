// group_mlp_bn.hip -- the fused set-abstraction layer of pointnet2 with TRAINING-MODE BatchNorm (batch statistics) for gfx950: forward
// and backward of, over the live pairs R = {(p, j): p a live centre, j < nsample}, k = idx[p, j],
//     x = [features[k] | xyz[k] - new_xyz[p] (use_xyz)],  z_l = W_l h_(l-1) + b_l,  y_l = gamma_l (z_l - mu_l) rstd_l + beta_l,
//     h_l = ReLU(y_l),  out[p] = max_j h_(L,j)  or  (sum_j h_(L,j)) / nsample,
// with mu_l / v_l the mean and the biased variance of z_l over R.  Every slot j < nsample counts, the slots that repeat the ball
// query's first hit included (the composition counts them too).  The ABI takes W_1 in the module's order, position columns first;
// inside, a pair's row is [features (c) | position (3)], so that every feature quad is 16-byte aligned (GmRow of group_mlp_shape.h).
//
// The flat pair list (B, M nsample) is a list of rows like any other: the passes, the statistics, the saved state and the rules are
// fp_mlp_bn.hip's, through the shared fp_mlp_bn_pass.h -- a wave owns 32 pair rows, four waves per workgroup, one workgroup per 128
// rows, no persistent loop.  Liveness is FpRow's with n = M nsample and ulen = clamp(qlen) nsample (gbn_ulen_kernel).  What is this
// unit's own:
//   GbnGather            layer 1's input: one feature row per pair loaded straight into the k-step layout, the relative coordinates
//                        formed in registers in the quad at column c;
//   gbn_pool_kernel      out[p] = pool_j ReLU(bn_y(a, z_L, c)) over the centre's nsample consecutive rows, zeros for a padded centre;
//   gbn_gy_last_kernel   the pool's backward with the same bn_y expression: max sends g[p, ch] to the LOWEST j with
//                        h_(L,j)[ch] == out[p, ch] (F.max_pool2d's rule; a pooled value <= 0 sends nothing), mean sends g[p] / nsample
//                        through the ReLU mask; gy_L per pair and the partials of its sums, a fixed set of centres per workgroup;
//   gbn_new_xyz_kernel   grad_new_xyz[p] = -sum_j dx[position] in slot order.
// dx goes per pair to the workspace as (pairs, c) | (pairs, 3); the scatters are mcp_group_rows_grad_sorted over the caller's
// (order, seg), the weight sums mcp_linear_wgrad (dW_1 in the internal order, then laid into [position | features]):
// gm_backward_tail of group_mlp_tile.h, which mcp_group_mlp_grad ends with too.  The same header holds what else the unit shares
// with group_mlp.hip and group_mlp_grad.hip: the supported shapes (gm_supported), which centres are live (gm_centre_live), the two
// pack kernels and the backward-only parts of the workspace (gm_back_layout).
//
// No atomics, every sum in a fixed order, two calls give identical bits; the variance is Chan-merged; no activation is kept between
// forward and backward; a padded centre's float inputs, grad_out included, are never read, it takes part in no statistic and writes
// zeros to its rows of out, grad_new_xyz and dx; with a live count below 2 every division is by max(m, 1).  No allocation, no
// environment variable, no host read of a length.
//
// Image (mcp_group_mlp_bn_pack), one for both directions, from the unfolded (W_l, b_l): [forward slabs | biases] [backward slabs] in
// the order and operand layouts of mcp_fp_mlp_grad_pack for a layer-1 input of c + 3 contiguous columns.
//
// Built WITHOUT -fno-honor-nans: a training kernel.
#include "fp_mlp_bn_pass.h"
#include "group_mlp_tile.h"

namespace {

// The set-abstraction layer's names for the shared pass arguments:  n = M nsample,  m = N (points of a cloud),  c2 = c,  c1 = 3 with
// use_xyz else 0,  rule = nsample;  known_feats = features (B, N, c),  skip = xyz (B, N, 3),  dist = new_xyz (B, M, 3),
// idx = idx (B, M, nsample);  w3, w_used unused.
struct GbnRaw {
    float4 a0, a1;
};
struct GbnGather {
    typedef GbnRaw Raw;
    const float *frow = nullptr;
    float4 rel = make_float4(0.f, 0.f, 0.f, 0.f);   // xyz[k] - new_xyz[p], 0: zeros in a padded row
    bool inr = false, live = false;
    int c = 0, px = 0, ldx = 0, h = 0;

    __device__ __forceinline__ void begin(const FpRow &me, const BnArgs &a, const BnPtrs &q) {
        inr = me.inr; live = me.live;
        c = a.c2; px = a.c1;
        ldx = (c + px + 3) & ~3;
        h = (threadIdx.x & 63) >> 5;
        frow = q.known_feats;
        if (live) {
            const long long src = me.bb * a.m + q.idx[me.p];
            frow = q.known_feats + src * c;
            if (px) {
                const long long centre = mcp_div(me.p, a.rule, mcp_fits32(a.total));
                const float *xr = q.skip + src * 3, *nr = q.dist + centre * 3;
                rel = make_float4(xr[0] - nr[0], xr[1] - nr[1], xr[2] - nr[2], 0.f);
            }
        }
    }
    // input k-step s: the two quads at columns 16 s + 4 h and 16 s + 8 + 4 h of the pair's row; only feature quads are loads
    __device__ __forceinline__ Raw fetch(int s) const {
        const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
        Raw r{z4, z4};
        if (live) {
            const int ch0 = 16 * s + 4 * h, ch1 = ch0 + 8;
            if (ch0 < c) r.a0 = *reinterpret_cast<const float4 *>(frow + ch0);
            if (ch1 < c) r.a1 = *reinterpret_cast<const float4 *>(frow + ch1);
        }
        return r;
    }
    __device__ __forceinline__ McpSplit3 finish(const Raw &r, int s, float *__restrict__ x, long long p) const {
        const int ch0 = 16 * s + 4 * h, ch1 = ch0 + 8;
        const float4 q0 = (px && ch0 == c) ? rel : r.a0, q1 = (px && ch1 == c) ? rel : r.a1;
        const float v[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
        if (x && inr) {   // rows of x hold ldx floats: c + 3 rounded up to whole quads
            if (ch0 < ldx) *reinterpret_cast<float4 *>(x + p * ldx + ch0) = q0;
            if (ch1 < ldx) *reinterpret_cast<float4 *>(x + p * ldx + ch1) = q1;
        }
        return mcp_split8(v);
    }
};

// ulen[bb] = clamp(qlen[bb], 0, M) nsample: the live pair rows of cloud bb
__global__ __launch_bounds__(64) void gbn_ulen_kernel(int b, int m, int nsample, const int *__restrict__ qlen, int *__restrict__ ulen) {
    for (int i = threadIdx.x; i < b; i += 64) ulen[i] = min(max(qlen[i], 0), m) * nsample;
}

__device__ __forceinline__ bool gbn_centre_live(long long pc, long long centres, int m, const int *__restrict__ qlen) {
    return gm_centre_live(pc, qlen ? mcp_div(pc, m, mcp_fits32(centres)) : 0, m, qlen);
}

// out[p] = pool_j ReLU(a z_L + c) over the centre's nsample rows, in slot order; zeros for a padded centre: one quad per thread
__global__ __launch_bounds__(256) void gbn_pool_kernel(long long centres, int m, int nsample, int c, int pool, const int *__restrict__ qlen,
                                                       const float *__restrict__ z, const float *__restrict__ coef, float *__restrict__ out) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    const int quads = c >> 2;
    if (e >= centres * quads) return;
    const long long pc = mcp_div(e, quads, mcp_fits32(centres * quads));
    const int ch = 4 * (int)(e - pc * quads);
    float o[4] = {0.f, 0.f, 0.f, 0.f};
    if (gbn_centre_live(pc, centres, m, qlen)) {
        const float4 ka = *reinterpret_cast<const float4 *>(coef + ch), kc = *reinterpret_cast<const float4 *>(coef + c + ch);
        const float av[4] = {ka.x, ka.y, ka.z, ka.w}, cv[4] = {kc.x, kc.y, kc.z, kc.w};
        const float *zr = z + pc * nsample * c + ch;
        for (int j = 0; j < nsample; ++j) {
            const float4 zq = *reinterpret_cast<const float4 *>(zr + (size_t)j * c);
            const float zv[4] = {zq.x, zq.y, zq.z, zq.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float y = bn_y(av[i], zv[i], cv[i]);
                const float hv = y > 0.f ? y : 0.f;
                if (pool == 0) o[i] = hv > o[i] ? hv : o[i];
                else o[i] += hv;
            }
        }
        if (pool != 0) {
#pragma unroll
            for (int i = 0; i < 4; ++i) o[i] = o[i] / (float)nsample;
        }
    }
    *reinterpret_cast<float4 *>(out + pc * c + ch) = make_float4(o[0], o[1], o[2], o[3]);
}

// gy_L per pair with the partials of sum gy_L, sum gy_L zhat_L and sum (z_L - mu_L).  A workgroup takes `cpw` consecutive centres; a
// thread owns one channel quad and every (1024 / C)-th of them, in ascending order, each centre's slots in ascending order; the centre
// subsets are then added in order.  The winner of a channel is found over recomputed values (first loop), so the forward's out is not
// read; the strict comparison keeps the lowest slot of a tie.
__global__ __launch_bounds__(256) void gbn_gy_last_kernel(long long centres, int m, int nsample, int c, int pool, int cpw, const int *__restrict__ qlen,
                                                          const float *__restrict__ z, const float *__restrict__ coef,
                                                          const float *__restrict__ grad_out, float *__restrict__ gy, float *__restrict__ part) {
    __shared__ float acc[3072];   // [subset][3][C] with 1024 / C subsets
    const int quads = c >> 2, subsets = 256 / quads;
    const int ch = 4 * (threadIdx.x % quads), sub = threadIdx.x / quads;
    const float4 ka = *reinterpret_cast<const float4 *>(coef + ch), kc = *reinterpret_cast<const float4 *>(coef + c + ch);
    const float4 km = *reinterpret_cast<const float4 *>(coef + 2 * c + ch), kr = *reinterpret_cast<const float4 *>(coef + 3 * c + ch);
    const float av[4] = {ka.x, ka.y, ka.z, ka.w}, cv[4] = {kc.x, kc.y, kc.z, kc.w}, mv[4] = {km.x, km.y, km.z, km.w}, rv[4] = {kr.x, kr.y, kr.z, kr.w};
    float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f}, s3[4] = {0.f, 0.f, 0.f, 0.f};
    for (int r = sub; r < cpw; r += subsets) {
        const long long pc = (long long)blockIdx.x * cpw + r;
        if (pc >= centres) break;
        const float *zr = z + pc * nsample * c + ch;
        float *gr = gy + pc * nsample * c + ch;
        if (!gbn_centre_live(pc, centres, m, qlen)) {
            for (int j = 0; j < nsample; ++j) *reinterpret_cast<float4 *>(gr + (size_t)j * c) = make_float4(0.f, 0.f, 0.f, 0.f);
            continue;
        }
        const float4 gq = *reinterpret_cast<const float4 *>(grad_out + pc * c + ch);
        const float gv[4] = {gq.x, gq.y, gq.z, gq.w};
        float best[4] = {-1.f, -1.f, -1.f, -1.f}, share[4];
        int win[4] = {0, 0, 0, 0};
        if (pool == 0) {
            for (int j = 0; j < nsample; ++j) {
                const float4 zq = *reinterpret_cast<const float4 *>(zr + (size_t)j * c);
                const float zv[4] = {zq.x, zq.y, zq.z, zq.w};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float y = bn_y(av[i], zv[i], cv[i]);
                    const float hv = y > 0.f ? y : 0.f;
                    if (hv > best[i]) { best[i] = hv; win[i] = j; }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) share[i] = gv[i] / (float)nsample;
        for (int j = 0; j < nsample; ++j) {
            const float4 zq = *reinterpret_cast<const float4 *>(zr + (size_t)j * c);
            const float zv[4] = {zq.x, zq.y, zq.z, zq.w};
            float o[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (pool == 0) o[i] = (j == win[i] && best[i] > 0.f) ? gv[i] : 0.f;
                else o[i] = bn_y(av[i], zv[i], cv[i]) > 0.f ? share[i] : 0.f;
                s1[i] += o[i];
                s2[i] += o[i] * ((zv[i] - mv[i]) * rv[i]);
                s3[i] += zv[i] - mv[i];
            }
            *reinterpret_cast<float4 *>(gr + (size_t)j * c) = make_float4(o[0], o[1], o[2], o[3]);
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        acc[(sub * 3 + 0) * c + ch + j] = s1[j];
        acc[(sub * 3 + 1) * c + ch + j] = s2[j];
        acc[(sub * 3 + 2) * c + ch + j] = s3[j];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < 3 * c; e += 256) {
        float s = acc[e];
        for (int u = 1; u < subsets; ++u) s += acc[u * 3 * c + e];
        part[(size_t)blockIdx.x * 3 * c + e] = s;
    }
}

// grad_new_xyz[p] = -sum_j dx[p, j][position], slots in ascending order (a padded centre's rows of dx are zeros)
__global__ __launch_bounds__(256) void gbn_new_xyz_kernel(long long centres, int nsample, const float *__restrict__ dxp, float *__restrict__ grad_new_xyz) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= centres * 3) return;
    const long long pc = mcp_div(e, 3, mcp_fits32(centres * 3));
    const int k = (int)(e - pc * 3);
    float s = 0.f;
    for (int j = 0; j < nsample; ++j) s += dxp[(pc * nsample + j) * 3 + k];
    grad_new_xyz[e] = 0.f - s;
}

// ---- host side ----
struct GbnShape {
    FgShape g;          // the shared passes' shape: a layer-1 input of ldx contiguous columns (c2 = ldx, c1 = 0)
    GmRow x;
};
// false: outside mcp_group_mlp's supported set
inline bool gbn_shape(int c, int use_xyz, int layers, const int *widths, GbnShape *s) {
    return gm_supported(c, use_xyz, layers, widths, &s->x) && fg_shape(s->x.ldx, 0, layers, widths, &s->g);
}
inline size_t gbn_image_floats(const GbnShape &s) { return ((size_t)s.g.f.w_u4 + s.g.bwd_u4) * 4 + s.g.f.small_floats; }

// centres of one workgroup of gbn_gy_last_kernel: whole rounds of its 1024 / C centre subsets, and at least 128 pair rows, so that its
// workgroups are no more than the passes' and its partials fit the passes' part
inline int gbn_cpw(int nsample, int c_last) {
    const int subsets = 1024 / c_last, least = (32 * WAVES + nsample - 1) / nsample;
    return subsets * ((least + subsets - 1) / subsets);
}

// The caller-owned workspace: byte offsets of its parts, each 256-byte aligned.
struct GbnLayout {
    size_t z[MAX_LAYERS], coef[MAX_LAYERS], part, part_cnt, count, ulen;             // forward and backward
    size_t gy[MAX_LAYERS];                                                           // backward only: gy_l, then
    GmBack back;                                                                     // x, h_l, gz_l, dx and the weight sums' parts
    size_t bytes;
};
// false: mcp_linear_wgrad does not take one of the layers' products
inline bool gbn_layout(int b, long long total, const GbnShape &s, const int *widths, bool backward, GbnLayout *l) {
    FpTake take;
    const size_t rows = (size_t)total, groups = (size_t)((total + 32 * WAVES - 1) / (32 * WAVES));
    const int layers = s.g.f.layers;
    int widest = 0;
    for (int i = 0; i < layers; ++i) widest = widths[i] > widest ? widths[i] : widest;
    for (int i = 0; i < MAX_LAYERS; ++i) l->z[i] = take(i < layers ? rows * widths[i] : 0);
    for (int i = 0; i < MAX_LAYERS; ++i) l->coef[i] = take(i < layers ? (size_t)COEF * widths[i] : 0);
    l->part = take(groups * 3 * widest);
    l->part_cnt = take(groups);
    l->count = take(1);
    l->ulen = take((size_t)b);
    if (backward) {
        for (int i = 0; i < MAX_LAYERS; ++i) l->gy[i] = take(i < layers ? rows * widths[i] : 0);
        if (!gm_back_layout(take, total, s.x, layers, widths, &l->back)) return false;
    }
    l->bytes = take.at;
    return true;
}

// c.sh is set: the layout, the sizes, what every pass shares, the clouds' live rows and the live count
int gbn_prepare(BnCall &c, GbnLayout &lay, const GbnShape &sh, int b, int n, int m, int nsample, const int *widths, bool backward, const int *qlen,
                int *count, void *workspace, size_t workspace_bytes, mcp_stream_t stream) {
    if ((long long)m * nsample > 0x7FFFFFFFLL) return MCP_ERR_UNSUPPORTED;
    c.sh = sh.g;
    c.total = (long long)b * m * nsample;
    if (!gbn_layout(b, c.total, sh, widths, backward, &lay)) return MCP_ERR_UNSUPPORTED;
    if (workspace_bytes < lay.bytes) return MCP_ERR_BAD_ARG;
    const long long groups = (c.total + 32 * WAVES - 1) / (32 * WAVES);
    if (groups > 0x7FFFFFFFLL / (2 * 256)) return MCP_ERR_UNSUPPORTED;   // the partials are indexed in 32 bits per workgroup row
    c.groups = (int)groups;
    c.ws = reinterpret_cast<char *>(workspace);
    c.s = (hipStream_t)stream;
    c.a = BnArgs{};
    c.a.total = c.total;
    c.a.n = m * nsample; c.a.m = n; c.a.c2 = sh.x.c; c.a.c1 = sh.x.px; c.a.rule = nsample;
    c.a.ksb = sh.g.f.ksb;
    c.q = BnPtrs{};
    c.q.part = c.part(lay.part);
    c.q.part_cnt = reinterpret_cast<int *>(c.ws + lay.part_cnt);
    for (int l = 0; l < MAX_LAYERS; ++l) {
        c.z[l] = c.part(lay.z[l]);
        c.coef[l] = c.part(lay.coef[l]);
        c.gy[l] = backward ? c.part(lay.gy[l]) : nullptr;
        c.gz[l] = backward ? c.part(lay.back.gz[l]) : nullptr;
    }
    int *ulen = nullptr;
    if (qlen) {
        ulen = reinterpret_cast<int *>(c.ws + lay.ulen);
        hipLaunchKernelGGL(gbn_ulen_kernel, dim3(1), dim3(64), 0, c.s, b, m, nsample, qlen, ulen);
        const int rc = mcp_launch_status();
        if (rc != MCP_OK) return rc;
    }
    c.q.ulen = ulen;
    hipLaunchKernelGGL(fpbn_count_kernel, dim3(1), dim3(64), 0, c.s, b, m * nsample, ulen, count ? count : reinterpret_cast<int *>(c.ws + lay.count));
    return mcp_launch_status();
}

}  // namespace

MCP_EXPORT int mcp_group_mlp_bn_packed_floats(int c, int use_xyz, int layers, const int *widths) {
    GbnShape sh;
    if (!gbn_shape(c, use_xyz, layers, widths, &sh)) return 0;
    return (int)gbn_image_floats(sh);
}

MCP_EXPORT int mcp_group_mlp_bn_pack(int c, int use_xyz, int layers, const int *widths, const float *const *w, const float *const *b, float *packed,
                                     mcp_stream_t stream) {
    MCP_CHECK_ARGS(widths && w && b && packed);
    GbnShape sh;
    if (!gbn_shape(c, use_xyz, layers, widths, &sh)) return MCP_ERR_UNSUPPORTED;
    for (int l = 0; l < layers; ++l) MCP_CHECK_ARGS(w[l] && b[l]);
    if (((uintptr_t)packed) & 15) return MCP_ERR_BAD_ARG;
    const FpShape &f = sh.g.f;
    hipStream_t s = (hipStream_t)stream;
    uint4 *pw = reinterpret_cast<uint4 *>(packed);
    float *small = packed + (size_t)f.w_u4 * 4;
    int rc;
    // Slabs: a k-step's entries lie together, [s][t].  Column j of a pair's row is W_1's column px + j for j < c (features), j - c for
    // the px position columns behind them; a later layer's input is its features alone.
    for (int l = 0; l < layers; ++l) {   // [forward slabs | biases]
        const int ld = l == 0 ? sh.x.cin : widths[l - 1], px = l == 0 ? sh.x.px : 0;
        if ((rc = gm_pack_fwd(s, w[l], b[l], ld, px, ld - px, px, f.ks[l], f.tiles[l], 1, f.tiles[l], pw, nullptr, small + f.boff[l])) != MCP_OK) return rc;
        pw += (size_t)f.tiles[l] * f.ks[l] * TILE_U4;
    }
    pw = reinterpret_cast<uint4 *>(packed + (size_t)f.w_u4 * 4 + f.small_floats);
    for (int l = layers - 1; l >= 1; --l)
        if ((rc = gm_pack_bwd(s, w[l], widths[l - 1], widths[l - 1], 0, 0, f.tiles[l - 1], 2 * f.tiles[l], 1, f.tiles[l - 1], pw)) != MCP_OK) return rc;
    for (int c0 = 0; c0 < sh.g.dxt; c0 += f.tmax) {   // dx in chunks of tmax output tiles, as BWD_DX takes them
        const int tc = sh.g.dxt - c0 < f.tmax ? sh.g.dxt - c0 : f.tmax;
        if ((rc = gm_pack_bwd(s, w[0], sh.x.cin, c, sh.x.px, c0, tc, 2 * f.tiles[0], 1, tc, pw)) != MCP_OK) return rc;
    }
    return MCP_OK;
}

MCP_EXPORT size_t mcp_group_mlp_bn_workspace_bytes(int b, int m, int c, int nsample, int use_xyz, int layers, const int *widths, int backward) {
    GbnShape sh;
    if (b <= 0 || m <= 0 || nsample < 1 || nsample > 64 || !gbn_shape(c, use_xyz, layers, widths, &sh)) return 0;
    GbnLayout lay;
    return gbn_layout(b, (long long)b * m * nsample, sh, widths, backward != 0, &lay) ? lay.bytes : 0;
}

MCP_EXPORT int mcp_group_mlp_bn_forward(int b, int n, int m, int c, int nsample, int use_xyz, int pool, int layers, const int *widths, const float *xyz,
                                        const float *new_xyz, const float *features, const int *idx, const int *qlen, const float *packed,
                                        const float *const *gamma, const float *const *beta, const float *eps, float *out, float *const *mean,
                                        float *const *var, float *const *rstd, int *count, void *workspace, size_t workspace_bytes,
                                        mcp_stream_t stream) {
    MCP_CHECK_ARGS(b > 0 && n > 0 && m > 0 && widths && idx && packed && gamma && beta && eps && out && mean && var && rstd && count && workspace &&
                   (pool == 0 || pool == 1));
    MCP_CHECK_ARGS((!use_xyz || (xyz && new_xyz)) && (c <= 0 || features));
    GbnShape sh;
    if (!gbn_shape(c, use_xyz, layers, widths, &sh) || nsample < 1 || nsample > 64) return MCP_ERR_UNSUPPORTED;
    for (int l = 0; l < layers; ++l) MCP_CHECK_ARGS(mean[l] && var[l] && rstd[l] && eps[l] > 0.f);
    if (((uintptr_t)features | (uintptr_t)out | (uintptr_t)packed | (uintptr_t)workspace) & 15) return MCP_ERR_BAD_ARG;
    BnCall call;
    GbnLayout lay;
    int rc = gbn_prepare(call, lay, sh, b, n, m, nsample, widths, false, qlen, count, workspace, workspace_bytes, stream);
    if (rc != MCP_OK) return rc;
    call.q.known_feats = features; call.q.skip = xyz; call.q.dist = new_xyz; call.q.idx = idx; call.q.packed = packed;
    for (int l = 0; l < layers; ++l) {
        if ((rc = forward_pass<GbnGather>(call, l, widths, true, nullptr)) != MCP_OK) return rc;
        hipLaunchKernelGGL(fpbn_stats_reduce_kernel, dim3(widths[l]), dim3(REDUCE_THREADS), 0, call.s, call.groups, widths[l], call.q.part, call.q.part_cnt,
                           gamma[l], beta[l], eps[l], mean[l], var[l], rstd[l], call.coef[l]);
        if ((rc = mcp_launch_status()) != MCP_OK) return rc;
    }
    const int cl = widths[layers - 1];
    const long long centres = (long long)b * m, quads = centres * (cl / 4);
    hipLaunchKernelGGL(gbn_pool_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, call.s, centres, m, nsample, cl, pool, qlen, call.z[layers - 1],
                       call.coef[layers - 1], out);
    return mcp_launch_status();
}

MCP_EXPORT int mcp_group_mlp_bn_backward(int b, int n, int m, int c, int nsample, int use_xyz, int pool, int layers, const int *widths, const float *xyz,
                                         const float *new_xyz, const float *features, const int *idx, const int *qlen, const float *packed,
                                         const float *const *gamma, const float *const *beta, const float *const *mean, const float *const *rstd,
                                         const float *grad_out, const int *order, const int *seg, float *grad_features, float *grad_xyz,
                                         float *grad_new_xyz, float *const *grad_w, float *const *grad_b, float *const *grad_gamma,
                                         float *const *grad_beta, void *workspace, size_t workspace_bytes, mcp_stream_t stream) {
    MCP_CHECK_ARGS(b > 0 && n > 0 && m > 0 && widths && idx && packed && gamma && beta && mean && rstd && grad_out && grad_w && grad_b && grad_gamma &&
                   grad_beta && workspace && (pool == 0 || pool == 1));
    MCP_CHECK_ARGS((!use_xyz || (xyz && new_xyz)) && (c <= 0 || features) && (!(grad_features || grad_xyz) || (order && seg)));
    MCP_CHECK_ARGS((!grad_features || c > 0) && (!(grad_xyz || grad_new_xyz) || use_xyz));
    GbnShape sh;
    if (!gbn_shape(c, use_xyz, layers, widths, &sh) || nsample < 1 || nsample > 64) return MCP_ERR_UNSUPPORTED;
    for (int l = 0; l < layers; ++l) MCP_CHECK_ARGS(grad_w[l] && mean[l] && rstd[l]);
    if (((uintptr_t)features | (uintptr_t)packed | (uintptr_t)grad_out | (uintptr_t)grad_features | (uintptr_t)workspace) & 15) return MCP_ERR_BAD_ARG;
    BnCall call;
    GbnLayout lay;
    int rc = gbn_prepare(call, lay, sh, b, n, m, nsample, widths, true, qlen, nullptr, workspace, workspace_bytes, stream);
    if (rc != MCP_OK) return rc;
    call.q.known_feats = features; call.q.skip = xyz; call.q.dist = new_xyz; call.q.idx = idx; call.q.packed = packed;
    float *x = call.part(lay.back.x), *hid[2] = {call.part(lay.back.hid[0]), call.part(lay.back.hid[1])};
    float *dxf = call.part(lay.back.dxf), *dxp = call.part(lay.back.dxp);
    const int *count = reinterpret_cast<const int *>(call.ws + lay.count);

    // ---- the forward again, statistics given: x, z_l, h_l ----
    for (int l = 0; l < layers; ++l) {
        hipLaunchKernelGGL(fpbn_coef_kernel, dim3((widths[l] + 255) / 256), dim3(256), 0, call.s, widths[l], gamma[l], beta[l], mean[l], rstd[l], call.coef[l]);
        if ((rc = mcp_launch_status()) != MCP_OK) return rc;
        if ((rc = forward_pass<GbnGather>(call, l, widths, false, l == 0 ? x : hid[l - 1])) != MCP_OK) return rc;
    }
    // ---- the pool's backward: gy_L and its sums ----
    const int last = layers - 1, cpw = gbn_cpw(nsample, widths[last]);
    const long long centres = (long long)b * m;
    const int groups_last = (int)((centres + cpw - 1) / cpw);
    hipLaunchKernelGGL(gbn_gy_last_kernel, dim3(groups_last), dim3(256), 0, call.s, centres, m, nsample, widths[last], pool, cpw, qlen, call.z[last],
                       call.coef[last], grad_out, call.gy[last], call.q.part);
    if ((rc = mcp_launch_status()) != MCP_OK) return rc;
    if ((rc = backward_passes<GbnGather>(call, widths, groups_last, count, grad_gamma, grad_beta, dxf, dxp)) != MCP_OK) return rc;

    if (grad_new_xyz) {
        hipLaunchKernelGGL(gbn_new_xyz_kernel, dim3((unsigned)((centres * 3 + 255) / 256)), dim3(256), 0, call.s, centres, nsample, dxp, grad_new_xyz);
        if ((rc = mcp_launch_status()) != MCP_OK) return rc;
    }
    // the scatters and the weight sums (db_l is zero in exact arithmetic: the statistics absorb a bias)
    return gm_backward_tail(b, n, m, nsample, sh.x, layers, widths, call.ws, lay.back, order, seg, grad_features, grad_xyz, grad_w, grad_b, stream);
}
