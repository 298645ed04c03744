// fp_mlp_bn.hip -- the fused feature-propagation layer of pointnet2 with TRAINING-MODE BatchNorm (batch statistics) for gfx950: forward
// and backward of  x = [three-neighbour blend | skip],  z_l = W_l h_(l-1) + b_l,  y_l = gamma_l (z_l - mu_l) rstd_l + beta_l,
// h_l = ReLU(y_l),  out = h_L,  with mu_l / v_l the mean and the biased variance of z_l over the live rows.  The blend, the rules,
// ulen and the infinite slots are those of mcp_fp_mlp (fp_mlp.hip); the tiling, the 3-way bf16 split and the operand images are
// those of fp_mlp.hip / fp_mlp_grad.hip (a wave owns 32 rows, the MFMA column; four waves per workgroup; one workgroup per 128 rows).
//
// A pass ends where the next quantity needs a sum over all rows.  One kernel template, fpbn_pass_kernel<TMAX, STREAM, MODE>, is one
// layer's product with what surrounds it (the template has the layer-1 gather as a further, first argument):
//   FWD_GATHER  h_0 from the gathered rows (FpGather of fp_mlp_tile.h: the forward's layer 1), z_1 = W_1 h_0 + b_1 to the workspace;
//   FWD_ROWS    h_(l-1) = ReLU(a z_(l-1) + c) formed ON LOAD from the stored z_(l-1) (a = gamma rstd, c = beta - mu a), z_l to the
//               workspace;
//     both accumulate, in their epilogue, one (count, mean, M2) triple per channel and workgroup;
//   BWD_MID     gz_l = p (gy_l - k1) + q (z_l - mu_l) formed ON LOAD from the stored gy_l and z_l (p = gamma rstd, k1 = dbeta / m,
//               q = -gamma rstd^2 dgamma / m), gh_(l-1) = W_l^T gz_l, gy_(l-1) = gh_(l-1) . [y_(l-1) > 0] to the workspace; its
//               epilogue accumulates sum gy_(l-1), sum gy_(l-1) zhat_(l-1) and sum (z_(l-1) - mu_(l-1)) per channel and workgroup;
//   BWD_DX      the same load for layer 1, dx = W_1^T gz_1 in chunks of TMAX output tiles -> grad_blend | grad_skip.
// Between the passes small kernels reduce the workgroups' partials (fpbn_stats_reduce_kernel -> mu, v, rstd, a, c;
// fpbn_sums_reduce_kernel -> dgamma, dbeta, p, k1, q); fpbn_out_kernel writes out = ReLU(a z_L + c); fpbn_gy_last_kernel forms
// gy_L = g . [y_L > 0] with its two sums.
//
// Statistics.  Every per-channel sum is taken per lane over the wave's 32 rows by a fixed butterfly, the four waves are merged in
// wave order, the workgroups in workgroup order (a fixed chunking); no atomics, two calls give identical bits.  The variance is NOT
// E[z^2] - E[z]^2: a wave takes the mean of its rows, then the sum of squared differences from THAT mean (two passes over values it
// holds in registers), and (count, mean, M2) triples are merged by Chan's update, whose correction term is the squared difference
// of two partial means.  A layer whose |mu| is a hundred times its sigma loses nothing to cancellation.  In the backward the
// fp32 mean's own rounding matters too: sum_R (z - mu) is -m times it, not zero, and dW = sum gz h^T would carry that times the mean
// of h.  The backward sums z - mu beside its two sums and folds lo = sum (z - mu) / m into k1 and dgamma (fpbn_sums_reduce_kernel).
//
// Saved state.  Between forward and backward the caller keeps the layer's inputs and the per-layer (mu, rstd) -- no activation.  The
// backward first runs the forward passes again with the statistics given (no epilogue sums; x, every h_l and z_l to the
// workspace), one pass per layer with (a, c) applied on load: the very kernels of the forward, so z_l has the forward's bits and
// every ReLU mask is the forward's.
//
// Padded rows (at or beyond ulen[bb]) write zeros, have none of their float inputs read and take part in no statistic.  A live
// count m below 2: every division is by max(m, 1), nothing is NaN or Inf, the statistics of such a call are meaningless.
//
// Weight and bias gradients: mcp_linear_wgrad over the stored gz_l and h_(l-1) (layer 1 in 256-column slices of x), the blend's
// scatter: mcp_interp3_apply_grad_sorted, both as mcp_fp_mlp_grad.  The images are mcp_fp_mlp_pack's (forward) and
// mcp_fp_mlp_grad_pack's (backward); fp_weights_in_lds / fg_whole decide, as there, between a layer's slabs staged whole in LDS and
// slabs streamed through two LDS buffers.
//
// Built WITHOUT -fno-honor-nans, as fp_mlp_grad.hip: masks and ReLU are comparisons and selections, a diverged run shows its NaN.
//
// The row, the gather, the slab sequence, the tile helpers and the dx epilogue are fp_mlp_tile.h's, shared with fp_mlp.hip and
// fp_mlp_grad.hip.  The pass kernel, the kernels between the passes and the host's walk over the layers are fp_mlp_bn_pass.h's, shared
// with group_mlp_bn.hip (the set-abstraction layer, whose rows are (centre, slot) pairs); this unit keeps fpbn_out_kernel,
// fpbn_gy_last_kernel, its workspace layout and its entry points.
#include "fp_mlp_bn_pass.h"

namespace {

// out = ReLU(a z_L + c), zeros in a padded row: one quad per thread
__global__ __launch_bounds__(256) void fpbn_out_kernel(long long total, int n, int c, const int *__restrict__ ulen, const float *__restrict__ z,
                                                       const float *__restrict__ coef, float *__restrict__ out) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    const int quads = c >> 2;
    if (e >= total * quads) return;
    const long long p = mcp_div(e, quads, mcp_fits32(total * quads));
    const int ch = 4 * (int)(e - p * quads);
    bool live = true;
    if (ulen) {
        const long long bb = mcp_div(p, n, mcp_fits32(total));
        live = (int)(p - bb * n) < min(max(ulen[bb], 0), n);
    }
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live) {
        const float4 zq = *reinterpret_cast<const float4 *>(z + p * c + ch);
        const float4 ka = *reinterpret_cast<const float4 *>(coef + ch), kc = *reinterpret_cast<const float4 *>(coef + c + ch);
        const float y0 = bn_y(ka.x, zq.x, kc.x), y1 = bn_y(ka.y, zq.y, kc.y), y2 = bn_y(ka.z, zq.z, kc.z), y3 = bn_y(ka.w, zq.w, kc.w);
        o = make_float4(y0 > 0.f ? y0 : 0.f, y1 > 0.f ? y1 : 0.f, y2 > 0.f ? y2 : 0.f, y3 > 0.f ? y3 : 0.f);
    }
    *reinterpret_cast<float4 *>(out + p * c + ch) = o;
}

// gy_L = g . [y_L > 0] with the partials of its sums (and of sum (z_L - mu_L), see fpbn_sums_reduce_kernel).  A workgroup takes the pass kernel's 128 rows; a thread owns one channel
// quad and every (1024 / C)-th row, in ascending order; the row subsets are then added in order.
__global__ __launch_bounds__(256) void fpbn_gy_last_kernel(long long total, int n, int c, const int *__restrict__ ulen, const float *__restrict__ z,
                                                           const float *__restrict__ coef, const float *__restrict__ grad_out, float *__restrict__ gy,
                                                           float *__restrict__ part) {
    __shared__ float acc[3072];   // [subset][3][C] with 1024 / C subsets
    const int quads = c >> 2, subsets = 256 / quads;
    const int ch = 4 * (threadIdx.x % quads), sub = threadIdx.x / quads;
    const float4 ka = *reinterpret_cast<const float4 *>(coef + ch), kc = *reinterpret_cast<const float4 *>(coef + c + ch);
    const float4 km = *reinterpret_cast<const float4 *>(coef + 2 * c + ch), kr = *reinterpret_cast<const float4 *>(coef + 3 * c + ch);
    const float av[4] = {ka.x, ka.y, ka.z, ka.w}, cv[4] = {kc.x, kc.y, kc.z, kc.w}, mv[4] = {km.x, km.y, km.z, km.w}, rv[4] = {kr.x, kr.y, kr.z, kr.w};
    float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f}, s3[4] = {0.f, 0.f, 0.f, 0.f};
    for (int r = sub; r < 32 * WAVES; r += subsets) {
        const long long p = (long long)blockIdx.x * (32 * WAVES) + r;
        if (p >= total) break;
        bool live = true;
        if (ulen) {
            const long long bb = mcp_div(p, n, mcp_fits32(total));
            live = (int)(p - bb * n) < min(max(ulen[bb], 0), n);
        }
        float o[4] = {0.f, 0.f, 0.f, 0.f};
        if (live) {
            const float4 zq = *reinterpret_cast<const float4 *>(z + p * c + ch), gq = *reinterpret_cast<const float4 *>(grad_out + p * c + ch);
            const float zv[4] = {zq.x, zq.y, zq.z, zq.w}, gv[4] = {gq.x, gq.y, gq.z, gq.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                o[j] = bn_y(av[j], zv[j], cv[j]) > 0.f ? gv[j] : 0.f;
                s1[j] += o[j];
                s2[j] += o[j] * ((zv[j] - mv[j]) * rv[j]);
                s3[j] += zv[j] - mv[j];
            }
        }
        *reinterpret_cast<float4 *>(gy + p * c + ch) = make_float4(o[0], o[1], o[2], o[3]);
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

// The caller-owned workspace: byte offsets of its parts, each 256-byte aligned.
struct BnLayout {
    size_t z[MAX_LAYERS], coef[MAX_LAYERS], part, part_cnt, count;                     // forward and backward
    size_t x, h1, h2, gy[MAX_LAYERS], gz[MAX_LAYERS], grad_blend, w_used, dw_slice, wgrad, wgrad_bytes;   // backward only
    size_t bytes;
};
// false: mcp_linear_wgrad does not take one of the layers' products
inline bool bn_layout(long long total, const FgShape &s, const int *widths, bool backward, BnLayout *l) {
    FpTake take;
    const size_t rows = (size_t)total, groups = (size_t)((total + 32 * WAVES - 1) / (32 * WAVES));
    const int layers = s.f.layers;
    int widest = 0;
    for (int i = 0; i < layers; ++i) widest = widths[i] > widest ? widths[i] : widest;
    for (int i = 0; i < MAX_LAYERS; ++i) l->z[i] = take(i < layers ? rows * widths[i] : 0);
    for (int i = 0; i < MAX_LAYERS; ++i) l->coef[i] = take(i < layers ? (size_t)COEF * widths[i] : 0);
    l->part = take(groups * 3 * widest);
    l->part_cnt = take(groups);
    l->count = take(1);
    l->wgrad = take.at;
    l->wgrad_bytes = 0;
    if (backward) {
        l->x = take(rows * s.cin);
        l->h1 = take(layers >= 2 ? rows * widths[0] : 0);
        l->h2 = take(layers >= 3 ? rows * widths[1] : 0);
        for (int i = 0; i < MAX_LAYERS; ++i) l->gy[i] = take(i < layers ? rows * widths[i] : 0);
        for (int i = 0; i < MAX_LAYERS; ++i) l->gz[i] = take(i < layers ? rows * widths[i] : 0);
        l->grad_blend = take(rows * s.f.c2);
        l->w_used = take(rows * 3);
        l->dw_slice = take(s.cin > WGRAD_COLS ? (size_t)widths[0] * WGRAD_COLS : 0);
        if (!fp_wgrad_bytes(total, s, widths, &l->wgrad_bytes)) return false;
        l->wgrad = take.at;
        take.at += FpTake::up(l->wgrad_bytes);
    }
    l->bytes = take.at;
    return true;
}

// c.sh is set: the layout, the sizes and what every pass shares
int prepare_call(BnCall &c, BnLayout &lay, int b, int n, int m, int c2, int c1, int rule, const int *widths, bool backward, void *workspace,
                 size_t workspace_bytes, mcp_stream_t stream) {
    c.total = (long long)b * n;
    if (!bn_layout(c.total, c.sh, widths, backward, &lay)) return MCP_ERR_UNSUPPORTED;
    if (workspace_bytes < lay.bytes) return MCP_ERR_BAD_ARG;
    const long long groups = (c.total + 32 * WAVES - 1) / (32 * WAVES);
    if (groups > 0x7FFFFFFFLL / (2 * 256)) return MCP_ERR_UNSUPPORTED;   // the partials are indexed in 32 bits per workgroup row
    c.groups = (int)groups;
    c.ws = reinterpret_cast<char *>(workspace);
    c.s = (hipStream_t)stream;
    c.a = BnArgs{};
    c.a.total = c.total;
    c.a.n = n; c.a.m = m; c.a.c2 = c2; c.a.c1 = c1; c.a.rule = rule;
    c.a.ksb = c.sh.f.ksb;
    c.q = BnPtrs{};
    c.q.part = c.part(lay.part);
    c.q.part_cnt = reinterpret_cast<int *>(c.ws + lay.part_cnt);
    for (int l = 0; l < MAX_LAYERS; ++l) {
        c.z[l] = c.part(lay.z[l]);
        c.coef[l] = c.part(lay.coef[l]);
        c.gy[l] = backward ? c.part(lay.gy[l]) : nullptr;
        c.gz[l] = backward ? c.part(lay.gz[l]) : nullptr;
    }
    return MCP_OK;
}

}  // namespace

MCP_EXPORT size_t mcp_fp_mlp_bn_workspace_bytes(int b, int n, int c2, int c1, int layers, const int *widths, int backward) {
    FgShape sh;
    if (b <= 0 || n <= 0 || !fg_shape(c2, c1, layers, widths, &sh)) return 0;
    BnLayout lay;
    return bn_layout((long long)b * n, sh, widths, backward != 0, &lay) ? lay.bytes : 0;
}

MCP_EXPORT int mcp_fp_mlp_bn_forward(int b, int n, int m, int c2, int c1, int rule, int layers, const int *widths, const float *known_feats,
                                     const float *skip, const int *idx, const float *dist, const float *w3, const int *ulen, const float *packed,
                                     const float *const *gamma, const float *const *beta, const float *eps, float *out, float *const *mean,
                                     float *const *var, float *const *rstd, int *count, void *workspace, size_t workspace_bytes,
                                     mcp_stream_t stream) {
    MCP_CHECK_ARGS(b > 0 && n > 0 && m > 0 && widths && known_feats && idx && packed && gamma && beta && eps && out && mean && var && rstd && count &&
                   workspace && rule >= 0 && rule <= 2);
    MCP_CHECK_ARGS((c1 <= 0 || skip) && (rule == 0 ? w3 != nullptr : dist != nullptr));
    BnCall c;
    if (!fg_shape(c2, c1, layers, widths, &c.sh)) return MCP_ERR_UNSUPPORTED;
    for (int l = 0; l < layers; ++l) MCP_CHECK_ARGS(mean[l] && var[l] && rstd[l] && eps[l] > 0.f);
    if (((uintptr_t)known_feats | (uintptr_t)out | (uintptr_t)packed | (uintptr_t)workspace | ((c1 & 3) == 0 ? (uintptr_t)skip : 0)) & 15) return MCP_ERR_BAD_ARG;
    BnLayout lay;
    int rc = prepare_call(c, lay, b, n, m, c2, c1, rule, widths, false, workspace, workspace_bytes, stream);
    if (rc != MCP_OK) return rc;
    c.q.known_feats = known_feats; c.q.skip = skip; c.q.idx = idx; c.q.dist = dist; c.q.w3 = w3; c.q.ulen = ulen; c.q.packed = packed;
    hipLaunchKernelGGL(fpbn_count_kernel, dim3(1), dim3(64), 0, c.s, b, n, ulen, count);
    if ((rc = mcp_launch_status()) != MCP_OK) return rc;
    for (int l = 0; l < layers; ++l) {
        if ((rc = forward_pass<FpBnGather>(c, l, widths, true, nullptr)) != MCP_OK) return rc;
        hipLaunchKernelGGL(fpbn_stats_reduce_kernel, dim3(widths[l]), dim3(REDUCE_THREADS), 0, c.s, c.groups, widths[l], c.q.part, c.q.part_cnt, gamma[l], beta[l],
                           eps[l], mean[l], var[l], rstd[l], c.coef[l]);
        if ((rc = mcp_launch_status()) != MCP_OK) return rc;
    }
    const int cl = widths[layers - 1];
    const long long quads = c.total * (cl / 4);
    if ((quads + 255) / 256 > 0x7FFFFFFFLL) return MCP_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(fpbn_out_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, c.s, c.total, n, cl, ulen, c.z[layers - 1],
                       c.coef[layers - 1], out);
    return mcp_launch_status();
}

MCP_EXPORT int mcp_fp_mlp_bn_backward(int b, int n, int m, int c2, int c1, int rule, int layers, const int *widths, const float *known_feats,
                                      const float *skip, const int *idx, const float *dist, const float *w3, const int *ulen, const float *packed,
                                      const float *const *gamma, const float *const *beta, const float *const *mean, const float *const *rstd,
                                      const float *grad_out, const int *order, const int *seg, float *grad_known_feats, float *grad_skip,
                                      float *const *grad_w, float *const *grad_b, float *const *grad_gamma, float *const *grad_beta, void *workspace,
                                      size_t workspace_bytes, mcp_stream_t stream) {
    MCP_CHECK_ARGS(b > 0 && n > 0 && m > 0 && widths && known_feats && idx && packed && gamma && beta && mean && rstd && grad_out && grad_w && grad_b &&
                   grad_gamma && grad_beta && workspace && rule >= 0 && rule <= 2);
    MCP_CHECK_ARGS((c1 <= 0 || (skip && grad_skip)) && (rule == 0 ? w3 != nullptr : dist != nullptr) && (!grad_known_feats || (order && seg)));
    BnCall c;
    if (!fg_shape(c2, c1, layers, widths, &c.sh)) return MCP_ERR_UNSUPPORTED;
    for (int l = 0; l < layers; ++l) MCP_CHECK_ARGS(grad_w[l] && mean[l] && rstd[l]);
    const uintptr_t quads = (uintptr_t)known_feats | (uintptr_t)packed | (uintptr_t)grad_out | (uintptr_t)workspace |
                            ((c1 & 3) == 0 ? (uintptr_t)skip | (uintptr_t)grad_skip : 0);
    if (quads & 15) return MCP_ERR_BAD_ARG;
    BnLayout lay;
    int rc = prepare_call(c, lay, b, n, m, c2, c1, rule, widths, true, workspace, workspace_bytes, stream);
    if (rc != MCP_OK) return rc;
    float *x = c.part(lay.x), *hid[2] = {c.part(lay.h1), c.part(lay.h2)};
    float *const *z = c.z, *const *gy = c.gy, *const *gz = c.gz, *const *coef = c.coef;
    float *grad_blend = c.part(lay.grad_blend), *w_used = c.part(lay.w_used);
    int *count = reinterpret_cast<int *>(c.ws + lay.count);
    c.q.known_feats = known_feats; c.q.skip = skip; c.q.idx = idx; c.q.dist = dist; c.q.w3 = w3; c.q.ulen = ulen; c.q.packed = packed;
    c.q.w_used = w_used;

    // ---- the forward again, statistics given: x, z_l, h_l ----
    hipLaunchKernelGGL(fpbn_count_kernel, dim3(1), dim3(64), 0, c.s, b, n, ulen, count);
    if ((rc = mcp_launch_status()) != MCP_OK) return rc;
    for (int l = 0; l < layers; ++l) {
        hipLaunchKernelGGL(fpbn_coef_kernel, dim3((widths[l] + 255) / 256), dim3(256), 0, c.s, widths[l], gamma[l], beta[l], mean[l], rstd[l], coef[l]);
        if ((rc = mcp_launch_status()) != MCP_OK) return rc;
        if ((rc = forward_pass<FpBnGather>(c, l, widths, false, l == 0 ? x : hid[l - 1])) != MCP_OK) return rc;
    }
    // ---- gy_L and its sums ----
    const int last = layers - 1;
    hipLaunchKernelGGL(fpbn_gy_last_kernel, dim3(c.groups), dim3(256), 0, c.s, c.total, n, widths[last], ulen, z[last], coef[last], grad_out, gy[last], c.q.part);
    if ((rc = mcp_launch_status()) != MCP_OK) return rc;
    if ((rc = backward_passes<FpBnGather>(c, widths, c.groups, count, grad_gamma, grad_beta, grad_blend, grad_skip)) != MCP_OK) return rc;

    // the blend's scatter: every destination row's addends in ascending position 3 p + j
    if (grad_known_feats) {
        rc = mcp_interp3_apply_grad_sorted(b, n, m, c2, nullptr, idx, w_used, grad_blend, order, seg, grad_known_feats, nullptr, stream);
        if (rc != MCP_OK) return rc;
    }
    // dW_l = gz_l^T h_(l-1), db_l = column sums of gz_l (zero in exact arithmetic: the statistics absorb a bias)
    void *wws = c.ws + lay.wgrad;
    for (int l = last; l >= 1; --l) {
        rc = mcp_linear_wgrad(c.total, widths[l], widths[l - 1], gz[l], widths[l], hid[l - 1], widths[l - 1], grad_w[l], grad_b[l], wws, lay.wgrad_bytes, stream);
        if (rc != MCP_OK) return rc;
    }
    const int cin = c.sh.cin;
    if (cin <= WGRAD_COLS) return mcp_linear_wgrad(c.total, widths[0], cin, gz[0], widths[0], x, cin, grad_w[0], grad_b[0], wws, lay.wgrad_bytes, stream);
    float *slice = c.part(lay.dw_slice);
    for (int c0 = 0; c0 < cin; c0 += WGRAD_COLS) {   // columns c0 .. c0 + kb - 1 of x through the row stride; the dense (width, kb) block is then laid into dW_1
        const int kb = cin - c0 < WGRAD_COLS ? cin - c0 : WGRAD_COLS;
        rc = mcp_linear_wgrad(c.total, widths[0], kb, gz[0], widths[0], x + c0, cin, slice, c0 == 0 ? grad_b[0] : nullptr, wws, lay.wgrad_bytes, stream);
        if (rc != MCP_OK) return rc;
        const hipError_t e = hipMemcpy2DAsync(grad_w[0] + c0, (size_t)cin * sizeof(float), slice, (size_t)kb * sizeof(float), (size_t)kb * sizeof(float),
                                              (size_t)widths[0], hipMemcpyDeviceToDevice, c.s);
        if (e != hipSuccess) return (int)e;
    }
    return MCP_OK;
}
