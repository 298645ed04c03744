// fp_mlp_bn.hip -- the fused feature-propagation layer of pointnet2 with TRAINING-MODE BatchNorm (batch statistics) for gfx950: forward
// and backward of  x = [three-neighbour blend | skip],  z_l = W_l h_(l-1) + b_l,  y_l = gamma_l (z_l - mu_l) rstd_l + beta_l,
// h_l = ReLU(y_l),  out = h_L,  with mu_l / v_l the mean and the biased variance of z_l over the live rows.  The blend, the rules,
// ulen and the infinite slots are those of mcp_fp_mlp (fp_mlp.hip); the tiling, the 3-way bf16 split and the operand images are
// those of fp_mlp.hip / fp_mlp_grad.hip (a wave owns 32 rows, the MFMA column; four waves per workgroup; one workgroup per 128 rows).
//
// A pass ends where the next quantity needs a sum over all rows.  One kernel template, fpbn_pass_kernel<TMAX, STREAM, MODE>, is one
// layer's product with what surrounds it:
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
// fp_mlp_grad.hip.
#include "fp_mlp_tile.h"

namespace {

enum { FWD_GATHER = 0, FWD_ROWS = 1, BWD_MID = 2, BWD_DX = 3 };
constexpr int COEF = 8;   // per-channel coefficient rows of one layer in the workspace: a, c, mu, rstd | p, k1, q, mu
constexpr int REDUCE_THREADS = 64;

// the one expression of y_l every kernel uses: the ReLU masks of the backward are the forward's, bit for bit
__device__ __forceinline__ float bn_y(float a, float z, float c) { return a * z + c; }

// sum over the 32 lanes of this lane's half of the wave: a fixed butterfly, the same bits in every lane of the half
__device__ __forceinline__ float half_sum(float v) {
#pragma unroll
    for (int mask = 1; mask < 32; mask <<= 1) v += __shfl_xor(v, mask);
    return v;
}

struct Triple {
    float n, mean, m2;
};
// Chan's update of (count, mean, M2): b appended to a
__device__ __forceinline__ Triple merge(const Triple &a, const Triple &b) {
    if (b.n == 0.f) return a;
    if (a.n == 0.f) return b;
    const float n = a.n + b.n, delta = b.mean - a.mean;
    return Triple{n, a.mean + delta * (b.n / n), (a.m2 + b.m2) + (delta * delta) * (a.n * (b.n / n))};
}

struct BnArgs {
    long long total;   // B * n rows
    int n, m, c2, c1, rule;
    int ksb;           // FWD_GATHER: k-steps of the blend
    int ks;            // k-steps of the input row
    int tiles;         // output tiles (BWD_DX: all tiles of dx)
    int cin;           // floats of an input row (FWD_ROWS, BWD_*)
    int slab_u4;       // first slab of this pass in the image, in uint4
    int pass_u4;       // uint4 of all slabs of this pass
    int bias_at;       // FWD_*: float offset of this layer's bias in the image
    int stats;         // FWD_*: accumulate the (count, mean, M2) partials
    int coef_floats, stat_floats;   // LDS in front of the slabs
};
struct BnPtrs {
    const float *known_feats, *skip, *dist, *w3, *packed;
    const int *idx, *ulen;
    const float *in0, *in1;      // FWD_ROWS: z_(l-1); BWD_*: gy_l, z_l
    const float *coef_in;        // FWD_ROWS: a, c of layer l - 1 (2 cin floats); BWD_*: p, k1, q, mu of layer l (4 cin floats)
    const float *coef_out;       // BWD_MID: a, c, mu, rstd of layer l - 1
    const float *z_prev;         // BWD_MID: z_(l-1)
    float *out;                  // FWD_*: z_l; BWD_MID: gy_(l-1)
    float *side;                 // FWD_GATHER: x; FWD_ROWS: h_(l-1); BWD_*: gz_l (NULL: not written)
    float *w_used;               // FWD_GATHER (NULL: not written)
    float *grad_blend, *grad_skip;
    float *part;                 // (workgroups, 2, 32 tiles): mean | M2, or (workgroups, 3, 32 tiles): the backward's three sums
    int *part_cnt;               // (workgroups): live rows
};

struct BnRows {    // what one k-step of a stored row reads: two quads of in0, two of in1
    FpQuads a, b;
};

template <int TMAX, bool STREAM, int MODE>
__global__ __launch_bounds__(THREADS, TMAX == 8 ? 1 : 2) void fpbn_pass_kernel(const BnArgs a, const BnPtrs q) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *coef = lds;                                                           // the input channels' coefficients
    float *stat = lds + a.coef_floats;                                           // [wave][2][output channels], then the waves' live rows
    int *wave_cnt = reinterpret_cast<int *>(lds + a.coef_floats + a.stat_floats) - WAVES;   // (all of the LDS is dynamic: the whole 160 KB may be asked for)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, col = lane & 31;
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);

    FpSlabs<TMAX, STREAM> slabs;   // behind coef and stat: this pass's slabs, or two slab buffers
    {
        if constexpr (MODE != FWD_GATHER)
            for (int e = tid; e < a.coef_floats / 4; e += THREADS) reinterpret_cast<float4 *>(coef)[e] = reinterpret_cast<const float4 *>(q.coef_in)[e];
        slabs.begin(reinterpret_cast<u32x4 *>(lds + a.coef_floats + a.stat_floats), reinterpret_cast<const u32x4 *>(q.packed) + a.slab_u4,
                    MODE == BWD_DX ? min(TMAX, a.tiles) : a.tiles, a.pass_u4);
    }
    __syncthreads();

    const FpRow me(a.total, a.n, q.ulen);
    const long long p = me.p;
    const bool inr = me.inr, live = me.live;
    FpGather gather;   // FWD_GATHER: the three weights and the three known rows
    if constexpr (MODE == FWD_GATHER) {
        gather.begin(me, a.m, a.c2, a.c1, a.rule, a.ksb, q.known_feats, q.skip, q.idx, q.dist, q.w3);
        if (q.w_used) gather.store_w_used(q.w_used, p);
    }

    // ---- FWD_ROWS, BWD_*: k-step s of the lane's own stored row is the two quads at 16 s and 16 s + 8 (from channel 4 h) ----
    const long long in_at = p * a.cin + 4 * h;
    auto load_rows = [&](int s) {
        BnRows r{fp_row_kstep(q.in0 + in_at, s, live), FpQuads{z4, z4}};
        if constexpr (MODE >= BWD_MID) r.b = fp_row_kstep(q.in1 + in_at, s, live);
        return r;
    };
    // the operand of k-step s formed on load: h_(l-1) = ReLU(a z + c), or gz_l = p (gy - k1) + q (z - mu); zeros in a padded row;
    // written to the workspace (the weight sums read it) when `keep`
    auto finish_rows = [&](const BnRows &r, int s, bool keep) {
        float v[8];
        const float in0[8] = {r.a.a0.x, r.a.a0.y, r.a.a0.z, r.a.a0.w, r.a.a1.x, r.a.a1.y, r.a.a1.z, r.a.a1.w};
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const int ch = 16 * s + 8 * half + 4 * h;
            const float4 k0 = *reinterpret_cast<const float4 *>(coef + ch), k1 = *reinterpret_cast<const float4 *>(coef + a.cin + ch);
            const float c0[4] = {k0.x, k0.y, k0.z, k0.w}, c1[4] = {k1.x, k1.y, k1.z, k1.w};
            if constexpr (MODE == FWD_ROWS) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float y = bn_y(c0[i], in0[4 * half + i], c1[i]);
                    v[4 * half + i] = (live && y > 0.f) ? y : 0.f;
                }
            } else {
                const float in1[8] = {r.b.a0.x, r.b.a0.y, r.b.a0.z, r.b.a0.w, r.b.a1.x, r.b.a1.y, r.b.a1.z, r.b.a1.w};
                const float4 k2 = *reinterpret_cast<const float4 *>(coef + 2 * a.cin + ch), k3 = *reinterpret_cast<const float4 *>(coef + 3 * a.cin + ch);
                const float c2[4] = {k2.x, k2.y, k2.z, k2.w}, c3[4] = {k3.x, k3.y, k3.z, k3.w};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float gz = c0[i] * (in0[4 * half + i] - c1[i]) + c2[i] * (in1[4 * half + i] - c3[i]);
                    v[4 * half + i] = live ? gz : 0.f;
                }
            }
            if (keep && q.side && inr) *reinterpret_cast<float4 *>(q.side + in_at + 16 * s + 8 * half) = make_float4(v[4 * half], v[4 * half + 1], v[4 * half + 2], v[4 * half + 3]);
        }
        return mcp_split8(v);
    };
    // bank += image . rows over the pass's k-steps; `after`: the output tiles of the slab behind the product's last (0: none); in
    // FWD_GATHER x is written on the way when the backward asks for it (q.side)
    auto product = [&](f32x16(&bank)[TMAX], int tiles, int after, bool keep) {
        if constexpr (MODE == FWD_GATHER) {
            fp_ksteps(a.ks, [&](int s) { return gather.fetch(s); },
                      [&](const FpGatherRaw &now, int s, bool last) { slabs.into(bank, tiles, gather.finish(now, s, q.side, p), last ? after : tiles); });
        } else {
            fp_ksteps(a.ks, load_rows, [&](const BnRows &now, int s, bool last) { slabs.into(bank, tiles, finish_rows(now, s, keep), last ? after : tiles); });
        }
    };
    // the workgroup's partials: the waves' entries of stat in wave order
    const int cout = a.tiles * 32;
    float *part = q.part + (size_t)blockIdx.x * 2 * cout;

    f32x16 bank[TMAX];
    if constexpr (MODE == FWD_GATHER || MODE == FWD_ROWS) {
        // ---- z_l = W_l h_(l-1) + b_l; the statistics' partials ----
#pragma unroll
        for (int t = 0; t < TMAX; ++t) fp_bias_tile(bank[t], t, a.tiles, q.packed + a.bias_at);
        product(bank, a.tiles, 0, true);
        const int cnt = __popcll(__ballot(live) & 0xFFFFFFFFull);   // live rows of this wave
        const float inv = 1.0f / (float)max(cnt, 1);
        float *orow = q.out + p * cout + 4 * h;
#pragma unroll
        for (int t = 0; t < TMAX; ++t) {
            if (t < a.tiles) {
                if (inr) {
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        float4 v = make_float4(bank[t][4 * g + 0], bank[t][4 * g + 1], bank[t][4 * g + 2], bank[t][4 * g + 3]);
                        if (!live) v = z4;
                        *reinterpret_cast<float4 *>(orow + 32 * t + 8 * g) = v;
                    }
                }
                if (a.stats) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float mean = half_sum(live ? bank[t][r] : 0.f) * inv;
                        const float d = live ? bank[t][r] - mean : 0.f;
                        const float m2 = half_sum(d * d);
                        if (col == 0) {
                            const int ch = 32 * t + mcp_chan_of(r, h);
                            stat[(wave * 2 + 0) * cout + ch] = mean;
                            stat[(wave * 2 + 1) * cout + ch] = m2;
                        }
                    }
                }
            }
        }
        if (a.stats) {
            if (lane == 0) wave_cnt[wave] = cnt;
            __syncthreads();
            for (int c = tid; c < cout; c += THREADS) {
                Triple acc{0.f, 0.f, 0.f};
#pragma unroll
                for (int w = 0; w < WAVES; ++w) acc = merge(acc, Triple{(float)wave_cnt[w], stat[(w * 2 + 0) * cout + c], stat[(w * 2 + 1) * cout + c]});
                part[c] = acc.mean;
                part[cout + c] = acc.m2;
            }
            if (tid == 0) q.part_cnt[blockIdx.x] = (wave_cnt[0] + wave_cnt[1]) + (wave_cnt[2] + wave_cnt[3]);
        }
    } else if constexpr (MODE == BWD_MID) {
        // ---- gy_(l-1) = (W_l^T gz_l) . [y_(l-1) > 0]; the partials of sum gy_(l-1), sum gy_(l-1) zhat_(l-1) and sum (z_(l-1) - mu) ----
        fp_zero_bank(bank);
        product(bank, a.tiles, 0, true);
        fp_pin_bank(bank);
        const long long at = p * cout + 4 * h;
#pragma unroll
        for (int t = 0; t < TMAX; ++t) {
            if (t < a.tiles) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int ch = 32 * t + 8 * g + 4 * h;
                    const float4 ka = *reinterpret_cast<const float4 *>(q.coef_out + ch), kc = *reinterpret_cast<const float4 *>(q.coef_out + cout + ch);
                    const float4 km = *reinterpret_cast<const float4 *>(q.coef_out + 2 * cout + ch), kr = *reinterpret_cast<const float4 *>(q.coef_out + 3 * cout + ch);
                    float4 zq = z4;
                    if (live) zq = *reinterpret_cast<const float4 *>(q.z_prev + at + 32 * t + 8 * g);
                    const float zv[4] = {zq.x, zq.y, zq.z, zq.w}, av[4] = {ka.x, ka.y, ka.z, ka.w}, cv[4] = {kc.x, kc.y, kc.z, kc.w};
                    const float mv[4] = {km.x, km.y, km.z, km.w}, rv[4] = {kr.x, kr.y, kr.z, kr.w};
                    float gy[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const bool pos = bn_y(av[j], zv[j], cv[j]) > 0.f;
                        gy[j] = (live && pos) ? bank[t][4 * g + j] : 0.f;
                        const float s1 = half_sum(gy[j]);
                        const float s2 = half_sum(live ? gy[j] * ((zv[j] - mv[j]) * rv[j]) : 0.f);
                        const float s3 = half_sum(live ? zv[j] - mv[j] : 0.f);
                        if (col == 0) {
                            stat[(wave * 3 + 0) * cout + ch + j] = s1;
                            stat[(wave * 3 + 1) * cout + ch + j] = s2;
                            stat[(wave * 3 + 2) * cout + ch + j] = s3;
                        }
                    }
                    if (inr) *reinterpret_cast<float4 *>(q.out + at + 32 * t + 8 * g) = make_float4(gy[0], gy[1], gy[2], gy[3]);
                }
            }
        }
        __syncthreads();
        for (int c = tid; c < 3 * cout; c += THREADS) q.part[(size_t)blockIdx.x * 3 * cout + c] = ((stat[c] + stat[3 * cout + c]) + stat[6 * cout + c]) + stat[9 * cout + c];
    } else {
        // ---- dx = W_1^T gz_1 in chunks of TMAX output tiles: grad_blend | grad_skip ----
#pragma unroll 1
        for (int c0 = 0; c0 < a.tiles; c0 += TMAX) {
            const int tc = min(TMAX, a.tiles - c0);
            fp_zero_bank(bank);
            product(bank, tc, min(TMAX, a.tiles - c0 - TMAX), c0 == 0);
            if (inr) fp_store_dx(bank, c0, tc, p, a.c2, a.c1, q.grad_blend, q.grad_skip);
        }
    }
}

// live rows of the call: sum of the clamped lengths, or B * n
__global__ __launch_bounds__(64) void fpbn_count_kernel(int b, int n, const int *__restrict__ ulen, int *__restrict__ count) {
    if (threadIdx.x != 0) return;
    long long c = (long long)b * n;
    if (ulen) {
        c = 0;
        for (int i = 0; i < b; ++i) c += min(max(ulen[i], 0), n);
    }
    *count = (int)(c > 0x7FFFFFFFLL ? 0x7FFFFFFFLL : c);
}

// a, c, mu, rstd of one layer from the saved statistics (the backward's recompute)
__global__ __launch_bounds__(256) void fpbn_coef_kernel(int c, const float *__restrict__ gamma, const float *__restrict__ beta, const float *__restrict__ mean,
                                                        const float *__restrict__ rstd, float *__restrict__ coef) {
    const int ch = blockIdx.x * 256 + threadIdx.x;
    if (ch >= c) return;
    const float a = (gamma ? gamma[ch] : 1.f) * rstd[ch];
    coef[ch] = a;
    coef[c + ch] = (beta ? beta[ch] : 0.f) - mean[ch] * a;
    coef[2 * c + ch] = mean[ch];
    coef[3 * c + ch] = rstd[ch];
}

// One block per channel.  Thread i merges the workgroups i * chunk .. (i + 1) * chunk - 1 in order, thread 0 the 64 chunks in order.
__global__ __launch_bounds__(REDUCE_THREADS) void fpbn_stats_reduce_kernel(int groups, int c, const float *__restrict__ part, const int *__restrict__ part_cnt,
                                                                           const float *__restrict__ gamma, const float *__restrict__ beta, float eps,
                                                                           float *__restrict__ mean, float *__restrict__ var, float *__restrict__ rstd,
                                                                           float *__restrict__ coef) {
    __shared__ Triple chunks[REDUCE_THREADS];
    const int ch = blockIdx.x, chunk = (groups + REDUCE_THREADS - 1) / REDUCE_THREADS;
    Triple acc{0.f, 0.f, 0.f};
    for (int g = threadIdx.x * chunk; g < min(groups, (int)(threadIdx.x + 1) * chunk); ++g)
        acc = merge(acc, Triple{(float)part_cnt[g], part[(size_t)g * 2 * c + ch], part[(size_t)g * 2 * c + c + ch]});
    chunks[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int i = 1; i < REDUCE_THREADS; ++i) acc = merge(acc, chunks[i]);
    const float v = acc.m2 / fmaxf(acc.n, 1.f), rs = 1.0f / sqrtf(v + eps);
    const float a = (gamma ? gamma[ch] : 1.f) * rs;
    mean[ch] = acc.mean;
    var[ch] = v;
    rstd[ch] = rs;
    coef[ch] = a;
    coef[c + ch] = (beta ? beta[ch] : 0.f) - acc.mean * a;
    coef[2 * c + ch] = acc.mean;
    coef[3 * c + ch] = rs;
}

// The same walk over plain sums: dbeta = sum gy, dgamma = sum gy zhat, and the coefficients of gz = p (gy - k1) + q (z - mu).
// The third sum, r = sum (z - mu), is zero for the exact mean; for the fp32 mu it is -m times mu's rounding error, which a layer with
// |mu| >> sigma feels: sum gz would miss zero by q r, and dW = sum gz h^T carries that times the mean of h.  lo = r / m is the low
// part of the mean, (z - mu) - lo the centred value: it is folded into k1 (no fourth operand on load) and into dgamma.
__global__ __launch_bounds__(REDUCE_THREADS) void fpbn_sums_reduce_kernel(int groups, int c, const float *__restrict__ part, const int *__restrict__ count,
                                                                          float *__restrict__ coef, float *__restrict__ grad_gamma, float *__restrict__ grad_beta) {
    __shared__ float s1[REDUCE_THREADS], s2[REDUCE_THREADS], s3[REDUCE_THREADS];
    const int ch = blockIdx.x, chunk = (groups + REDUCE_THREADS - 1) / REDUCE_THREADS;
    float a1 = 0.f, a2 = 0.f, a3 = 0.f;
    for (int g = threadIdx.x * chunk; g < min(groups, (int)(threadIdx.x + 1) * chunk); ++g) {
        a1 += part[(size_t)g * 3 * c + ch];
        a2 += part[(size_t)g * 3 * c + c + ch];
        a3 += part[(size_t)g * 3 * c + 2 * c + ch];
    }
    s1[threadIdx.x] = a1;
    s2[threadIdx.x] = a2;
    s3[threadIdx.x] = a3;
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int i = 1; i < REDUCE_THREADS; ++i) {
        a1 += s1[i];
        a2 += s2[i];
        a3 += s3[i];
    }
    const float m = (float)max(*count, 1);
    const float p = coef[ch], rs = coef[3 * c + ch], lo = a3 / m;
    const float dgamma = a2 - (lo * rs) * a1;
    if (grad_beta) grad_beta[ch] = a1;
    if (grad_gamma) grad_gamma[ch] = dgamma;
    coef[4 * c + ch] = p;
    coef[5 * c + ch] = a1 / m - (rs * (dgamma / m)) * lo;   // p (gy - k1) + q (z - mu) with q lo folded in: q / p = -rs dgamma / m
    coef[6 * c + ch] = -(p * rs) * (dgamma / m);
    coef[7 * c + ch] = coef[2 * c + ch];
}

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

template <int MODE>
int launch_mode(int tmax, bool stream, const BnArgs &a, const BnPtrs &q, hipStream_t s) {
    return fp_dispatch(tmax, stream, [&](auto tm, auto stream_w) {
        constexpr int T = decltype(tm)::value;
        constexpr bool S = decltype(stream_w)::value;
        return fp_launch<fpbn_pass_kernel<T, S, MODE>, T, S>(a.total, a.coef_floats + a.stat_floats, a.pass_u4, s, a, q);
    });
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

struct BnCall {   // what every pass of one call shares
    FgShape sh;
    BnLayout lay;
    long long total;
    int groups;
    char *ws;
    hipStream_t s;
    BnArgs a;
    BnPtrs q;
    float *part(size_t off) const { return reinterpret_cast<float *>(ws + off); }
    int fwd_slab(int l) const {   // first forward slab of layer l, in uint4
        int u4 = 0;
        for (int j = 0; j < l; ++j) u4 += sh.f.tiles[j] * sh.f.ks[j] * TILE_U4;
        return u4;
    }
    int bwd_slab(int l) const {   // first slab of W_l^T (l >= 1), or of the chunks of dx (l = 0)
        int u4 = sh.f.w_u4 + sh.f.small_floats / 4;
        for (int j = sh.f.layers - 1; j > l; --j) u4 += 2 * sh.f.tiles[j] * sh.f.tiles[j - 1] * TILE_U4;
        return u4;
    }
};

// the forward pass of layer l: z_l, and with `stats` its partials reduced into (mean, var, rstd) and the layer's a, c
int forward_pass(BnCall &c, int l, const int *widths, bool stats, float *side) {
    const FpShape &f = c.sh.f;
    BnArgs a = c.a;
    BnPtrs q = c.q;
    a.ks = f.ks[l];
    a.tiles = f.tiles[l];
    a.cin = l == 0 ? c.sh.cin : widths[l - 1];
    a.slab_u4 = c.fwd_slab(l);
    a.pass_u4 = f.tiles[l] * f.ks[l] * TILE_U4;
    a.bias_at = f.w_u4 * 4 + f.boff[l];
    a.stats = stats ? 1 : 0;
    a.coef_floats = l == 0 ? 0 : 2 * a.cin;
    a.stat_floats = WAVES * 2 * widths[l] + WAVES;
    q.in0 = l == 0 ? nullptr : c.part(c.lay.z[l - 1]);
    q.coef_in = l == 0 ? nullptr : c.part(c.lay.coef[l - 1]);
    q.out = c.part(c.lay.z[l]);
    q.side = side;
    if (l != 0) q.w_used = nullptr;
    const bool stream = !fp_weights_in_lds(f);
    return l == 0 ? launch_mode<FWD_GATHER>(f.tmax, stream, a, q, c.s) : launch_mode<FWD_ROWS>(f.tmax, stream, a, q, c.s);
}

// c.sh is set: the layout, the sizes and what every pass shares
int prepare_call(BnCall &c, int b, int n, int m, int c2, int c1, int rule, const int *widths, bool backward, void *workspace,
                 size_t workspace_bytes, mcp_stream_t stream) {
    c.total = (long long)b * n;
    if (!bn_layout(c.total, c.sh, widths, backward, &c.lay)) return MCP_ERR_UNSUPPORTED;
    if (workspace_bytes < c.lay.bytes) return MCP_ERR_BAD_ARG;
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
    c.q.part = c.part(c.lay.part);
    c.q.part_cnt = reinterpret_cast<int *>(c.ws + c.lay.part_cnt);
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
    int rc = prepare_call(c, b, n, m, c2, c1, rule, widths, false, workspace, workspace_bytes, stream);
    if (rc != MCP_OK) return rc;
    c.q.known_feats = known_feats; c.q.skip = skip; c.q.idx = idx; c.q.dist = dist; c.q.w3 = w3; c.q.ulen = ulen; c.q.packed = packed;
    hipLaunchKernelGGL(fpbn_count_kernel, dim3(1), dim3(64), 0, c.s, b, n, ulen, count);
    if ((rc = mcp_launch_status()) != MCP_OK) return rc;
    for (int l = 0; l < layers; ++l) {
        if ((rc = forward_pass(c, l, widths, true, nullptr)) != MCP_OK) return rc;
        hipLaunchKernelGGL(fpbn_stats_reduce_kernel, dim3(widths[l]), dim3(REDUCE_THREADS), 0, c.s, c.groups, widths[l], c.q.part, c.q.part_cnt, gamma[l], beta[l],
                           eps[l], mean[l], var[l], rstd[l], c.part(c.lay.coef[l]));
        if ((rc = mcp_launch_status()) != MCP_OK) return rc;
    }
    const int cl = widths[layers - 1];
    const long long quads = c.total * (cl / 4);
    if ((quads + 255) / 256 > 0x7FFFFFFFLL) return MCP_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(fpbn_out_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, c.s, c.total, n, cl, ulen, c.part(c.lay.z[layers - 1]),
                       c.part(c.lay.coef[layers - 1]), out);
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
    int rc = prepare_call(c, b, n, m, c2, c1, rule, widths, true, workspace, workspace_bytes, stream);
    if (rc != MCP_OK) return rc;
    const FpShape &f = c.sh.f;
    const BnLayout &lay = c.lay;
    float *x = c.part(lay.x), *hid[2] = {c.part(lay.h1), c.part(lay.h2)};
    float *z[MAX_LAYERS], *gy[MAX_LAYERS], *gz[MAX_LAYERS], *coef[MAX_LAYERS];
    for (int l = 0; l < MAX_LAYERS; ++l) { z[l] = c.part(lay.z[l]); gy[l] = c.part(lay.gy[l]); gz[l] = c.part(lay.gz[l]); coef[l] = c.part(lay.coef[l]); }
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
        if ((rc = forward_pass(c, l, widths, false, l == 0 ? x : hid[l - 1])) != MCP_OK) return rc;
    }
    // ---- gy_L and its sums ----
    const int last = layers - 1;
    hipLaunchKernelGGL(fpbn_gy_last_kernel, dim3(c.groups), dim3(256), 0, c.s, c.total, n, widths[last], ulen, z[last], coef[last], grad_out, gy[last], c.q.part);
    if ((rc = mcp_launch_status()) != MCP_OK) return rc;
    const bool stream_w = !fg_whole(c.sh);
    for (int l = last; l >= 0; --l) {
        hipLaunchKernelGGL(fpbn_sums_reduce_kernel, dim3(widths[l]), dim3(REDUCE_THREADS), 0, c.s, c.groups, widths[l], c.q.part, count, coef[l], grad_gamma[l],
                           grad_beta[l]);
        if ((rc = mcp_launch_status()) != MCP_OK) return rc;
        BnArgs a = c.a;
        BnPtrs q = c.q;
        a.ks = 2 * f.tiles[l];
        a.cin = widths[l];
        a.slab_u4 = c.bwd_slab(l);
        a.coef_floats = 4 * a.cin;
        q.in0 = gy[l]; q.in1 = z[l]; q.coef_in = coef[l] + 4 * widths[l]; q.side = gz[l];
        if (l > 0) {
            a.tiles = f.tiles[l - 1];
            a.pass_u4 = a.ks * a.tiles * TILE_U4;
            a.stat_floats = WAVES * 3 * widths[l - 1] + WAVES;
            q.coef_out = coef[l - 1]; q.z_prev = z[l - 1]; q.out = gy[l - 1];
            rc = launch_mode<BWD_MID>(f.tmax, stream_w, a, q, c.s);
        } else {
            a.tiles = c.sh.dxt;
            a.pass_u4 = a.ks * a.tiles * TILE_U4;
            a.stat_floats = 0;
            q.grad_blend = grad_blend; q.grad_skip = grad_skip;
            rc = launch_mode<BWD_DX>(f.tmax, stream_w, a, q, c.s);
        }
        if (rc != MCP_OK) return rc;
    }

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
