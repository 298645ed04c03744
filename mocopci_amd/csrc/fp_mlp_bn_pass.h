// fp_mlp_bn_pass.h -- the passes of a shared MLP under TRAINING-MODE BatchNorm over a flat list of rows, stated once for the two fused
// point layers that train with batch statistics: feature propagation (fp_mlp_bn.hip) and set abstraction (group_mlp_bn.hip, whose
// rows are the (centre, slot) pairs).  fp_mlp_bn.hip's header describes the passes, the statistics and the saved state; what lives
// here is
//   fpbn_pass_kernel<G, TMAX, STREAM, MODE>   one layer's product with what surrounds it (FWD_GATHER, FWD_ROWS, BWD_MID, BWD_DX);
//   fpbn_count_kernel, fpbn_coef_kernel, fpbn_stats_reduce_kernel, fpbn_sums_reduce_kernel   the small kernels between the passes;
//   BnCall, forward_pass<G>, backward_passes<G>   the host's walk over the layers.
// G is the gather policy of layer 1, the only thing the two layers' passes differ in:
//   typename G::Raw                      what one input k-step reads;
//   void begin(row, args, ptrs)          once per row (FWD_GATHER only);
//   Raw fetch(s)                         the loads of input k-step s;
//   McpSplit3 finish(raw, s, x, p)       the operand of k-step s; its 8 values go to row p of x when x is not NULL.
// A unit keeps its output kernel, the kernel that forms gy_L, its workspace layout and its entry points.  The tiling, the slab
// sequence and the tile helpers are fp_mlp_tile.h's.
#pragma once
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

// The five shape arguments and the five input pointers of layer 1 are named for feature propagation; group_mlp_bn.hip's gather
// reads them under the names its header gives (GbnGather).
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

// feature propagation's layer-1 input: FpGather of fp_mlp_tile.h (the three weights and the three known rows, then the skip row)
struct FpBnGather {
    typedef FpGatherRaw Raw;
    FpGather g;
    __device__ __forceinline__ void begin(const FpRow &me, const BnArgs &a, const BnPtrs &q) {
        g.begin(me, a.m, a.c2, a.c1, a.rule, a.ksb, q.known_feats, q.skip, q.idx, q.dist, q.w3);
        if (q.w_used) g.store_w_used(q.w_used, me.p);
    }
    __device__ __forceinline__ Raw fetch(int s) const { return g.fetch(s); }
    __device__ __forceinline__ McpSplit3 finish(const Raw &r, int s, float *__restrict__ x, long long p) const { return g.finish(r, s, x, p); }
};

template <class G, int TMAX, bool STREAM, int MODE>
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
    G gather;   // FWD_GATHER: what the row's layer-1 input is read with
    if constexpr (MODE == FWD_GATHER) gather.begin(me, a, q);

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
                      [&](const typename G::Raw &now, int s, bool last) { slabs.into(bank, tiles, gather.finish(now, s, q.side, p), last ? after : tiles); });
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

template <class G, int MODE>
int launch_mode(int tmax, bool stream, const BnArgs &a, const BnPtrs &q, hipStream_t s) {
    return fp_dispatch(tmax, stream, [&](auto tm, auto stream_w) {
        constexpr int T = decltype(tm)::value;
        constexpr bool S = decltype(stream_w)::value;
        return fp_launch<fpbn_pass_kernel<G, T, S, MODE>, T, S>(a.total, a.coef_floats + a.stat_floats, a.pass_u4, s, a, q);
    });
}

struct BnCall {   // what every pass of one call shares
    FgShape sh;
    long long total;
    int groups;
    char *ws;
    hipStream_t s;
    BnArgs a;
    BnPtrs q;
    float *z[MAX_LAYERS], *coef[MAX_LAYERS], *gy[MAX_LAYERS], *gz[MAX_LAYERS];   // the layers' parts of the workspace (gy, gz: backward)
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

// the forward pass of layer l: z_l, and with `stats` its partials (the caller reduces them into (mean, var, rstd) and the layer's a, c)
template <class G>
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
    q.in0 = l == 0 ? nullptr : c.z[l - 1];
    q.coef_in = l == 0 ? nullptr : c.coef[l - 1];
    q.out = c.z[l];
    q.side = side;
    if (l != 0) q.w_used = nullptr;
    const bool stream = !fp_weights_in_lds(f);
    return l == 0 ? launch_mode<G, FWD_GATHER>(f.tmax, stream, a, q, c.s) : launch_mode<G, FWD_ROWS>(f.tmax, stream, a, q, c.s);
}

// The backward's walk from gy_L (in c.gy[L-1], its three sums' partials of `groups_last` workgroups in c.q.part) down to dx: per layer
// the sums' reduction (dgamma_l, dbeta_l, the coefficients of gz_l), then BWD_MID or, for layer 1, BWD_DX into (dx_a | dx_b).
template <class G>
int backward_passes(BnCall &c, const int *widths, int groups_last, const int *count, float *const *grad_gamma, float *const *grad_beta, float *dx_a,
                    float *dx_b) {
    const FpShape &f = c.sh.f;
    const int last = f.layers - 1;
    const bool stream_w = !fg_whole(c.sh);
    for (int l = last; l >= 0; --l) {
        hipLaunchKernelGGL(fpbn_sums_reduce_kernel, dim3(widths[l]), dim3(REDUCE_THREADS), 0, c.s, l == last ? groups_last : c.groups, widths[l], c.q.part, count,
                           c.coef[l], grad_gamma[l], grad_beta[l]);
        int rc = mcp_launch_status();
        if (rc != MCP_OK) return rc;
        BnArgs a = c.a;
        BnPtrs q = c.q;
        a.ks = 2 * f.tiles[l];
        a.cin = widths[l];
        a.slab_u4 = c.bwd_slab(l);
        a.coef_floats = 4 * a.cin;
        q.in0 = c.gy[l]; q.in1 = c.z[l]; q.coef_in = c.coef[l] + 4 * widths[l]; q.side = c.gz[l];
        if (l > 0) {
            a.tiles = f.tiles[l - 1];
            a.pass_u4 = a.ks * a.tiles * TILE_U4;
            a.stat_floats = WAVES * 3 * widths[l - 1] + WAVES;
            q.coef_out = c.coef[l - 1]; q.z_prev = c.z[l - 1]; q.out = c.gy[l - 1];
            rc = launch_mode<G, BWD_MID>(f.tmax, stream_w, a, q, c.s);
        } else {
            a.tiles = c.sh.dxt;
            a.pass_u4 = a.ks * a.tiles * TILE_U4;
            a.stat_floats = 0;
            q.grad_blend = dx_a; q.grad_skip = dx_b;
            rc = launch_mode<G, BWD_DX>(f.tmax, stream_w, a, q, c.s);
        }
        if (rc != MCP_OK) return rc;
    }
    return MCP_OK;
}

}  // namespace
