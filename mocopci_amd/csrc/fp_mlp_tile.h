// fp_mlp_tile.h -- the device code and the launch code that the three units of the fused feature-propagation layer share: the forward
// (fp_mlp.hip), its backward (fp_mlp_grad.hip) and the training-mode BatchNorm form (fp_mlp_bn.hip; through fp_mlp_bn_pass.h also the
// set-abstraction layer's, group_mlp_bn.hip, which brings its own gather).  fp_mlp_shape.h holds the host's
// shape arithmetic; this header holds what a wave does with one column of the MFMA: its row (FpRow), the layer-1 input k-step
// (FpGather), the slab sequence with the hazard fence (FpSlabs), the small tile helpers, the dx epilogue, and the launch.  Every unit
// keeps its argument structs, its pack kernel, its layer control flow and its epilogues.
//
// Rules the callers rely on: every loop over tiles is fully unrolled and an absent tile is skipped by a wave-uniform branch, so no
// accumulator or operand array is indexed with a run-time value; weights and masks are comparisons and selections (no fmaxf), so
// the units' differing -fno-honor-nans settings give the same bits; the blend is rounded fp32 products in one sum order.
#pragma once
#include <math.h>

#include <type_traits>

#include "common.h"
#include "mfma_split.h"
#include "fp_mlp_shape.h"

namespace {

constexpr int WAVES = 4;
constexpr int THREADS = 64 * WAVES;
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// ---- this column's row of the flattened (B * n) list: a wave owns 32 rows, a workgroup 32 * WAVES.  A row at or beyond the clamped
// ulen[bb] is in range but not live: it writes zeros and none of its inputs is read. ----
struct FpRow {
    long long p, bb;
    bool inr, live;
    __device__ __forceinline__ FpRow(long long total, int n, const int *__restrict__ ulen) {
        p = ((long long)blockIdx.x * WAVES + (threadIdx.x >> 6)) * 32 + (threadIdx.x & 31);
        inr = p < total;
        bb = inr ? mcp_div(p, n, mcp_fits32(total)) : 0;
        live = inr;
        if (inr && ulen) {
            const int ul = min(max(ulen[bb], 0), n);
            live = (int)(p - bb * n) < ul;
        }
    }
};

// ---- the layer-1 input: x = [(w0 f[i0] + w1 f[i1]) + w2 f[i2] (C2 values) | skip row (C1 values)], 16 channels per k-step ----
struct FpGatherRaw {  // what one input k-step reads: the two float4 of each of the three known rows, or of the skip row (in a*)
    float4 a0, a1, b0, b1, c0, c1;
};

struct FpGather {
    float w0 = 0.f, w1 = 0.f, w2 = 0.f;
    bool u0 = false, u1 = false, u2 = false;  // the slot's row is read
    bool inr = false, live = false, skip_q = false;
    const float *f0 = nullptr, *f1 = nullptr, *f2 = nullptr, *srow = nullptr;
    int c2 = 0, c1 = 0, ksb = 0, h = 0;

    // The three weights by `rule` (the forward's header states them) and the rows they go with.  Under rules 1 and 2 a slot whose
    // dist is +inf has the weight 0 by selection and its row is not read; a row that is not live reads nothing at all.
    __device__ __forceinline__ void begin(const FpRow &r, int m, int c2_, int c1_, int rule, int ksb_, const float *__restrict__ known_feats,
                                          const float *__restrict__ skip, const int *__restrict__ idx, const float *__restrict__ dist,
                                          const float *__restrict__ w3) {
        const long long p = r.p;
        inr = r.inr; live = r.live;
        c2 = c2_; c1 = c1_; ksb = ksb_;
        h = (threadIdx.x & 63) >> 5;
        f0 = f1 = f2 = known_feats;
        srow = skip;
        if (live) {
            const int *ip = idx + p * 3;
            const long long base = r.bb * m;
            f0 = known_feats + (base + ip[0]) * c2;
            f1 = known_feats + (base + ip[1]) * c2;
            f2 = known_feats + (base + ip[2]) * c2;
            if (c1) srow = skip + p * c1;
            if (rule == 0) {
                w0 = w3[p * 3 + 0]; w1 = w3[p * 3 + 1]; w2 = w3[p * 3 + 2];
                u0 = u1 = u2 = true;
            } else {
                float d0 = dist[p * 3 + 0], d1 = dist[p * 3 + 1], d2 = dist[p * 3 + 2];
                u0 = d0 < INFINITY; u1 = d1 < INFINITY; u2 = d2 < INFINITY;
                if (rule == 1) {
                    d0 = d0 + 1e-8f; d1 = d1 + 1e-8f; d2 = d2 + 1e-8f;
                } else {
                    d0 = d0 * d0; d1 = d1 * d1; d2 = d2 * d2;
                    d0 = d0 < 1e-10f ? 1e-10f : d0; d1 = d1 < 1e-10f ? 1e-10f : d1; d2 = d2 < 1e-10f ? 1e-10f : d2;
                }
                const float r0 = u0 ? 1.0f / d0 : 0.f, r1 = u1 ? 1.0f / d1 : 0.f, r2 = u2 ? 1.0f / d2 : 0.f;
                const float sum = (r0 + r1) + r2;
                const bool any = sum > 0.f;  // false: no known point at all -- zeros, not 0 / 0
                w0 = any ? r0 / sum : 0.f; w1 = any ? r1 / sum : 0.f; w2 = any ? r2 / sum : 0.f;
            }
        }
        skip_q = (c1 & 3) == 0;  // skip rows (and so the rows of x and grad_skip) are 16-byte aligned
    }
    // the weights the blend uses, row p of a (B, n, 3) array: an infinite slot holds an exact 0, a padded row three
    __device__ __forceinline__ void store_w_used(float *__restrict__ w_used, long long p) const {
        if (inr && h == 0) {
            float *wu = w_used + p * 3;
            wu[0] = u0 ? w0 : 0.f; wu[1] = u1 ? w1 : 0.f; wu[2] = u2 ? w2 : 0.f;
        }
    }
    // the raw rows of input k-step s: ceil(C2 / 16) k-steps of the blend, then ceil(C1 / 16) of the skip row
    __device__ __forceinline__ FpGatherRaw fetch(int s) const {
        const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
        FpGatherRaw r{z4, z4, z4, z4, z4, z4};
        if (s < ksb) {
            const int ch0 = 16 * s + 4 * h, ch1 = ch0 + 8;
            if (ch0 < c2) {
                if (u0) r.a0 = *reinterpret_cast<const float4 *>(f0 + ch0);
                if (u1) r.b0 = *reinterpret_cast<const float4 *>(f1 + ch0);
                if (u2) r.c0 = *reinterpret_cast<const float4 *>(f2 + ch0);
            }
            if (ch1 < c2) {
                if (u0) r.a1 = *reinterpret_cast<const float4 *>(f0 + ch1);
                if (u1) r.b1 = *reinterpret_cast<const float4 *>(f1 + ch1);
                if (u2) r.c1 = *reinterpret_cast<const float4 *>(f2 + ch1);
            }
        } else if (live) {
            const int ch0 = 16 * (s - ksb) + 4 * h, ch1 = ch0 + 8;
            if (skip_q) {
                if (ch0 < c1) r.a0 = *reinterpret_cast<const float4 *>(srow + ch0);
                if (ch1 < c1) r.a1 = *reinterpret_cast<const float4 *>(srow + ch1);
            } else {
                if (ch0 + 0 < c1) r.a0.x = srow[ch0 + 0];
                if (ch0 + 1 < c1) r.a0.y = srow[ch0 + 1];
                if (ch0 + 2 < c1) r.a0.z = srow[ch0 + 2];
                if (ch0 + 3 < c1) r.a0.w = srow[ch0 + 3];
                if (ch1 + 0 < c1) r.a1.x = srow[ch1 + 0];
                if (ch1 + 1 < c1) r.a1.y = srow[ch1 + 1];
                if (ch1 + 2 < c1) r.a1.z = srow[ch1 + 2];
                if (ch1 + 3 < c1) r.a1.w = srow[ch1 + 3];
            }
        }
        return r;
    }
    __device__ __forceinline__ float blend(float fa, float fb, float fc) const { return (w0 * fa + w1 * fb) + w2 * fc; }
    // The operand of k-step s.  With `x` (the (rows, C2 + C1) array of the layer's input, or NULL) its 8 values are written to row q
    // on the way; the caller passes the row index so that a unit can form it where it likes.
    __device__ __forceinline__ McpSplit3 finish(const FpGatherRaw &r, int s, float *__restrict__ x, long long q) const {
        float v[8];
        const bool blended = s < ksb;
        if (blended) {
            v[0] = blend(r.a0.x, r.b0.x, r.c0.x); v[1] = blend(r.a0.y, r.b0.y, r.c0.y);
            v[2] = blend(r.a0.z, r.b0.z, r.c0.z); v[3] = blend(r.a0.w, r.b0.w, r.c0.w);
            v[4] = blend(r.a1.x, r.b1.x, r.c1.x); v[5] = blend(r.a1.y, r.b1.y, r.c1.y);
            v[6] = blend(r.a1.z, r.b1.z, r.c1.z); v[7] = blend(r.a1.w, r.b1.w, r.c1.w);
        } else {
            v[0] = r.a0.x; v[1] = r.a0.y; v[2] = r.a0.z; v[3] = r.a0.w;
            v[4] = r.a1.x; v[5] = r.a1.y; v[6] = r.a1.z; v[7] = r.a1.w;
        }
        if (x && inr) {
            const int lim = blended ? c2 : c1;
            const int loc = 16 * (blended ? s : s - ksb) + 4 * h;
            float *xr = x + q * (c2 + c1) + (blended ? 0 : c2);
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                const int lc = loc + 8 * half;
                if (skip_q) {   // C2 and C1 multiples of 4: whole quads
                    if (lc < lim) *reinterpret_cast<float4 *>(xr + lc) = make_float4(v[4 * half], v[4 * half + 1], v[4 * half + 2], v[4 * half + 3]);
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (lc + i < lim) xr[lc + i] = v[4 * half + i];
                }
            }
        }
        return mcp_split8(v);
    }
};

// ---- the slab sequence.  A slab is one k-step of one layer: `tiles` output tiles of TILE_U4 uint4 each, in the order the image
// holds them.  Either the unit's whole run of slabs lies in LDS (STREAM false) or the workgroup holds two slab buffers and fetches slab
// q + 1 while slab q is multiplied, one barrier per slab.  A streamed slab is fetched one slab ahead, so every into() names the
// output tiles of the slab AFTER its own (0: none) and the uint4 that lie between the two in the image (the backward's biases):
// both are known where the call stands, no walk of a table. ----
template <int TMAX, bool STREAM>
struct FpSlabs {
    static constexpr int LOADS = (TMAX * TILE_U4 + THREADS - 1) / THREADS;
    static constexpr int BUF = LOADS * THREADS;  // uint4 of one LDS slab buffer: the widest slab rounded up to whole passes of the workgroup
    u32x4 pre[LOADS];      // staging registers of the slab after the one being multiplied
    const u32x4 *nxt_src;  // streamed: where the next slab to fetch starts
    const u32x4 *wcur;     // staged whole: the next slab in LDS
    u32x4 *wl;             // the whole run of slabs, or [2][BUF]
    int cur = 0;

    // bytes of LDS the slabs take behind the unit's own: host side
    static size_t lds_bytes(int whole_u4) { return STREAM ? (size_t)2 * BUF * 16 : (size_t)whole_u4 * 16; }

    __device__ __forceinline__ void fetch(int tiles, int skip_u4) {
        if (tiles > 0) {
            nxt_src += skip_u4;
            const int n4 = tiles * TILE_U4, tid = threadIdx.x;
#pragma unroll
            for (int u = 0; u < LOADS; ++u) pre[u] = nxt_src[min(tid + u * THREADS, n4 - 1)];  // entries past the slab repeat its last one, never used
            nxt_src += n4;
        }
    }
    __device__ __forceinline__ void stash(int buf) {
#pragma unroll
        for (int u = 0; u < LOADS; ++u) wl[buf * BUF + threadIdx.x + u * THREADS] = pre[u];
    }
    // The first slab (of first_tiles tiles) into buffer 0, or all whole_u4 uint4 of the run into LDS; the caller's barrier follows.
    __device__ __forceinline__ void begin(u32x4 *lds_slabs, const u32x4 *image, int first_tiles, int whole_u4) {
        wl = lds_slabs;
        wcur = lds_slabs;
        nxt_src = image;
#pragma unroll
        for (int u = 0; u < LOADS; ++u) pre[u] = u32x4{0u, 0u, 0u, 0u};
        if constexpr (STREAM) {
            fetch(first_tiles, 0);
            stash(0);
        } else {
            for (int e = threadIdx.x; e < whole_u4; e += THREADS) wl[e] = image[e];
        }
    }
    // staged whole: another run of slabs takes the place of the one that has been consumed (streamed: nothing to do)
    __device__ __forceinline__ void restage(const u32x4 *image, int whole_u4) {
        if constexpr (!STREAM) {
            __syncthreads();
            for (int e = threadIdx.x; e < whole_u4; e += THREADS) wl[e] = image[e];
            __syncthreads();
            wcur = wl;
        }
    }
    // one k-step slab into every output tile of a bank
    __device__ __forceinline__ void into(f32x16 (&bank)[TMAX], int tiles, const McpSplit3 &xs, int next_tiles, int skip_u4 = 0) {
        const uint4 *w;
        if constexpr (STREAM) {
            fetch(next_tiles, skip_u4);
            __syncthreads();  // the slab is complete in buffer cur; nobody reads buffer cur ^ 1 any more
            w = reinterpret_cast<const uint4 *>(wl + cur * BUF) + (threadIdx.x & 63);
        } else {
            w = reinterpret_cast<const uint4 *>(wcur) + (threadIdx.x & 63);
            wcur += tiles * TILE_U4;
        }
#pragma unroll
        for (int t = 0; t < TMAX; ++t)
            if (t < tiles) bank[t] = mcp_mfma_split(w + t * TILE_U4, xs, bank[t]);
        // The wave-uniform branches around absent tiles leave paths on which this compiler moves a finished tile between register
        // files 8 .. 11 wait states after its last MFMA (12 are needed; its hazard pass does not follow those branch chains, and
        // tools/isa_lint.py finds them).  16 idle issue slots after the slab's last MFMA cover every such path; they pass while the
        // matrix pipe is still busy with that MFMA.
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_nop 15");
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (STREAM) {
            stash(cur ^ 1);
            cur ^= 1;
        }
    }
};

// ---- tile helpers.  Rows of a (rows, 32 * tiles) array in accumulator order: register 4 g + j of tile t is channel 32 t + 8 g + 4 h + j
// (`row` points at channel 4 h of the lane's row).  K-step s of such a row -- registers 8 (s & 1) .. + 7 of tile s >> 1, what
// mcp_split_kstep takes -- is therefore the two quads at 16 s and 16 s + 8, written by this very lane. ----
template <int TMAX>
__device__ __forceinline__ void fp_zero_bank(f32x16 (&bank)[TMAX]) {
#pragma unroll
    for (int t = 0; t < TMAX; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) bank[t][r] = 0.f;
}
// The bank behind a compiler barrier, between a product's k-step loop and an epilogue that holds many loads in flight.  Without it
// the register allocator may split the bank's live range INSIDE the loop: a second copy of every tile, brought up to date by 16
// v_mov per tile and slab -- one more bank of registers and a lower occupancy (tools/isa_resources.py shows it).
template <int TMAX>
__device__ __forceinline__ void fp_pin_bank(f32x16 (&bank)[TMAX]) {
#pragma unroll
    for (int t = 0; t < TMAX; ++t) asm volatile("" : "+v"(bank[t]));
}
// tile t = its bias (zeros for an absent tile); `bias` is the layer's, in accumulator order [t][h][r], in LDS or in the image
__device__ __forceinline__ void fp_bias_tile(f32x16 &tile, int t, int tiles, const float *bias) {
#pragma unroll
    for (int r = 0; r < 16; ++r) tile[r] = 0.f;
    if (t < tiles) {
        const float4 *bq = reinterpret_cast<const float4 *>(bias + (t * 2 + ((threadIdx.x & 63) >> 5)) * 16);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 v = bq[g];
            tile[4 * g + 0] = v.x; tile[4 * g + 1] = v.y; tile[4 * g + 2] = v.z; tile[4 * g + 3] = v.w;
        }
    }
}
__device__ __forceinline__ void fp_store_tile(float *row, int t, const f32x16 &v) {
#pragma unroll
    for (int g = 0; g < 4; ++g) *reinterpret_cast<float4 *>(row + 32 * t + 8 * g) = make_float4(v[4 * g + 0], v[4 * g + 1], v[4 * g + 2], v[4 * g + 3]);
}
struct FpQuads {
    float4 a0, a1;
};
// k-step s of a stored row (zeros when !ok: nothing is read)
__device__ __forceinline__ FpQuads fp_row_kstep(const float *row, int s, bool ok) {
    FpQuads r{make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f)};
    if (ok) {
        r.a0 = *reinterpret_cast<const float4 *>(row + 16 * s);
        r.a1 = *reinterpret_cast<const float4 *>(row + 16 * s + 8);
    }
    return r;
}
// The rolled loop over a layer's input k-steps: what k-step s + 1 reads is in flight while use(raw, s, last) multiplies k-step s.  The
// last k-step loads itself again: no branch in the loop body.
template <class Load, class Use>
__device__ __forceinline__ void fp_ksteps(int ks, Load load, Use use) {
    auto now = load(0);
#pragma unroll 1
    for (int s = 0; s < ks; ++s) {
        const auto nxt = load(min(s + 1, ks - 1));
        use(now, s, s + 1 == ks);
        now = nxt;
    }
}

// tiles c0 .. c0 + tc - 1 of row q of dx = W_1^T gz_1 -> grad_blend (channels below C2) | grad_skip (quad or dword by skip_q)
template <int TMAX>
__device__ __forceinline__ void fp_store_dx(const f32x16 (&bank)[TMAX], int c0, int tc, long long q, int c2, int c1, float *__restrict__ grad_blend,
                                            float *__restrict__ grad_skip) {
    const int h = (threadIdx.x & 63) >> 5;
    const bool skip_q = (c1 & 3) == 0;
#pragma unroll
    for (int t = 0; t < TMAX; ++t) {
        if (t < tc) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int ch = 32 * (c0 + t) + 8 * g + 4 * h;
                const float v0 = bank[t][4 * g + 0], v1 = bank[t][4 * g + 1], v2 = bank[t][4 * g + 2], v3 = bank[t][4 * g + 3];
                if (ch < c2) {   // C2 is a multiple of 4: a quad lies on one side
                    *reinterpret_cast<float4 *>(grad_blend + q * c2 + ch) = make_float4(v0, v1, v2, v3);
                } else {
                    const int cs = ch - c2;
                    float *gs = grad_skip + q * c1 + cs;
                    if (skip_q) {
                        if (cs < c1) *reinterpret_cast<float4 *>(gs) = make_float4(v0, v1, v2, v3);
                    } else {
                        if (cs + 0 < c1) gs[0] = v0;
                        if (cs + 1 < c1) gs[1] = v1;
                        if (cs + 2 < c1) gs[2] = v2;
                        if (cs + 3 < c1) gs[3] = v3;
                    }
                }
            }
        }
    }
}

// ---- host side.  One launch for the three kernel templates: KERN is an instantiation <TMAX, STREAM, ...>, one workgroup per
// 32 * WAVES rows, front_floats of the unit's own LDS in front of the slabs; the LDS attribute is set once per device and instantiation. ----
template <auto KERN, int TMAX, bool STREAM, class... Args>
int fp_launch(long long total, int front_floats, int whole_u4, hipStream_t s, const Args &...args) {
    if (const int rc = mcp_allow_lds<KERN>()) return rc;
    const size_t lds = (size_t)front_floats * sizeof(float) + FpSlabs<TMAX, STREAM>::lds_bytes(whole_u4);
    const long long grid = (total + 32 * WAVES - 1) / (32 * WAVES);
    if (grid > 0x7FFFFFFFLL) return MCP_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(KERN, dim3((unsigned)grid), dim3(THREADS), lds, s, args...);
    return mcp_launch_status();
}
// f(TMAX, STREAM) with the two as compile-time constants (decltype(tmax)::value): the register class and the staging of a call
template <class F>
int fp_dispatch(int tmax, bool stream, F f) {
    using std::integral_constant;
    if (tmax == 2) return stream ? f(integral_constant<int, 2>{}, std::true_type{}) : f(integral_constant<int, 2>{}, std::false_type{});
    if (tmax == 4) return stream ? f(integral_constant<int, 4>{}, std::true_type{}) : f(integral_constant<int, 4>{}, std::false_type{});
    return stream ? f(integral_constant<int, 8>{}, std::true_type{}) : f(integral_constant<int, 8>{}, std::false_type{});
}

}  // namespace
