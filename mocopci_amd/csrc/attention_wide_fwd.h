// attention_wide_fwd.h -- the forward of the wide-head attention (head widths 32 / 64 / 256), stated once for the inference kernels
// (attention_forward.h: attention_wide_kernel, attention_wide_ksplit_kernel and their length forms) and the training kernels (attention_wide_grad.hip:
// attention_wide_lse_kernel, attention_wide_ksplit_lse_kernel).  A kernel is its dynamic LDS declaration and one call of a body.
// The training forward adds two things to the inference one: with `lse` the row's log-sum-exp (log2 domain) is stored, and with DROP
// the hash mask of attention_dropout.h multiplies P in P.V only (row sums are taken before the mask).  Same instruction sequence per
// (query, key) and the same dispatch rule (wide_keys_split), so at drop_p = 0 the training output is the inference output bit for bit.
// Each body ends in a parameter pack that is empty for these kernels and one AttnLengths for their length forms (attention_lengths.h;
// the length wrappers of attention_forward.h and the AttnLengths instantiations of attention_wide_grad.hip): per-element query / key counts of a padded batch.
#pragma once
#include "common.h"
#include "attention_dropout.h"
#include "attention_lengths.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr int WAVES = 4;

// register r of lane half h of an accumulator tile -> its channel: mcp_chan_of (common.h)

// ---- wide heads (32: EI cross-former of level 3, mocopci.py:72-86 with dim 256 / 8 heads; 256: Cross_Frame_Att, whose 4 "heads"
// are C = 256 wide, mocopci.py:499-522) --------------------------------------------------------------------------------
// Both products on fp32 MFMA.  A wave owns 32 queries (MFMA column); per 32-key tile
//   S^T = K . Q^T      : HD/2 v_mfma_f32_32x32x2_f32, A = K tile from LDS (padded rows), B = Q resident in VGPRs (pre-scaled);
//   O^T += V^T . P     : per 32-channel tile of the head, 16 MFMAs whose B operand is the P tile exactly as the softmax left
//                        it in the accumulator layout (k-step r <-> keys mcp_chan_of(r, half)), A = V rows read from LDS in that
//                        same key order; O^T stays in HD/32 accumulator tiles, every register of a lane belongs to that
//                        lane's query, so the online-softmax rescale is lane-local.
// The running maximum is shared by the two lane halves of a query (one cross-half exchange per tile) because both halves feed
// the same MFMA sum; the row sums stay per half and are added once at the end.
template <int HD>
struct WideCfg {
    static constexpr int KT = 32, KS = HD + 1, TD = HD / 32;
    static constexpr size_t LDS_BYTES = 2 * (size_t)KT * (KS + HD) * sizeof(float);
};

// what a length form (attention_lengths.h) writes for a query row at or beyond its element's length, or of an element without keys:
// zeros, each lane half its half of the head's channels, and a zero log-sum-exp
template <int HD>
__device__ __forceinline__ void wide_zero_rows(bool inside, int h, float *dst, float *lse) {
    if (!inside) return;
    attn_zero_row<HD / 2>(dst + h * (HD / 2));
    if (lse && h == 0) *lse = 0.f;
}

// bkv: the batch element whose keys / values the queries of batch element blockIdx.z attend to; os: row stride of out (floats);
// heads, seed, threshold, inv_keep are read only with lse or DROP (row = the query's index over (batch, head, query));
// lens: empty, or one AttnLengths (the key loop then ends at the element's own length kl, rows at or beyond ql are zeros)
template <int HD, bool DROP, class... L>
__device__ __forceinline__ void attention_wide_body(float *lds_w, int nq, int nk, int heads, const float *__restrict__ q, int qs,
                                                    const float *__restrict__ k, int ks, const float *__restrict__ v, int vs, int bkv,
                                                    float scale_log2e, uint32_t seed, uint32_t threshold, float inv_keep,
                                                    float *__restrict__ out, int os, float *__restrict__ lse, L... lens) {
    constexpr bool LEN = sizeof...(L) != 0;
    using C = WideCfg<HD>;
    constexpr int KT = C::KT, KS = C::KS, TD = C::TD;
    float *kt = lds_w;                   // [2][KT][KS]
    float *vt = lds_w + 2 * KT * KS;     // [2][KT][HD]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, col = lane & 31;
    const int head = blockIdx.y, bf = blockIdx.z;
    const int qi = blockIdx.x * (32 * WAVES) + wave * 32 + col;
    const AttnSpan sp = attn_span(nq, nk, bf, bkv, lens...);   // the element's own lengths (nq, nk without)
    const int kl = sp.kl;
    const bool live = qi < sp.ql;
    if constexpr (LEN) {
        // a query block wholly beyond the length, or an element without keys: zeros, before a key is loaded
        if ((int)blockIdx.x * (32 * WAVES) >= sp.ql || kl == 0) {
            wide_zero_rows<HD>(qi < nq, h, out + ((size_t)bf * nq + qi) * os + head * HD, lse ? lse + ((size_t)bf * heads + head) * nq + qi : nullptr);
            return;
        }
    }
    const uint32_t row = (uint32_t)(((size_t)bf * heads + head) * nq + qi);
    q += ((size_t)bf * nq + (live ? qi : 0)) * qs + head * HD;
    k += (size_t)bkv * nk * ks + head * HD;
    v += (size_t)bkv * nk * vs + head * HD;

    float qf[HD / 2];
#pragma unroll
    for (int s4 = 0; s4 < HD / 4; ++s4) {  // Q[query][2s + h]: one float4 holds the operands of two k-steps for both halves
        const float4 t = *reinterpret_cast<const float4 *>(q + 4 * s4);
        qf[2 * s4 + 0] = (h ? t.y : t.x) * scale_log2e;
        qf[2 * s4 + 1] = (h ? t.w : t.z) * scale_log2e;
    }
    f32x16 o[TD];
#pragma unroll
    for (int d = 0; d < TD; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[d][r] = 0.f;
    float m = -INFINITY, l = 0.f;

    // Staging: K and V tiles of the NEXT stage are fetched separately (K under the S MFMAs, V under the P.V MFMAs), so only one
    // tile's worth of registers (HD/8 float4 per thread) is ever in flight -- at HD = 256 both at once would spill.
    constexpr int F4_ROW = HD / 4, F4_TILE = KT * F4_ROW;              // float4s per K (or V) tile
    constexpr int LOADS = (F4_TILE + 64 * WAVES - 1) / (64 * WAVES);
    float4 pre[LOADS];
    auto fetch = [&](int t, const float *src, int stride) {
#pragma unroll
        for (int u = 0; u < LOADS; ++u) {
            const int e = tid + u * 64 * WAVES;
            const int row = e / F4_ROW, c4 = e % F4_ROW, key = t * KT + row;
            pre[u] = make_float4(0.f, 0.f, 0.f, 0.f);  // keys past kl: zero rows (their scores are masked, 0 * 0 stays 0)
            if (e < F4_TILE && key < kl) pre[u] = *reinterpret_cast<const float4 *>(src + (size_t)key * stride + c4 * 4);
        }
    };
    auto stash_k = [&](int buf) {
#pragma unroll
        for (int u = 0; u < LOADS; ++u) {
            const int e = tid + u * 64 * WAVES;
            if (e >= F4_TILE) continue;
            float *dst = &kt[(buf * KT + e / F4_ROW) * KS + (e % F4_ROW) * 4];
            dst[0] = pre[u].x; dst[1] = pre[u].y; dst[2] = pre[u].z; dst[3] = pre[u].w;
        }
    };
    auto stash_v = [&](int buf) {
#pragma unroll
        for (int u = 0; u < LOADS; ++u) {
            const int e = tid + u * 64 * WAVES;
            if (e < F4_TILE) *reinterpret_cast<float4 *>(&vt[(buf * KT + e / F4_ROW) * HD + (e % F4_ROW) * 4]) = pre[u];
        }
    };

    const int stages = (kl + KT - 1) / KT;
    fetch(0, k, ks);
    stash_k(0);
    fetch(0, v, vs);
    stash_v(0);
    for (int t = 0; t < stages; ++t) {
        const int cur = t & 1;
        const bool more = t + 1 < stages;
        __syncthreads();  // stage `cur` is complete; every wave has finished reading stage cur^1 (previous iteration)
        if (more) fetch(t + 1, k, ks);
        const float *ka = &kt[(cur * KT + col) * KS + h];
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
        for (int s = 0; s < HD / 2; ++s) {
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ka[2 * s], qf[s], acc, 0, 0, 0);
            if (HD > 64 && (s & 15) == 15) __builtin_amdgcn_sched_barrier(0);  // keep the LDS operand reads from being hoisted en bloc (registers)
        }
        if (more) {
            stash_k(cur ^ 1);
            fetch(t + 1, v, vs);
        } else {
            // Last stage: nothing sits between the S MFMAs and the first vector read of their result when the tile is also full (the
            // masking below is skipped).  With the accumulators in ordinary VGPRs (-amdgpu-mfma-vgpr-form) this compiler's hazard
            // recogniser left 5 of the 18 wait states a 16-pass MFMA result needs on that path (tools/isa_lint.py found it; every
            // other consumer of an MFMA result in the library has its wait states) -- so they are spelled out here, once per launch
            // and wave.
            asm volatile("s_nop 15\n\ts_nop 1" ::: "memory");
        }
        const int kbase = t * KT;
        if (kbase + KT > kl) {
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (kbase + mcp_chan_of(r, h) >= kl) acc[r] = -INFINITY;
        }
        float mt = acc[0];
#pragma unroll
        for (int r = 1; r < 16; ++r) mt = fmaxf(mt, acc[r]);
        mt = fmaxf(mt, __shfl_xor(mt, 32));          // both halves of a query agree on the maximum (tile 0 always has key 0)
        const float mn = fmaxf(m, mt);
        const float alpha = __builtin_amdgcn_exp2f(m - mn);
        m = mn;
        l *= alpha;
#pragma unroll
        for (int d = 0; d < TD; ++d)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[d][r] *= alpha;
        float p[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            p[r] = __builtin_amdgcn_exp2f(acc[r] - mn);
            l += p[r];
            if (DROP) p[r] *= drop_scale(seed, row, (uint32_t)(kbase + mcp_chan_of(r, h)), threshold, inv_keep);
        }
#pragma unroll
        for (int d = 0; d < TD; ++d) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float a = vt[(cur * KT + mcp_chan_of(r, h)) * HD + 32 * d + col];
                o[d] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, p[r], o[d], 0, 0, 0);
            }
            if (HD > 64) __builtin_amdgcn_sched_barrier(0);
        }
        if (more) stash_v(cur ^ 1);
    }
    const float lsum = l + __shfl_xor(l, 32);
    const float inv = 1.0f / lsum;
    if (live) {
        float *dst = out + ((size_t)bf * nq + qi) * os + head * HD;
#pragma unroll
        for (int d = 0; d < TD; ++d)
#pragma unroll
            for (int g = 0; g < 4; ++g)  // registers 4g..4g+3 = channels 32d + 8g + 4h .. +3
                *reinterpret_cast<float4 *>(dst + 32 * d + 8 * g + 4 * h) =
                    make_float4(o[d][4 * g] * inv, o[d][4 * g + 1] * inv, o[d][4 * g + 2] * inv, o[d][4 * g + 3] * inv);
        if (lse && h == 0) lse[((size_t)bf * heads + head) * nq + qi] = m + __builtin_amdgcn_logf(lsum);  // v_log_f32 is log2
    } else if constexpr (LEN) {
        wide_zero_rows<HD>(qi < nq, h, out + ((size_t)bf * nq + qi) * os + head * HD, lse ? lse + ((size_t)bf * heads + head) * nq + qi : nullptr);
    }
}

// ---- the same attention with the KEYS split over the waves of a workgroup (round 5) --------------------------------------------------
// Cross_Frame_Att (mocopci.py:499-522) is 16 x 3 problems of 256 queries x 256 keys at head width 256: in the kernel above that is 96
// workgroups = 384 waves of 8 key stages each, 55 us of f32-MFMA work per wave on a third of the chip's SIMDs (107 us per launch).  Here a
// workgroup owns 32 queries and its four waves take the 32-key stages w, w + 4, ...: four times the waves, a quarter of the serial MFMA
// chain each.  A wave stages its K tile, then (in the same LDS buffer, once the S MFMAs have read K) its V tile -- the tiles are not
// shared between waves any more, so there is no workgroup barrier in the loop; the four partial results (running maximum, row sums,
// O^T tiles) meet in LDS at the end and wave w finishes the output channels 64 w .. 64 w + 63:
//     M = max_i m_i,  O = sum_i exp2(m_i - M) O_i / sum_i exp2(m_i - M) l_i        (the usual log-sum-exp merge, waves in order).
// Same MFMA sequence per (query, key stage) as attention_wide_kernel; the merge changes the order in which the stages' contributions
// are added, so results agree to rounding (tests: same tolerance against float64), not bit for bit.
template <int HD>
struct WideSplitCfg {
    static constexpr int KT = 32, KS = HD + 1, TD = HD / 32;
    static constexpr int BUF = KT * KS;                                  // floats per wave: K tile (padded rows) or V tile or the wave's O^T
    static constexpr size_t LDS_BYTES = (size_t)WAVES * (BUF + 2 * 64) * sizeof(float);
    static_assert(TD * 16 * 64 <= BUF, "a wave's O^T tiles fit its staging buffer");
    static_assert(TD % WAVES == 0, "output tiles shared out evenly");
};

template <int HD, bool DROP, class... L>
__device__ __forceinline__ void attention_wide_ksplit_body(float *lds_ws, int nq, int nk, int heads, const float *__restrict__ q, int qs,
                                                           const float *__restrict__ k, int ks, const float *__restrict__ v, int vs, int bkv,
                                                           float scale_log2e, uint32_t seed, uint32_t threshold, float inv_keep,
                                                           float *__restrict__ out, int os, float *__restrict__ lse, L... lens) {
    constexpr bool LEN = sizeof...(L) != 0;
    using C = WideSplitCfg<HD>;
    constexpr int KT = C::KT, KS = C::KS, TD = C::TD, BUF = C::BUF;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, col = lane & 31;
    float *buf = lds_ws + wave * BUF;                       // this wave's staging buffer
    float *ml = lds_ws + WAVES * BUF;                       // [WAVES][2][64]: running maximum, row sum
    const int head = blockIdx.y, bf = blockIdx.z;
    const int qi = blockIdx.x * 32 + col;
    // With lengths the key stages are shared out from the element's own kl: a short element leaves waves without a stage (they enter
    // the merge with m = -inf, l = 0 and weigh nothing); one without keys, or a query block beyond ql, is zeros before a key is loaded
    const AttnSpan sp = attn_span(nq, nk, bf, bkv, lens...);
    const int kl = sp.kl;
    const bool live = qi < sp.ql;
    if constexpr (LEN) {
        if ((int)blockIdx.x * 32 >= sp.ql || kl == 0) {
            if (wave == 0) wide_zero_rows<HD>(qi < nq, h, out + ((size_t)bf * nq + qi) * os + head * HD, lse ? lse + ((size_t)bf * heads + head) * nq + qi : nullptr);
            return;
        }
    }
    const uint32_t row = (uint32_t)(((size_t)bf * heads + head) * nq + qi);
    q += ((size_t)bf * nq + (live ? qi : 0)) * qs + head * HD;
    k += (size_t)bkv * nk * ks + head * HD;
    v += (size_t)bkv * nk * vs + head * HD;

    float qf[HD / 2];
#pragma unroll
    for (int s4 = 0; s4 < HD / 4; ++s4) {
        const float4 t = *reinterpret_cast<const float4 *>(q + 4 * s4);
        qf[2 * s4 + 0] = (h ? t.y : t.x) * scale_log2e;
        qf[2 * s4 + 1] = (h ? t.w : t.z) * scale_log2e;
    }
    f32x16 o[TD];
#pragma unroll
    for (int d = 0; d < TD; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[d][r] = 0.f;
    float m = -INFINITY, l = 0.f;

    // A wave stages a 32-key tile by itself: 32 x HD/4 float4 = 32 per lane, all in flight at once and UNDER the MFMA phase in front of
    // their use: the V tile is requested before the S MFMAs, the next stage's K tile before the P.V MFMAs (one round trip per tile,
    // hidden; four dependent round trips of eight loads each, exposed, made the first version of this kernel 85 us)
    constexpr int F4_ROW = HD / 4, PER_LANE = KT * F4_ROW / 64;
    float4 pre[PER_LANE];
    auto issue = [&](int t, const float *src, int stride) {
#pragma unroll
        for (int u = 0; u < PER_LANE; ++u) {
            const int e = u * 64 + lane;
            const int row = e / F4_ROW, c4 = e % F4_ROW, key = t * KT + row;
            pre[u] = key < kl ? *reinterpret_cast<const float4 *>(src + (size_t)key * stride + c4 * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    auto commit = [&](bool padded) {
#pragma unroll
        for (int u = 0; u < PER_LANE; ++u) {
            const int e = u * 64 + lane;
            const int row = e / F4_ROW, c4 = e % F4_ROW;
            if (padded) {
                float *dst = &buf[row * KS + c4 * 4];
                dst[0] = pre[u].x; dst[1] = pre[u].y; dst[2] = pre[u].z; dst[3] = pre[u].w;
            } else {
                *reinterpret_cast<float4 *>(&buf[row * HD + c4 * 4]) = pre[u];
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    };
    const int stages = (kl + KT - 1) / KT;
    if (wave < stages) issue(wave, k, ks);
    for (int t = wave; t < stages; t += WAVES) {
        commit(true);                      // this stage's K tile
        issue(t, v, vs);                   // its V tile: in flight under the S MFMAs
        const float *ka = &buf[col * KS + h];
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
        for (int s = 0; s < HD / 2; ++s) {
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ka[2 * s], qf[s], acc, 0, 0, 0);
            if ((s & 15) == 15) __builtin_amdgcn_sched_barrier(0);
        }
        __builtin_amdgcn_wave_barrier();   // every lane's K reads are issued; LDS serves a wave's accesses in order: V may overwrite the buffer
        commit(false);
        if (t + WAVES < stages) issue(t + WAVES, k, ks);   // the next stage's K tile: in flight under the softmax and the P.V MFMAs
        const int kbase = t * KT;
        if (kbase + KT > kl) {
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (kbase + mcp_chan_of(r, h) >= kl) acc[r] = -INFINITY;
        }
        float mt = acc[0];
#pragma unroll
        for (int r = 1; r < 16; ++r) mt = fmaxf(mt, acc[r]);
        mt = fmaxf(mt, __shfl_xor(mt, 32));
        const float mn = fmaxf(m, mt);
        const float alpha = __builtin_amdgcn_exp2f(m - mn);
        m = mn;
        l *= alpha;
#pragma unroll
        for (int d = 0; d < TD; ++d)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[d][r] *= alpha;
        float p[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            p[r] = __builtin_amdgcn_exp2f(acc[r] - mn);
            l += p[r];
            if (DROP) p[r] *= drop_scale(seed, row, (uint32_t)(kbase + mcp_chan_of(r, h)), threshold, inv_keep);
        }
#pragma unroll
        for (int d = 0; d < TD; ++d) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float a = buf[mcp_chan_of(r, h) * HD + 32 * d + col];
                o[d] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, p[r], o[d], 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        __builtin_amdgcn_wave_barrier();   // V reads issued before the next stage's K tile is written
    }
    // ---- the four partial results meet in LDS ----
    const float lq = l + __shfl_xor(l, 32);   // the query's row sum over this wave's stages (both lane halves)
#pragma unroll
    for (int d = 0; d < TD; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) buf[(d * 16 + r) * 64 + lane] = o[d][r];
    ml[(wave * 2 + 0) * 64 + lane] = m;
    ml[(wave * 2 + 1) * 64 + lane] = lq;
    __syncthreads();
    float mm = -INFINITY;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) mm = fmaxf(mm, ml[(w * 2 + 0) * 64 + lane]);
    float sc[WAVES], lsum = 0.f;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        const float mw = ml[(w * 2 + 0) * 64 + lane];
        sc[w] = mw == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(mw - mm);   // a wave without stages (nk < 32 * WAVES) contributes nothing
        lsum += sc[w] * ml[(w * 2 + 1) * 64 + lane];
    }
    const float inv = 1.0f / lsum;
    if (live) {
        float *dst = out + ((size_t)bf * nq + qi) * os + head * HD;
        constexpr int TPW = TD / WAVES;
#pragma unroll
        for (int dd = 0; dd < TPW; ++dd) {
            const int d = wave * TPW + dd;
            float res[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float a = 0.f;
#pragma unroll
                for (int w = 0; w < WAVES; ++w) a += sc[w] * lds_ws[w * BUF + (d * 16 + r) * 64 + lane];
                res[r] = a * inv;
            }
#pragma unroll
            for (int g = 0; g < 4; ++g)
                *reinterpret_cast<float4 *>(dst + 32 * d + 8 * g + 4 * h) = make_float4(res[4 * g], res[4 * g + 1], res[4 * g + 2], res[4 * g + 3]);
        }
        if (lse && wave == 0 && h == 0) lse[((size_t)bf * heads + head) * nq + qi] = mm + __builtin_amdgcn_logf(lsum);
    } else if constexpr (LEN) {
        if (wave == 0) wide_zero_rows<HD>(qi < nq, h, out + ((size_t)bf * nq + qi) * os + head * HD, lse ? lse + ((size_t)bf * heads + head) * nq + qi : nullptr);
    }
}

// Head width 256: few, long problems -- when the query-stationary form would not cover the chip's 1024 SIMDs and there are key stages
// to share out, the waves of a workgroup split the keys instead
inline bool wide_keys_split(int bf, int nq, int nk, int heads) {
    return (long long)mcp_divup(nq, 32 * WAVES) * heads * bf * WAVES < 1024 && nk >= 32 * WAVES;
}

}  // namespace
