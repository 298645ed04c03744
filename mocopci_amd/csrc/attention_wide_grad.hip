// attention_wide_grad.hip -- training forward (kept log-sum-exp, in-kernel dropout) and backward of the wide-head attention
// (mcp_attention_wide, head widths 32 / 64 / 256) on gfx950.  Callers in a training graph: the CrossAttention of the level-3 EI
// cross-former (mocopci.py:72-86 at dim 256 / 8 heads) and Cross_Frame_Att (mocopci.py:499-522: 16 x 3 head slots of 256 x 256 at
// width 256).  Every product is v_mfma_f32_32x32x2_f32 (exact fp32); nothing of size Nq x Nk is written; every sum has a fixed order.
//
//   forward   the bodies of attention_wide_fwd.h (shared with the inference kernels of attention.hip) with the log-sum-exp output and,
//             with DROP, the dropout mask; at drop_p = 0 the output is mcp_attention_wide's bit for bit.
//   dsum      D = dO . O per (batch, head, query), one elementwise pass.
//   dq        query-stationary: a wave owns 32 queries on the MFMA column, keys stream through LDS in 32-key tiles:
//             S^T = K Q^T, dP^T = V dO^T, p = exp2(s - L), ds = p (m dP - D), dQ^T += K^T ds  (ds stays in the accumulator layout
//             and is the B operand of the last product through mcp_chan_of, as P is in the forward).
//   dkv       key-stationary, the same with the roles exchanged: S = Q K^T, dP = dO V^T, dV^T += dO^T (m p), dK^T += Q^T ds.
//             In all three the score's factor scale * log2 e sits on Q, so at head widths 32 / 64 (no channel split) the backward's s
//             is the forward's bit for bit and p = exp2(s - L) is exactly the P the forward normalised.
//
// Head width 256 does not fit one wave's registers (dkv: K, V as operands and dK^T, dV^T as accumulators are 512 before anything else),
// so there the CHANNELS are split over the four waves of a workgroup: the workgroup owns one block of 32 rows, wave w the channels
// 64 w .. 64 w + 63.  S and dP contract over all channels: each wave forms the partial sums of its slice (from its own slice of the
// streamed tile -- no tile is shared), the four partials meet in LDS and every wave adds them in wave order, so all four hold the same
// bits.  The products with HD output columns need no merge at all: a wave owns its 64 output channels outright.  MFMA count per tile pair
// is the unsplit one (3 HD/2 for dq, 4 HD/2 for dkv), registers per wave are those of head width 64, and the 16 x 3 x 256 x 256 call of
// the training step is 384 workgroups instead of 96.  Head widths 32 / 64: no split, a workgroup is four independent waves.
#include "common.h"
#include "attention_wide_fwd.h"  // f32x16, WAVES, drop_scale; the forward bodies

namespace {

// =====================================================================================================================================
// forward
// =====================================================================================================================================
// out is dense (row stride heads * HD), keys / values are the batch element's own
// L: empty, or one AttnLengths (attention_lengths.h) -- the length forms of mcp_attention_wide_lse_lengths
template <int HD, bool DROP, class... L>
__global__ __launch_bounds__(64 * WAVES, 1) void attention_wide_lse_kernel(int nq, int nk, int heads, const float *__restrict__ q, int qs,
                                                                           const float *__restrict__ k, int ks, const float *__restrict__ v, int vs,
                                                                           float scale_log2e, uint32_t seed, uint32_t threshold, float inv_keep,
                                                                           float *__restrict__ out, float *__restrict__ lse, L... lens) {
    extern __shared__ __attribute__((aligned(16))) float lds_w[];
    attention_wide_body<HD, DROP>(lds_w, nq, nk, heads, q, qs, k, ks, v, vs, (int)blockIdx.z, scale_log2e, seed, threshold, inv_keep, out, heads * HD,
                                  lse, lens...);
}

// the keys split over the waves of a workgroup
template <int HD, bool DROP, class... L>
__global__ __launch_bounds__(64 * WAVES, 1) void attention_wide_ksplit_lse_kernel(int nq, int nk, int heads, const float *__restrict__ q, int qs,
                                                                                  const float *__restrict__ k, int ks, const float *__restrict__ v, int vs,
                                                                                  float scale_log2e, uint32_t seed, uint32_t threshold, float inv_keep,
                                                                                  float *__restrict__ out, float *__restrict__ lse, L... lens) {
    extern __shared__ __attribute__((aligned(16))) float lds_ws[];
    attention_wide_ksplit_body<HD, DROP>(lds_ws, nq, nk, heads, q, qs, k, ks, v, vs, (int)blockIdx.z, scale_log2e, seed, threshold, inv_keep, out,
                                         heads * HD, lse, lens...);
}

// lens: empty, or one AttnLengths; the key-split dispatch is decided from the padded sizes either way (the host never reads a length)
template <int HD, bool DROP, class... L>
int launch_forward(int bf, int nq, int nk, int heads, const float *q, int qs, const float *k, int ks, const float *v, int vs, float sl2, uint32_t seed,
                   uint32_t threshold, float inv_keep, float *out, float *lse, hipStream_t s, L... lens) {
    if constexpr (HD == 256) {
        if (wide_keys_split(bf, nq, nk, heads)) {
            constexpr auto kern = attention_wide_ksplit_lse_kernel<HD, DROP, L...>;
            if (const int rc = mcp_allow_lds<kern>()) return rc;
            hipLaunchKernelGGL(kern, dim3(mcp_divup(nq, 32), heads, bf), dim3(64 * WAVES), WideSplitCfg<HD>::LDS_BYTES, s, nq, nk, heads, q, qs, k, ks, v, vs,
                               sl2, seed, threshold, inv_keep, out, lse, lens...);
            return mcp_launch_status();
        }
    }
    constexpr auto kern = attention_wide_lse_kernel<HD, DROP, L...>;
    if (const int rc = mcp_allow_lds<kern>()) return rc;
    hipLaunchKernelGGL(kern, dim3(mcp_divup(nq, 32 * WAVES), heads, bf), dim3(64 * WAVES), WideCfg<HD>::LDS_BYTES, s, nq, nk, heads, q, qs, k, ks, v, vs, sl2,
                       seed, threshold, inv_keep, out, lse, lens...);
    return mcp_launch_status();
}

// =====================================================================================================================================
// backward
// =====================================================================================================================================
template <int HD>
struct GradCfg {
    static constexpr int SPLIT = HD > 64 ? WAVES : 1;        // waves that share one block of 32 rows, each a slice of the channels
    static constexpr int CW = HD / SPLIT;                    // channels per wave
    static constexpr int TD = CW / 32;                       // 32-channel output tiles per wave
    static constexpr int RS = CW + 1;                        // padded row stride of a staged tile: row reads and column reads conflict-free
    static constexpr int TILE = 32 * RS;                     // floats of one staged tile (32 rows of the wave's channel slice)
    static constexpr int WAVE_FLOATS = 2 * TILE + 64;        // two tiles + the streamed rows' statistics (dkv)
    static constexpr int XCH = SPLIT > 1 ? WAVES * 2 * 16 * 64 : 0;   // partial S and dP tiles of the four waves
    static constexpr int RPW = WAVES / SPLIT;                // 32-row blocks per workgroup
    static constexpr int PER = 32 * (CW / 4) / 64;           // float4s per lane and staged tile
    static constexpr size_t LDS_BYTES = ((size_t)WAVES * WAVE_FLOATS + XCH) * sizeof(float);
    static_assert(CW % 32 == 0 && LDS_BYTES <= 160 * 1024, "slices are whole MFMA tiles; the workgroup's LDS fits a CU");
};

// D = dO . O per (batch, head, query): HD / 4 lanes per row, one float4 each, a butterfly over the row's lanes (fixed order)
template <int HD>
__global__ __launch_bounds__(256) void attention_wide_dsum_kernel(long long rows, int heads, const float *__restrict__ out, const float *__restrict__ gout, int nq,
                                                                  float *__restrict__ dsum) {
    constexpr int LPR = HD / 4;
    // row = (batch, query, head) in the memory order of out / gout; dsum is (batch, head, query)
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x, r_ = e / LPR;
    const int c4 = (int)(e % LPR);
    float d = 0.f;
    if (r_ < rows) {
        const float4 a = *reinterpret_cast<const float4 *>(gout + r_ * HD + c4 * 4), b = *reinterpret_cast<const float4 *>(out + r_ * HD + c4 * 4);
        d = __builtin_fmaf(a.w, b.w, __builtin_fmaf(a.z, b.z, __builtin_fmaf(a.y, b.y, a.x * b.x)));
    }
#pragma unroll
    for (int o = LPR / 2; o > 0; o >>= 1) d += __shfl_xor(d, o);
    if (r_ < rows && c4 == 0) {
        const long long bq = r_ / heads;
        const int head = (int)(r_ - bq * heads);
        const long long bfi = bq / nq;
        const int qi = (int)(bq - bfi * nq);
        dsum[(bfi * heads + head) * nq + qi] = d;
    }
}

// Staging of a wave's own tiles: 32 rows x CW channels of two row-major sources, global -> registers (in flight under the MFMAs of the
// tile in front) -> the wave's LDS buffers (padded rows).  Rows at or past `n` are zero.  The first source may be multiplied by a
// constant on its way into LDS.
template <int CW, int PER>
__device__ __forceinline__ void tile_issue(float4 (&pa)[PER], float4 (&pb)[PER], int lane, int t, int n, const float *a, size_t as, const float *b, size_t bs) {
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        const int e = u * 64 + lane, r_ = e / (CW / 4), c4 = e % (CW / 4), row = t * 32 + r_;
        pa[u] = row < n ? *reinterpret_cast<const float4 *>(a + (size_t)row * as + c4 * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        pb[u] = row < n ? *reinterpret_cast<const float4 *>(b + (size_t)row * bs + c4 * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}
template <int CW, int PER>
__device__ __forceinline__ void tile_commit(const float4 (&pa)[PER], const float4 (&pb)[PER], int lane, float *ta, float *tb, float fa = 1.0f) {
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        const int e = u * 64 + lane, r_ = e / (CW / 4), c4 = e % (CW / 4);
        float *da = &ta[r_ * (CW + 1) + c4 * 4], *db = &tb[r_ * (CW + 1) + c4 * 4];
        da[0] = pa[u].x * fa; da[1] = pa[u].y * fa; da[2] = pa[u].z * fa; da[3] = pa[u].w * fa;   // fa: the pre-scaling of a streamed Q tile (dkv)
        db[0] = pb[u].x; db[1] = pb[u].y; db[2] = pb[u].z; db[3] = pb[u].w;
    }
}

// The partial S and dP tiles of the four channel slices -> their sums, added in wave order (the same bits in every wave)
__device__ __forceinline__ void merge_partials(float *xch, int wave, int lane, f32x16 &acc, f32x16 &accp) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        xch[((wave * 2 + 0) * 16 + r) * 64 + lane] = acc[r];
        xch[((wave * 2 + 1) * 16 + r) * 64 + lane] = accp[r];
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        float a = xch[((0 * 2 + 0) * 16 + r) * 64 + lane], b = xch[((0 * 2 + 1) * 16 + r) * 64 + lane];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) {
            a += xch[((w * 2 + 0) * 16 + r) * 64 + lane];
            b += xch[((w * 2 + 1) * 16 + r) * 64 + lane];
        }
        acc[r] = a;
        accp[r] = b;
    }
    __syncthreads();   // every wave has read the partials before the next tile's are written
}

// ---- dq: query-stationary ----
// L: empty, or one AttnLengths: the key loop ends at the element's kl, rows at or beyond ql are zeros.  L and D of a row at or beyond
// ql (the dsum pass covers the padded tensor, so D may be anything there) are never read: lanes past ql take row 0 of the element.
template <int HD, bool DROP, class... LN>
__global__ __launch_bounds__(64 * WAVES, 1) void attention_wide_dq_kernel(int nq, int nk, int heads, const float *__restrict__ q, int qs,
                                                                          const float *__restrict__ k, int ks, const float *__restrict__ v, int vs,
                                                                          float scale_log2e, float scale, uint32_t seed, uint32_t threshold, float inv_keep,
                                                                          const float *__restrict__ gout, const float *__restrict__ lse,
                                                                          const float *__restrict__ dsum, float *__restrict__ dq, LN... lens) {
    constexpr bool LEN = sizeof...(LN) != 0;   // (L is the row's log-sum-exp below)
    using C = GradCfg<HD>;
    constexpr int SPLIT = C::SPLIT, CW = C::CW, TD = C::TD, RS = C::RS, PER = C::PER;
    extern __shared__ __attribute__((aligned(16))) float lds_g[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, col = lane & 31;
    const int part = wave % SPLIT, rb = blockIdx.x * C::RPW + wave / SPLIT;
    if (SPLIT == 1 && rb * 32 >= nq) return;   // independent waves: no workgroup barrier below
    float *kt = lds_g + wave * C::WAVE_FLOATS, *vt = kt + C::TILE;   // K slice: A operand of S by rows, of dQ^T by columns; V slice: A operand of dP
    float *xch = lds_g + WAVES * C::WAVE_FLOATS;
    const int head = blockIdx.y, bf = blockIdx.z;
    const int qi = rb * 32 + col;
    const AttnSpan sp = attn_span(nq, nk, bf, bf, lens...);
    const int kl = sp.kl;
    const bool live = qi < sp.ql;
    const size_t qrow = (size_t)bf * nq + (live ? qi : 0);
    const int c0 = head * HD + part * CW;
    if constexpr (LEN) {
        if (rb * 32 >= sp.ql) {   // the row block (one per wave, or one per workgroup with the channel split) lies beyond the length: zeros
            if (qi < nq) attn_zero_row<CW / 2>(dq + ((size_t)bf * nq + qi) * (size_t)(heads * HD) + c0 + h * (CW / 2));
            return;
        }
    }
    const float *qp = q + qrow * qs + c0, *gp = gout + qrow * (size_t)(heads * HD) + c0;
    k += (size_t)bf * nk * ks + c0;
    v += (size_t)bf * nk * vs + c0;
    const size_t so = ((size_t)bf * heads + head) * nq + (live ? qi : 0);
    const float L = lse[so], D = dsum[so];
    const uint32_t drow = (uint32_t)(((size_t)bf * heads + head) * nq + qi);

    float qf[CW / 2], gf[CW / 2];   // B operands: Q (pre-scaled: s in the log2 domain) and dO of this lane's query, channels 2s + h of the slice
#pragma unroll
    for (int s4 = 0; s4 < CW / 4; ++s4) {
        const float4 a = *reinterpret_cast<const float4 *>(qp + 4 * s4), b = *reinterpret_cast<const float4 *>(gp + 4 * s4);
        qf[2 * s4 + 0] = (h ? a.y : a.x) * scale_log2e;
        qf[2 * s4 + 1] = (h ? a.w : a.z) * scale_log2e;
        gf[2 * s4 + 0] = h ? b.y : b.x;
        gf[2 * s4 + 1] = h ? b.w : b.z;
    }
    f32x16 acc_q[TD];
#pragma unroll
    for (int d = 0; d < TD; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc_q[d][r] = 0.f;

    float4 pk[PER], pv[PER];
    const int stages = (kl + 31) / 32;
    tile_issue<CW, PER>(pk, pv, lane, 0, kl, k, (size_t)ks, v, (size_t)vs);
    for (int t = 0; t < stages; ++t) {
        tile_commit<CW, PER>(pk, pv, lane, kt, vt);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (t + 1 < stages) tile_issue<CW, PER>(pk, pv, lane, t + 1, kl, k, (size_t)ks, v, (size_t)vs);
        const float *ka = &kt[col * RS + h], *va = &vt[col * RS + h];
        f32x16 acc, accp;
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc[r] = 0.f; accp[r] = 0.f; }
#pragma unroll
        for (int s = 0; s < CW / 2; ++s) {
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ka[2 * s], qf[s], acc, 0, 0, 0);     // S^T[key][query]
            accp = __builtin_amdgcn_mfma_f32_32x32x2f32(va[2 * s], gf[s], accp, 0, 0, 0);   // dP^T[key][query] = V_key . dO_query
        }
        if (SPLIT > 1) merge_partials(xch, wave, lane, acc, accp);
        const int kbase = t * 32;
        float ds[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key = kbase + mcp_chan_of(r, h);
            float p = __builtin_amdgcn_exp2f(acc[r] - L);
            if (key >= kl) p = 0.f;
            const float mk = DROP ? drop_scale(seed, drow, (uint32_t)key, threshold, inv_keep) : 1.0f;
            ds[r] = p * ((DROP ? mk * accp[r] : accp[r]) - D);
        }
#pragma unroll
        for (int d = 0; d < TD; ++d)
#pragma unroll
            for (int r = 0; r < 16; ++r)   // dQ^T[channel][query] += K[key][channel] ds[key][query]; k-step r <-> keys mcp_chan_of(r, half)
                acc_q[d] = __builtin_amdgcn_mfma_f32_32x32x2f32(kt[mcp_chan_of(r, h) * RS + 32 * d + col], ds[r], acc_q[d], 0, 0, 0);
        __builtin_amdgcn_wave_barrier();   // this tile's LDS reads are issued before the next tile is written (a wave's LDS accesses are served in order)
    }
    if constexpr (LEN) {
        // The length form's exit from the tile loop runs into the scaled stores of acc_q without the wait states a 16-pass MFMA result
        // needs before a vector read (tools/isa_lint.py found 13 of 18 on that path; the same gap of this compiler's hazard recogniser as
        // in attention_wide_body, attention_wide_fwd.h) -- spelled out here, once per launch and wave.  The plain kernel's layout has them.
        asm volatile("s_nop 15\n\ts_nop 1" ::: "memory");
    }
    if (live) {
        float *dst = dq + qrow * (size_t)(heads * HD) + c0;
#pragma unroll
        for (int d = 0; d < TD; ++d)
#pragma unroll
            for (int g = 0; g < 4; ++g)  // registers 4g..4g+3 = channels 32d + 8g + 4h .. +3
                *reinterpret_cast<float4 *>(dst + 32 * d + 8 * g + 4 * h) =
                    make_float4(acc_q[d][4 * g] * scale, acc_q[d][4 * g + 1] * scale, acc_q[d][4 * g + 2] * scale, acc_q[d][4 * g + 3] * scale);
    } else if constexpr (LEN) {
        if (qi < nq) attn_zero_row<CW / 2>(dq + ((size_t)bf * nq + qi) * (size_t)(heads * HD) + c0 + h * (CW / 2));
    }
}

// ---- dkv: key-stationary; writes dK | dV into a (BF, Nk, 2 heads HD) tensor laid out like the forward's kv ----
// L: empty, or one AttnLengths: the query loop ends at the element's ql (no L, D, Q or dO row beyond it is loaded), rows at or beyond kl
// are zeros in both halves.
template <int HD, bool DROP, class... L>
__global__ __launch_bounds__(64 * WAVES, 1) void attention_wide_dkv_kernel(int nq, int nk, int heads, const float *__restrict__ q, int qs,
                                                                           const float *__restrict__ k, int ks, const float *__restrict__ v, int vs,
                                                                           float scale_log2e, float k_scale, uint32_t seed, uint32_t threshold, float inv_keep,
                                                                           const float *__restrict__ gout, const float *__restrict__ lse,
                                                                           const float *__restrict__ dsum, float *__restrict__ dkv, L... lens) {
    constexpr bool LEN = sizeof...(L) != 0;
    using C = GradCfg<HD>;
    constexpr int SPLIT = C::SPLIT, CW = C::CW, TD = C::TD, RS = C::RS, PER = C::PER;
    extern __shared__ __attribute__((aligned(16))) float lds_g[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, col = lane & 31;
    const int part = wave % SPLIT, rb = blockIdx.x * C::RPW + wave / SPLIT;
    if (SPLIT == 1 && rb * 32 >= nk) return;
    float *qt = lds_g + wave * C::WAVE_FLOATS, *gt = qt + C::TILE, *st = gt + C::TILE;   // Q slice, dO slice, [L | D] of the tile's 32 queries
    float *xch = lds_g + WAVES * C::WAVE_FLOATS;
    const int head = blockIdx.y, bf = blockIdx.z;
    const int ki = rb * 32 + col;
    const bool live = ki < attn_klen(nk, bf, lens...);
    const size_t krow = (size_t)bf * nk + (live ? ki : 0);
    const int c0 = head * HD + part * CW;
    const int ql = attn_qlen(nq, bf, lens...);
    if constexpr (LEN) {
        if (rb * 32 >= attn_klen(nk, bf, lens...)) {   // the key block lies beyond the length: zeros in dK and dV
            if (ki < nk) {
                float *z = dkv + ((size_t)bf * nk + ki) * (size_t)(2 * heads * HD) + c0 + h * (CW / 2);
                attn_zero_row<CW / 2>(z);
                attn_zero_row<CW / 2>(z + heads * HD);
            }
            return;
        }
    }
    const float *kp = k + krow * ks + c0, *vp = v + krow * vs + c0;
    q += (size_t)bf * nq * qs + c0;
    gout += (size_t)bf * nq * (size_t)(heads * HD) + c0;
    lse += ((size_t)bf * heads + head) * nq;
    dsum += ((size_t)bf * heads + head) * nq;
    const uint32_t rbase = (uint32_t)(((size_t)bf * heads + head) * nq);

    // B operands: K and V of this lane's key.  The score's factor scale * log2 e goes on the streamed Q tile, as the forward and the dq
    // kernel put it on Q: every product (q c) k is then the forward's, and without the channel split (head widths 32 / 64) so is their
    // order -- s is the forward's bit for bit, p = exp2(s - L) is the forward's P.  dK^T accumulates ds (q c) and is scaled by scale / c.
    float kf[CW / 2], vf[CW / 2];
#pragma unroll
    for (int s4 = 0; s4 < CW / 4; ++s4) {
        const float4 a = *reinterpret_cast<const float4 *>(kp + 4 * s4), b = *reinterpret_cast<const float4 *>(vp + 4 * s4);
        kf[2 * s4 + 0] = h ? a.y : a.x;
        kf[2 * s4 + 1] = h ? a.w : a.z;
        vf[2 * s4 + 0] = h ? b.y : b.x;
        vf[2 * s4 + 1] = h ? b.w : b.z;
    }
    f32x16 acc_k[TD], acc_v[TD];
#pragma unroll
    for (int d = 0; d < TD; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc_k[d][r] = 0.f; acc_v[d][r] = 0.f; }

    float4 pq[PER], pg[PER];
    float pstat = 0.f;
    auto issue_stat = [&](int t) {   // lanes 0..31: the queries' log-sum-exp, lanes 32..63: their D; a query past ql contributes p = exp2(s - inf) = 0
        const int qq = t * 32 + col;
        pstat = qq < ql ? (h ? dsum[qq] : lse[qq]) : (h ? 0.f : INFINITY);
    };
    const int stages = (ql + 31) / 32;
    tile_issue<CW, PER>(pq, pg, lane, 0, ql, q, (size_t)qs, gout, (size_t)(heads * HD));
    issue_stat(0);
    for (int t = 0; t < stages; ++t) {
        tile_commit<CW, PER>(pq, pg, lane, qt, gt, scale_log2e);
        st[lane] = pstat;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (t + 1 < stages) {
            tile_issue<CW, PER>(pq, pg, lane, t + 1, ql, q, (size_t)qs, gout, (size_t)(heads * HD));
            issue_stat(t + 1);
        }
        const float *qa = &qt[col * RS + h], *ga = &gt[col * RS + h];
        f32x16 acc, accp;
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc[r] = 0.f; accp[r] = 0.f; }
#pragma unroll
        for (int s = 0; s < CW / 2; ++s) {
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(qa[2 * s], kf[s], acc, 0, 0, 0);     // S[query][key]: rows = the tile's queries, column = this lane's key
            accp = __builtin_amdgcn_mfma_f32_32x32x2f32(ga[2 * s], vf[s], accp, 0, 0, 0);   // dP[query][key] = dO_query . V_key
        }
        if (SPLIT > 1) merge_partials(xch, wave, lane, acc, accp);
        float pm[16], ds[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int qq = mcp_chan_of(r, h);
            const float p = __builtin_amdgcn_exp2f(acc[r] - st[qq]);
            const float mk = DROP ? drop_scale(seed, rbase + (uint32_t)(t * 32 + qq), (uint32_t)ki, threshold, inv_keep) : 1.0f;
            pm[r] = DROP ? p * mk : p;
            ds[r] = p * ((DROP ? mk * accp[r] : accp[r]) - st[32 + qq]);
        }
#pragma unroll
        for (int d = 0; d < TD; ++d)
#pragma unroll
            for (int r = 0; r < 16; ++r) {   // k-step r <-> queries mcp_chan_of(r, half)
                acc_v[d] = __builtin_amdgcn_mfma_f32_32x32x2f32(gt[mcp_chan_of(r, h) * RS + 32 * d + col], pm[r], acc_v[d], 0, 0, 0);   // dV^T += dO^T (m p)
                acc_k[d] = __builtin_amdgcn_mfma_f32_32x32x2f32(qt[mcp_chan_of(r, h) * RS + 32 * d + col], ds[r], acc_k[d], 0, 0, 0);   // dK^T += Q^T ds
            }
        __builtin_amdgcn_wave_barrier();
    }
    if (live) {
        float *dst = dkv + krow * (size_t)(2 * heads * HD) + c0;
#pragma unroll
        for (int d = 0; d < TD; ++d)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                *reinterpret_cast<float4 *>(dst + 32 * d + 8 * g + 4 * h) =
                    make_float4(acc_k[d][4 * g] * k_scale, acc_k[d][4 * g + 1] * k_scale, acc_k[d][4 * g + 2] * k_scale, acc_k[d][4 * g + 3] * k_scale);
                *reinterpret_cast<float4 *>(dst + heads * HD + 32 * d + 8 * g + 4 * h) =
                    make_float4(acc_v[d][4 * g], acc_v[d][4 * g + 1], acc_v[d][4 * g + 2], acc_v[d][4 * g + 3]);
            }
    } else if constexpr (LEN) {
        if (ki < nk) {
            float *z = dkv + ((size_t)bf * nk + ki) * (size_t)(2 * heads * HD) + c0 + h * (CW / 2);
            attn_zero_row<CW / 2>(z);
            attn_zero_row<CW / 2>(z + heads * HD);
        }
    }
}

template <int HD, bool DROP, class... L>
int launch_backward(int bf, int nq, int nk, int heads, const float *q, int qs, const float *k, int ks, const float *v, int vs, float scale, uint32_t seed,
                    uint32_t threshold, float inv_keep, const float *out, const float *gout, const float *lse, float *dq, float *dkv, float *dsum,
                    hipStream_t s, L... lens) {
    using C = GradCfg<HD>;
    const float sl2 = scale * 1.44269504088896340736f;
    constexpr auto kq = attention_wide_dq_kernel<HD, DROP, L...>;
    constexpr auto kk = attention_wide_dkv_kernel<HD, DROP, L...>;
    if (const int rc = mcp_allow_lds<kq>()) return rc;
    if (const int rc = mcp_allow_lds<kk>()) return rc;
    const long long rows = (long long)bf * nq * heads;
    hipLaunchKernelGGL(attention_wide_dsum_kernel<HD>, dim3((unsigned)((rows * (HD / 4) + 255) / 256)), dim3(256), 0, s, rows, heads, out, gout, nq, dsum);
    hipLaunchKernelGGL(kq, dim3(mcp_divup(nq, 32 * C::RPW), heads, bf), dim3(64 * WAVES), C::LDS_BYTES, s, nq, nk, heads, q, qs, k, ks, v, vs, sl2, scale, seed,
                       threshold, inv_keep, gout, lse, dsum, dq, lens...);
    hipLaunchKernelGGL(kk, dim3(mcp_divup(nk, 32 * C::RPW), heads, bf), dim3(64 * WAVES), C::LDS_BYTES, s, nq, nk, heads, q, qs, k, ks, v, vs, sl2, 0.69314718055994530942f /* scale / sl2 */,
                       seed, threshold, inv_keep, gout, lse, dsum, dkv, lens...);
    return mcp_launch_status();
}

template <class... L>
int forward_with(int bf, int nq, int nk, int heads, int hd, const float *q, int q_stride, const float *k, int k_stride, const float *v, int v_stride,
                 float scale, float drop_p, unsigned seed, float *out, float *lse, mcp_stream_t stream, L... lens) {
    MCP_CHECK_ARGS(bf > 0 && nq > 0 && nk > 0 && heads > 0 && q && k && v && out);
    if (hd != 32 && hd != 64 && hd != 256) return MCP_ERR_UNSUPPORTED;
    if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out) & 15) return MCP_ERR_BAD_ARG;
    if ((q_stride | k_stride | v_stride) & 3) return MCP_ERR_BAD_ARG;
    uint32_t threshold;
    float inv_keep;
    if (!drop_params(drop_p, &threshold, &inv_keep)) return MCP_ERR_BAD_ARG;
    hipStream_t s = (hipStream_t)stream;
    const float sl2 = scale * 1.44269504088896340736f;
    int rc;
    mcp_prof_begin(MCP_KERNEL_ATTENTION, s);
#define MCP_ATT_ARGS bf, nq, nk, heads, q, q_stride, k, k_stride, v, v_stride, sl2, seed, threshold, inv_keep, out, lse, s, lens...
    if (drop_p > 0.f) rc = hd == 32 ? launch_forward<32, true>(MCP_ATT_ARGS) : hd == 64 ? launch_forward<64, true>(MCP_ATT_ARGS) : launch_forward<256, true>(MCP_ATT_ARGS);
    else rc = hd == 32 ? launch_forward<32, false>(MCP_ATT_ARGS) : hd == 64 ? launch_forward<64, false>(MCP_ATT_ARGS) : launch_forward<256, false>(MCP_ATT_ARGS);
#undef MCP_ATT_ARGS
    mcp_prof_end(MCP_KERNEL_ATTENTION, s);
    return rc;
}

template <class... L>
int backward_with(int bf, int nq, int nk, int heads, int hd, const float *q, int q_stride, const float *k, int k_stride, const float *v, int v_stride,
                  float scale, float drop_p, unsigned seed, const float *out, const float *grad_out, const float *lse, float *grad_q, float *grad_kv,
                  void *workspace, size_t workspace_bytes, mcp_stream_t stream, L... lens) {
    MCP_CHECK_ARGS(bf > 0 && nq > 0 && nk > 0 && heads > 0 && q && k && v && out && grad_out && lse && grad_q && grad_kv && workspace);
    if (hd != 32 && hd != 64 && hd != 256) return MCP_ERR_UNSUPPORTED;
    if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out | (uintptr_t)grad_out | (uintptr_t)grad_q | (uintptr_t)grad_kv) & 15) return MCP_ERR_BAD_ARG;
    if (((uintptr_t)lse | (uintptr_t)workspace) & 3) return MCP_ERR_BAD_ARG;   // scalar float accesses only
    if ((q_stride | k_stride | v_stride) & 3) return MCP_ERR_BAD_ARG;
    if (workspace_bytes < mcp_attention_wide_grad_workspace_bytes(bf, nq, nk, heads, hd)) return MCP_ERR_BAD_ARG;
    uint32_t threshold;
    float inv_keep;
    if (!drop_params(drop_p, &threshold, &inv_keep)) return MCP_ERR_BAD_ARG;
    hipStream_t s = (hipStream_t)stream;
    float *dsum = static_cast<float *>(workspace);
    mcp_prof_begin(MCP_KERNEL_ATTENTION, s);
    int rc;
#define MCP_ATT_ARGS bf, nq, nk, heads, q, q_stride, k, k_stride, v, v_stride, scale, seed, threshold, inv_keep, out, grad_out, lse, grad_q, grad_kv, dsum, s, lens...
    if (drop_p > 0.f) rc = hd == 32 ? launch_backward<32, true>(MCP_ATT_ARGS) : hd == 64 ? launch_backward<64, true>(MCP_ATT_ARGS) : launch_backward<256, true>(MCP_ATT_ARGS);
    else rc = hd == 32 ? launch_backward<32, false>(MCP_ATT_ARGS) : hd == 64 ? launch_backward<64, false>(MCP_ATT_ARGS) : launch_backward<256, false>(MCP_ATT_ARGS);
#undef MCP_ATT_ARGS
    mcp_prof_end(MCP_KERNEL_ATTENTION, s);
    return rc;
}

}  // namespace

MCP_EXPORT int mcp_attention_wide_dropout(int bf, int nq, int nk, int heads, int hd, const float *q, int q_stride, const float *k, int k_stride,
                                          const float *v, int v_stride, float scale, float drop_p, unsigned seed, float *out, mcp_stream_t stream) {
    return forward_with(bf, nq, nk, heads, hd, q, q_stride, k, k_stride, v, v_stride, scale, drop_p, seed, out, nullptr, stream);
}

MCP_EXPORT int mcp_attention_wide_lse(int bf, int nq, int nk, int heads, int hd, const float *q, int q_stride, const float *k, int k_stride,
                                      const float *v, int v_stride, float scale, float drop_p, unsigned seed, float *out, float *lse,
                                      mcp_stream_t stream) {
    MCP_CHECK_ARGS(lse && !((uintptr_t)lse & 3));   // scalar float stores only
    return forward_with(bf, nq, nk, heads, hd, q, q_stride, k, k_stride, v, v_stride, scale, drop_p, seed, out, lse, stream);
}

MCP_EXPORT size_t mcp_attention_wide_grad_workspace_bytes(int bf, int nq, int nk, int heads, int hd) {
    if (bf <= 0 || nq <= 0 || nk <= 0 || heads <= 0 || hd <= 0) return 0;
    return (size_t)bf * heads * nq * sizeof(float);   // D = dO . O per (batch, head, query)
}

MCP_EXPORT int mcp_attention_wide_grad_lse(int bf, int nq, int nk, int heads, int hd, const float *q, int q_stride, const float *k, int k_stride,
                                           const float *v, int v_stride, float scale, float drop_p, unsigned seed, const float *out, const float *grad_out,
                                           const float *lse, float *grad_q, float *grad_kv, void *workspace, size_t workspace_bytes, mcp_stream_t stream) {
    return backward_with(bf, nq, nk, heads, hd, q, q_stride, k, k_stride, v, v_stride, scale, drop_p, seed, out, grad_out, lse, grad_q, grad_kv, workspace,
                         workspace_bytes, stream);
}

// ---- per-element lengths (attention_lengths.h); both arrays NULL: the plain calls above ----
MCP_EXPORT int mcp_attention_wide_lse_lengths(int bf, int nq, int nk, int heads, int hd, const float *q, int q_stride, const float *k, int k_stride,
                                              const float *v, int v_stride, float scale, float drop_p, unsigned seed, float *out, float *lse,
                                              const int *qlen, const int *klen, mcp_stream_t stream) {
    if (((uintptr_t)lse | (uintptr_t)qlen | (uintptr_t)klen) & 3) return MCP_ERR_BAD_ARG;   // scalar accesses only
    if (!qlen && !klen) return forward_with(bf, nq, nk, heads, hd, q, q_stride, k, k_stride, v, v_stride, scale, drop_p, seed, out, lse, stream);
    return forward_with(bf, nq, nk, heads, hd, q, q_stride, k, k_stride, v, v_stride, scale, drop_p, seed, out, lse, stream, AttnLengths{qlen, klen});
}

MCP_EXPORT int mcp_attention_wide_grad_lse_lengths(int bf, int nq, int nk, int heads, int hd, const float *q, int q_stride, const float *k, int k_stride,
                                                   const float *v, int v_stride, float scale, float drop_p, unsigned seed, const float *out,
                                                   const float *grad_out, const float *lse, float *grad_q, float *grad_kv, void *workspace,
                                                   size_t workspace_bytes, const int *qlen, const int *klen, mcp_stream_t stream) {
    if (((uintptr_t)qlen | (uintptr_t)klen) & 3) return MCP_ERR_BAD_ARG;
    if (!qlen && !klen)
        return backward_with(bf, nq, nk, heads, hd, q, q_stride, k, k_stride, v, v_stride, scale, drop_p, seed, out, grad_out, lse, grad_q, grad_kv,
                             workspace, workspace_bytes, stream);
    return backward_with(bf, nq, nk, heads, hd, q, q_stride, k, k_stride, v, v_stride, scale, drop_p, seed, out, grad_out, lse, grad_q, grad_kv, workspace,
                         workspace_bytes, stream, AttnLengths{qlen, klen});
}
