// attention_lengths.h -- per-element query / key lengths of a padded batch, the compile-time switch of the attention kernels.
// Every kernel (body) is stated once with a trailing parameter pack L that is either empty -- the plain kernel, with the parameter
// list and the code it always had -- or one AttnLengths.  qlen / klen are (BF) int32 device arrays, either may be null (that side is
// full); qlen is indexed by the query's batch element, klen by the batch element the keys / values come from.  The kernels clamp to
// [0, nq] / [0, nk]; the padded nq / nk keep giving the batch strides and the rows of the dropout hash.  A length is read through
// blockIdx only, so it is wave-uniform: a scalar load, scalar loop limits.
//
// What a length form writes: rows i < ql against keys j < kl as the plain kernel computes them on the prefixes; rows ql <= i < nq
// zeros (lse 0); every row zero when kl = 0.  Nothing at or beyond a length is loaded into a value that reaches an output: the
// stationary side's lanes past the length take row 0 of the element (live whenever the workgroup does not return early), the
// streamed side's loops and zero-filled loads end at the length.
#pragma once
#include "common.h"

namespace {

struct AttnLengths {
    const int *qlen, *klen;
};
struct AttnSpan {
    int ql, kl;
};
// one side's length: of batch element b, clamped to [0, n]; n without lengths
__device__ __forceinline__ int attn_len(const int *lens, int n, int b) { return lens ? min(max(lens[b], 0), n) : n; }
__device__ __forceinline__ int attn_qlen(int nq, int bq) { return nq; }
__device__ __forceinline__ int attn_qlen(int nq, int bq, const AttnLengths &len) { return attn_len(len.qlen, nq, bq); }
__device__ __forceinline__ int attn_klen(int nk, int bkv) { return nk; }
__device__ __forceinline__ int attn_klen(int nk, int bkv, const AttnLengths &len) { return attn_len(len.klen, nk, bkv); }
// both: queries of batch element bq, keys / values of batch element bkv
template <class... L>
__device__ __forceinline__ AttnSpan attn_span(int nq, int nk, int bq, int bkv, L... lens) {
    return AttnSpan{attn_qlen(nq, bq, lens...), attn_klen(nk, bkv, lens...)};
}

// W zeros at dst (16-byte aligned, W a multiple of 4)
template <int W>
__device__ __forceinline__ void attn_zero_row(float *dst) {
#pragma unroll
    for (int d = 0; d < W; d += 4) *reinterpret_cast<float4 *>(dst + d) = make_float4(0.f, 0.f, 0.f, 0.f);
}

}  // namespace
