// knn.hip -- fused brute-force K-nearest-neighbour search for gfx950.
//
// Replaces  square_distance + torch.topk  (mocopci.py:1130-1169 = pointconv_util.py:67-140)
// and pytorch3d.ops.knn_points (pointconv_util.py:910).  The reference materialises a
// (B,Q,N) fp32 distance matrix (24 B of HBM traffic per pair); this kernel never does:
//
//   * lane = one query (coordinates + |q|^2 in VGPRs), wave = 64 queries;
//   * reference points stream through a per-wave, double-buffered LDS tile of float4
//     (x,y,z,|r|^2); every lane reads the same float4 (LDS broadcast, conflict-free);
//   * selection: a per-lane threshold tau (the current K-th distance) filters candidates into
//     a per-lane LDS queue (column layout [slot][lane], conflict-free); when any lane's queue
//     is nearly full the wave sorts its queues with a register bitonic network and merges
//     them into the per-lane sorted K-list, tightening tau;
//   * small Q: SPLIT waves of a workgroup scan disjoint slices of the reference set for the
//     same 64 queries and merge their K-lists through LDS, so B*Q/64 < #SIMDs still fills
//     the chip.
//
// Result definition (same as oracle/pointset_oracle.c:orc_knn): the K smallest under the
// lexicographic order (distance, index), ascending; distances in the canon of common.h.
// Keys are the 64-bit (distance, index) keys of topk.h: a compare-exchange is one v_min_f64 / v_max_f64 pair.
//
// The device code is in knn_scan.h: two kernel bodies, each instantiated without lengths (mcp_knn: knn_small_kernel, knn_queue_kernel) and
// with per-cloud lengths (mcp_knn_lengths, mcp_chamfer_nn_lengths: knn_len_small_kernel, knn_len_queue_kernel).
#include "knn_scan.h"

namespace {

template <int MODE, int SPLIT>
__global__ __launch_bounds__(64 * SPLIT) void knn_small_kernel(int q, int n, int kout, const float *__restrict__ query,
                                                               const float *__restrict__ ref, int *__restrict__ idx,
                                                               float *__restrict__ dist) {
    __shared__ float4 tiles[SPLIT][2][TILE];
    __shared__ u64 mrg[SPLIT][4][64];
    knn_small_body<MODE, SPLIT, false>(tiles, mrg, q, n, kout, query, ref, nullptr, nullptr, idx, dist);
}
template <int MODE, int SPLIT>
__global__ __launch_bounds__(64 * SPLIT) void knn_len_small_kernel(int q, int n, int kout, const float *__restrict__ query,
                                                                   const float *__restrict__ ref, const int *__restrict__ qlen,
                                                                   const int *__restrict__ rlen, int *__restrict__ idx,
                                                                   float *__restrict__ dist) {
    __shared__ float4 tiles[SPLIT][2][TILE];
    __shared__ u64 mrg[SPLIT][4][64];
    knn_small_body<MODE, SPLIT, true>(tiles, mrg, q, n, kout, query, ref, qlen, rlen, idx, dist);
}

template <int K, int MODE, int SPLIT>
__global__ __launch_bounds__(64 * SPLIT) void knn_queue_kernel(int q, int n, int kout, const float *__restrict__ query,
                                                               const float *__restrict__ ref, int *__restrict__ idx,
                                                               float *__restrict__ dist) {
    extern __shared__ float4 smem_f4[];
    knn_queue_body<K, MODE, SPLIT, false>(smem_f4, q, n, kout, query, ref, nullptr, nullptr, idx, dist);
}
template <int K, int MODE, int SPLIT>
__global__ __launch_bounds__(64 * SPLIT) void knn_len_queue_kernel(int q, int n, int kout, const float *__restrict__ query,
                                                                   const float *__restrict__ ref, const int *__restrict__ qlen,
                                                                   const int *__restrict__ rlen, int *__restrict__ idx,
                                                                   float *__restrict__ dist) {
    extern __shared__ float4 smem_f4[];
    knn_queue_body<K, MODE, SPLIT, true>(smem_f4, q, n, kout, query, ref, qlen, rlen, idx, dist);
}

// Chamfer helper: nearest squared distance from every x to the set y (direct form).
__global__ __launch_bounds__(256) void nn1_kernel(int n, int m, const float *__restrict__ x, const float *__restrict__ y,
                                                  float *__restrict__ out) {
    __shared__ float tile[1024 * 3];
    const int b = blockIdx.y;
    const int p = blockIdx.x * 256 + threadIdx.x;
    const bool live = p < n;
    const float *u = x + ((size_t)b * n + (live ? p : 0)) * 3;
    const float ux = u[0], uy = u[1], uz = u[2];
    const float *yb = y + (size_t)b * m * 3;
    float best = INFINITY;
    for (int base = 0; base < m; base += 1024) {
        const int len = min(1024, m - base);
        __syncthreads();
        for (int i = threadIdx.x; i < len * 3; i += 256) tile[i] = yb[(size_t)base * 3 + i];
        __syncthreads();
        for (int k = 0; k < len; ++k) best = fminf(best, mcp_sqdist3(ux, uy, uz, tile[k * 3], tile[k * 3 + 1], tile[k * 3 + 2]));
    }
    if (live) out[(size_t)b * n + p] = best;
}

// The split comes from the PADDED sizes: the host does not know the lengths (reading them would be a synchronisation).  A short
// element leaves some of its SPLIT waves without a tile; they idle through the merge.
int pick_split(int b, int q, int n) {
    // aim for >= 2 waves per SIMD (1024 SIMDs) while keeping at least two 64-reference tiles per wave.  (The rule used to keep
    // two tiles per wave: the N = 512 / 1024 searches of the lower pyramid levels then ran 384-768 waves of 512 sequential
    // references each on 1024 SIMDs, ~40 us launches on the critical path; splitting them took 0.3 ms off the step.)
    const long long waves = (long long)b * ((q + 63) / 64);
    const int ntiles = (n + TILE - 1) / TILE;
    int split = 1;
    while (split < 8 && waves * split < 2048 && ntiles >= 2 * split) split *= 2;
    return split;
}

struct Args {
    int b, q, n, k;
    const float *query, *ref;
    const int *qlen, *rlen;  // LEN only
    int *idx;
    float *dist;
    hipStream_t s;
};

// one launch of either family: the plain kernels take no lengths
template <bool LEN, typename Plain, typename Len>
int launch(Plain plain, Len len, int split, size_t lds, const Args &a) {
    const dim3 grid(mcp_divup(a.q, 64), a.b), block(64 * split);
    if constexpr (LEN) hipLaunchKernelGGL(len, grid, block, lds, a.s, a.q, a.n, a.k, a.query, a.ref, a.qlen, a.rlen, a.idx, a.dist);
    else hipLaunchKernelGGL(plain, grid, block, lds, a.s, a.q, a.n, a.k, a.query, a.ref, a.idx, a.dist);
    return mcp_launch_status();
}
template <int MODE, int SPLIT, bool LEN>
int launch_small(const Args &a) {
    return launch<LEN>(knn_small_kernel<MODE, SPLIT>, knn_len_small_kernel<MODE, SPLIT>, SPLIT, 0, a);
}
template <int K, int MODE, int SPLIT, bool LEN>
int launch_queue(const Args &a) {
    constexpr auto plain = knn_queue_kernel<K, MODE, SPLIT>;
    constexpr auto len = knn_len_queue_kernel<K, MODE, SPLIT>;
    if constexpr (LEN) {
        if (const int rc = mcp_allow_lds<len>()) return rc;
    } else {
        if (const int rc = mcp_allow_lds<plain>()) return rc;
    }
    return launch<LEN>(plain, len, SPLIT, (size_t)KnnLds<K>::WAVE_BYTES * SPLIT, a);
}
template <int MODE, int SPLIT, bool LEN>
int dispatch_k(const Args &a) {
    if (a.k <= 4) return launch_small<MODE, SPLIT, LEN>(a);
    if (a.k <= 16) return launch_queue<16, MODE, SPLIT, LEN>(a);
    return launch_queue<32, MODE, SPLIT, LEN>(a);
}
template <int MODE, bool LEN>
int dispatch_split(const Args &a) {
    const int split = pick_split(a.b, a.q, a.n);
    if (split == 1) return dispatch_k<MODE, 1, LEN>(a);
    if (split == 2) return dispatch_k<MODE, 2, LEN>(a);
    if (split == 4) return dispatch_k<MODE, 4, LEN>(a);
    return dispatch_k<MODE, 8, LEN>(a);
}
template <bool LEN>
int search(int dist_form, const Args &a) {
    mcp_prof_begin(MCP_KERNEL_KNN, a.s);
    const int rc = dist_form == MCP_DIST_EXPANSION ? dispatch_split<MCP_DIST_EXPANSION, LEN>(a) : dispatch_split<MCP_DIST_DIRECT, LEN>(a);
    mcp_prof_end(MCP_KERNEL_KNN, a.s);
    return rc;
}

}  // namespace

MCP_EXPORT int mcp_knn(int b, int q, int n, int k, int dist_form, const float *query, const float *ref, int *idx, float *dist,
                       mcp_stream_t stream) {
    MCP_CHECK_ARGS(b > 0 && q > 0 && n > 0 && k > 0 && query && ref && idx);
    MCP_CHECK_ARGS(dist_form == MCP_DIST_EXPANSION || dist_form == MCP_DIST_DIRECT);
    if (k > 32) return MCP_ERR_UNSUPPORTED;
    return search<false>(dist_form, Args{b, q, n, k, query, ref, nullptr, nullptr, idx, dist, (hipStream_t)stream});
}

MCP_EXPORT int mcp_knn_lengths(int b, int q, int n, int k, int dist_form, const float *query, const float *ref, const int *qlen,
                               const int *rlen, int *idx, float *dist, mcp_stream_t stream) {
    if (!qlen && !rlen) return mcp_knn(b, q, n, k, dist_form, query, ref, idx, dist, stream);  // the same launch, the same bits
    MCP_CHECK_ARGS(b > 0 && q > 0 && n > 0 && k > 0 && query && ref && idx);
    MCP_CHECK_ARGS(dist_form == MCP_DIST_EXPANSION || dist_form == MCP_DIST_DIRECT);
    if (k > 32) return MCP_ERR_UNSUPPORTED;
    return search<true>(dist_form, Args{b, q, n, k, query, ref, qlen, rlen, idx, dist, (hipStream_t)stream});
}

MCP_EXPORT int mcp_chamfer_nn(int b, int n, int m, const float *x, const float *y, float *dxy, float *dyx, mcp_stream_t stream) {
    MCP_CHECK_ARGS(b > 0 && n > 0 && m > 0 && x && y && dxy && dyx);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(nn1_kernel, dim3(mcp_divup(n, 256), b), dim3(256), 0, s, n, m, x, y, dxy);
    hipLaunchKernelGGL(nn1_kernel, dim3(mcp_divup(m, 256), b), dim3(256), 0, s, m, n, y, x, dyx);
    return mcp_launch_status();
}

MCP_EXPORT int mcp_chamfer_nn_lengths(int b, int n, int m, const float *x, const float *y, const int *xlen, const int *ylen, float *dxy,
                                      float *dyx, mcp_stream_t stream) {
    MCP_CHECK_ARGS(b > 0 && n > 0 && m > 0 && x && y && dxy && dyx);
    if (!xlen && !ylen) return mcp_chamfer_nn(b, n, m, x, y, dxy, dyx, stream);
    hipStream_t s = (hipStream_t)stream;
    const int rc = search<true>(MCP_DIST_DIRECT, Args{b, n, m, 1, x, y, xlen, ylen, nullptr, dxy, s});
    if (rc) return rc;
    return search<true>(MCP_DIST_DIRECT, Args{b, m, n, 1, y, x, ylen, xlen, nullptr, dyx, s});
}
