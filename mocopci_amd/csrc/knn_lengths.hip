// knn_lengths.hip -- the exhaustive K-nearest-neighbour search of knn.hip for padded batches of clouds of different sizes.
//
// Element bb of the batch searches only the first rlen[bb] rows of ref (B,N,3) and only its first qlen[bb] rows of query (B,Q,3)
// are live (pytorch3d's lengths2 / lengths1).  The kernels are those of knn.hip -- lane = one query, per-wave double-buffered LDS
// tiles of float4 (x,y,z,|r|^2), the register 4-list for K <= 4 and the threshold-filtered LDS queues for K <= 16 / 32, SPLIT waves
// of a workgroup scanning disjoint slices and merging their K-lists through LDS -- with four differences:
//   * both lengths are read on the device, one wave-uniform load each per workgroup (blockIdx.y indexes them), and clamped to
//     [0, N] / [0, Q]; the host never sees them, so a launch needs no synchronisation;
//   * the tile count, and with it every wave's slice, comes from rlen[bb]: tiles that lie wholly beyond it are neither loaded nor
//     visited, and the partial last tile is masked with +inf distances exactly as knn.hip masks the tail of N.  A wave whose slice
//     is empty (rlen[bb] < SPLIT tiles) carries an all-empty K-list into the merge, where every empty slot loses each minimum;
//   * a padded query lane loads row 0 of its element (live whenever the workgroup gets that far) instead of its own row, and
//     writes index 0 / distance 0; a workgroup whose 64 queries are all padding writes its zeros and returns before any load;
//   * rows that no length covers are therefore never read: their contents cannot reach any output bit.
//
// Result definition for live rows: the K smallest under (distance, index) among references 0 .. rlen[bb]-1, ascending, distances
// in the canon of common.h -- what mcp_knn returns for the two prefixes on their own; fewer than K references repeat the last
// valid entry, none give index 0 / distance 0.  knn.hip is untouched: its kernels keep their instruction stream.
#include "common.h"
#include "topk.h"

namespace {

typedef mcp_key u64;
#define KEY_INF MCP_KEY_INF
constexpr int TILE = 64;  // as in knn.hip

template <int MODE>
__device__ __forceinline__ float pair_dist(float qx, float qy, float qz, float qn, const float4 r) {
    if (MODE == MCP_DIST_EXPANSION) return mcp_expdist(qx, qy, qz, qn, r.x, r.y, r.z, r.w);
    return mcp_sqdist3(qx, qy, qz, r.x, r.y, r.z);
}

// i < nl: the point; otherwise a point at distance +inf in both forms (never passes "d < tau").  nl is the element's length.
template <int MODE>
__device__ __forceinline__ float4 load_ref(const float *__restrict__ ref, int i, int nl) {
    if (i < nl) {
        const float x = ref[(size_t)i * 3 + 0], y = ref[(size_t)i * 3 + 1], z = ref[(size_t)i * 3 + 2];
        return make_float4(x, y, z, mcp_sqnorm3(x, y, z));
    }
    return MODE == MCP_DIST_EXPANSION ? make_float4(0.f, 0.f, 0.f, INFINITY) : make_float4(INFINITY, 0.f, 0.f, 0.f);
}

__device__ __forceinline__ int clamped_len(const int *__restrict__ len, int b, int full) {
    if (!len) return full;
    const int v = len[b];  // b = blockIdx.y: one scalar load per workgroup
    return v < 0 ? 0 : (v > full ? full : v);
}

// mcp_store_list with an optional index output (the Chamfer entry point wants distances only)
template <int K>
__device__ __forceinline__ void store_list(const u64 (&a)[K], int kout, int *oi, float *od) {
    u64 last = a[0];
#pragma unroll
    for (int j = 0; j < K; ++j) {
        if (j < kout) {
            const u64 kk = mcp_key_is_inf(a[j]) ? last : a[j];
            last = kk;
            if (oi) oi[j] = mcp_key_is_inf(kk) ? 0 : (int)mcp_key_index(kk);
            if (od) od[j] = mcp_key_is_inf(kk) ? 0.f : mcp_key_dist(kk);
        }
    }
}
__device__ __forceinline__ void store_zeros(int kout, int *oi, float *od) {
    for (int j = 0; j < kout; ++j) {
        if (oi) oi[j] = 0;
        if (od) od[j] = 0.f;
    }
}

// ---------------------------------------------------------------------------------------------
// K <= 4: sorted 4-list in registers, insertion guarded by a wave-uniform branch.
// ---------------------------------------------------------------------------------------------
template <int MODE, int SPLIT>
__global__ __launch_bounds__(64 * SPLIT) void knn_len_small_kernel(int q, int n, int kout, const float *__restrict__ query,
                                                                   const float *__restrict__ ref, const int *__restrict__ qlen,
                                                                   const int *__restrict__ rlen, int *__restrict__ idx,
                                                                   float *__restrict__ dist) {
    __shared__ float4 tiles[SPLIT][2][TILE];
    __shared__ u64 mrg[SPLIT][4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.y;
    const int ql = clamped_len(qlen, b, q), nl = clamped_len(rlen, b, n);
    const int qi = blockIdx.x * 64 + lane;
    int *oi = idx ? idx + ((size_t)b * q + qi) * kout : nullptr;
    float *od = dist ? dist + ((size_t)b * q + qi) * kout : nullptr;
    if ((int)blockIdx.x * 64 >= ql) {  // workgroup-uniform: nothing but padding here
        if (wave == 0 && qi < q) store_zeros(kout, oi, od);
        return;
    }
    const bool live = qi < ql;
    const float *qp = query + ((size_t)b * q + (live ? qi : 0)) * 3;  // row 0 is live: ql > blockIdx.x * 64 >= 0
    const float qx = qp[0], qy = qp[1], qz = qp[2];
    const float qn = mcp_sqnorm3(qx, qy, qz);
    ref += (size_t)b * n * 3;

    // slice of the VALID reference rows for this wave, in whole tiles
    const int ntiles = (nl + TILE - 1) / TILE;
    const int t0 = (int)((long long)ntiles * wave / SPLIT), t1 = (int)((long long)ntiles * (wave + 1) / SPLIT);

    u64 a[4] = {KEY_INF, KEY_INF, KEY_INF, KEY_INF};
    float tau = INFINITY;
    float4(*tile)[TILE] = tiles[wave];

    if (t0 < t1) tile[0][lane] = load_ref<MODE>(ref, t0 * TILE + lane, nl);
    for (int t = t0; t < t1; ++t) {
        const int cur = (t - t0) & 1;
        float4 nxt;
        if (t + 1 < t1) nxt = load_ref<MODE>(ref, (t + 1) * TILE + lane, nl);
        __builtin_amdgcn_wave_barrier();
        const int base = t * TILE;
        constexpr int G = 8;  // references per group: loads of group g+1 are in flight under the math of group g
        float4 rc[G];
#pragma unroll
        for (int u = 0; u < G; ++u) rc[u] = tile[cur][u];
        for (int r0 = 0; r0 < TILE; r0 += G) {
            float4 rn[G];
            const int rnext = r0 + G < TILE ? r0 + G : r0;
#pragma unroll
            for (int u = 0; u < G; ++u) rn[u] = tile[cur][rnext + u];
            float d[G];
            bool any = false;
#pragma unroll
            for (int u = 0; u < G; ++u) {
                d[u] = pair_dist<MODE>(qx, qy, qz, qn, rc[u]);
                any |= d[u] < tau;
            }
            if (__builtin_amdgcn_ballot_w64(any)) {
#pragma unroll
                for (int u = 0; u < G; ++u) {
                    if (__builtin_amdgcn_ballot_w64(d[u] < tau)) {
                        u64 key = mcp_make_key(d[u], (uint32_t)(base + r0 + u));
                        key = d[u] < tau ? key : KEY_INF;
                        a[3] = mcp_key_min(key, a[3]);
                        mcp_ce_asc(a[2], a[3]);
                        mcp_ce_asc(a[1], a[2]);
                        mcp_ce_asc(a[0], a[1]);
                        tau = mcp_tau_of(a[3]);
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < G; ++u) rc[u] = rn[u];
        }
        if (t + 1 < t1) {
            __builtin_amdgcn_wave_barrier();
            tile[cur ^ 1][lane] = nxt;
        }
    }
    if (SPLIT > 1) {
#pragma unroll
        for (int j = 0; j < 4; ++j) mrg[wave][j][lane] = a[j];
        __syncthreads();
        if (wave != 0) return;
        for (int w = 1; w < SPLIT; ++w) {
            u64 o[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = mrg[w][j][lane];
            mcp_merge_sorted<4, 4>(a, o);
        }
    }
    if (qi >= q) return;
    if (live)
        store_list<4>(a, kout, oi, od);
    else
        store_zeros(kout, oi, od);
}

// ---------------------------------------------------------------------------------------------
// K in {16, 32}: threshold-filtered LDS queues + register bitonic merges.
// ---------------------------------------------------------------------------------------------
template <int K>
struct KnnLds {  // as in knn.hip
    static constexpr int QS = 16;
    static constexpr int TILE_BYTES = 2 * TILE * 16;
    static constexpr int QUEUE_BYTES = QS * 64 * 8;
    static constexpr int MERGE_BYTES = K * 64 * 8;
    static constexpr int SCAN_BYTES = TILE_BYTES + QUEUE_BYTES;
    static constexpr int WAVE_BYTES = SCAN_BYTES > MERGE_BYTES ? SCAN_BYTES : MERGE_BYTES;
};

template <int K, int MODE, int SPLIT>
__global__ __launch_bounds__(64 * SPLIT) void knn_len_queue_kernel(int q, int n, int kout, const float *__restrict__ query,
                                                                   const float *__restrict__ ref, const int *__restrict__ qlen,
                                                                   const int *__restrict__ rlen, int *__restrict__ idx,
                                                                   float *__restrict__ dist) {
    using L = KnnLds<K>;
    constexpr int QS = L::QS;
    constexpr int CHK = 4;  // refs between queue-full checks
    extern __shared__ float4 smem_f4[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    char *wbase = reinterpret_cast<char *>(smem_f4) + (size_t)wave * L::WAVE_BYTES;
    float4(*tile)[TILE] = reinterpret_cast<float4(*)[TILE]>(wbase);
    uint2(*queue)[64] = reinterpret_cast<uint2(*)[64]>(wbase + L::TILE_BYTES);

    const int b = blockIdx.y;
    const int ql = clamped_len(qlen, b, q), nl = clamped_len(rlen, b, n);
    const int qi = blockIdx.x * 64 + lane;
    int *oi = idx ? idx + ((size_t)b * q + qi) * kout : nullptr;
    float *od = dist ? dist + ((size_t)b * q + qi) * kout : nullptr;
    if ((int)blockIdx.x * 64 >= ql) {  // workgroup-uniform: nothing but padding here
        if (wave == 0 && qi < q) store_zeros(kout, oi, od);
        return;
    }
    const bool live = qi < ql;
    const float *qp = query + ((size_t)b * q + (live ? qi : 0)) * 3;  // row 0 is live: ql > blockIdx.x * 64 >= 0
    const float qx = qp[0], qy = qp[1], qz = qp[2];
    const float qn = mcp_sqnorm3(qx, qy, qz);
    ref += (size_t)b * n * 3;

    const int ntiles = (nl + TILE - 1) / TILE;
    const int t0 = (int)((long long)ntiles * wave / SPLIT), t1 = (int)((long long)ntiles * (wave + 1) / SPLIT);

    u64 a[K];
#pragma unroll
    for (int j = 0; j < K; ++j) a[j] = KEY_INF;
    float tau = INFINITY;
    int cnt = 0;

    auto flush = [&]() {
        mcp_flush_queue<K, QS>(a, queue, lane, cnt);
        tau = mcp_tau_of(a[K - 1]);
        cnt = 0;
    };

    if (t0 < t1) tile[0][lane] = load_ref<MODE>(ref, t0 * TILE + lane, nl);
    for (int t = t0; t < t1; ++t) {
        const int cur = (t - t0) & 1;
        float4 nxt;
        if (t + 1 < t1) nxt = load_ref<MODE>(ref, (t + 1) * TILE + lane, nl);
        __builtin_amdgcn_wave_barrier();
        const int base = t * TILE;
        // software pipeline over groups of CHK references, as in knn.hip
        float4 rc[CHK];
#pragma unroll
        for (int u = 0; u < CHK; ++u) rc[u] = tile[cur][u];
        for (int r0 = 0; r0 < TILE; r0 += CHK) {
            float4 rn[CHK];
            const int rnext = r0 + CHK < TILE ? r0 + CHK : r0;  // last group re-reads itself (harmless)
#pragma unroll
            for (int u = 0; u < CHK; ++u) rn[u] = tile[cur][rnext + u];
            float d[CHK];
#pragma unroll
            for (int u = 0; u < CHK; ++u) d[u] = pair_dist<MODE>(qx, qy, qz, qn, rc[u]);
#pragma unroll
            for (int u = 0; u < CHK; ++u) {
                if (d[u] < tau) {
                    queue[cnt][lane] = make_uint2(__float_as_uint(d[u]), (uint32_t)(base + r0 + u));
                    ++cnt;
                }
            }
            if (__builtin_amdgcn_ballot_w64(cnt > QS - CHK)) flush();
#pragma unroll
            for (int u = 0; u < CHK; ++u) rc[u] = rn[u];
        }
        if (t + 1 < t1) {
            __builtin_amdgcn_wave_barrier();
            tile[cur ^ 1][lane] = nxt;
        }
    }
    flush();  // cnt == 0 in a wave with an empty slice: its list stays all-empty

    if (SPLIT > 1) {
        __syncthreads();  // every wave is done with its tile/queue region before it is reused for keys
        u64(*mrg)[64] = reinterpret_cast<u64(*)[64]>(wbase);
#pragma unroll
        for (int j = 0; j < K; ++j) mrg[j][lane] = a[j];
        __syncthreads();
        if (wave != 0) return;
        for (int w = 1; w < SPLIT; ++w) {
            u64(*om)[64] = reinterpret_cast<u64(*)[64]>(reinterpret_cast<char *>(smem_f4) + (size_t)w * L::WAVE_BYTES);
            u64 o[K];
#pragma unroll
            for (int j = 0; j < K; ++j) o[j] = om[j][lane];
            mcp_merge_sorted<K, K>(a, o);
        }
    }
    if (qi >= q) return;
    if (live)
        store_list<K>(a, kout, oi, od);
    else
        store_zeros(kout, oi, od);
}

// The split rule of knn.hip's pick_split on the PADDED sizes: the host does not know the lengths (reading them would be a
// synchronisation).  A short element leaves some of its SPLIT waves without a tile; they idle through the merge.
int pick_split(int b, int q, int n) {
    const long long waves = (long long)b * ((q + 63) / 64);
    const int ntiles = (n + TILE - 1) / TILE;
    int split = 1;
    while (split < 8 && waves * split < 2048 && ntiles >= 2 * split) split *= 2;
    return split;
}

struct Args {
    int b, q, n, k;
    const float *query, *ref;
    const int *qlen, *rlen;
    int *idx;
    float *dist;
    hipStream_t s;
};

template <int MODE, int SPLIT>
int launch_small(const Args &a) {
    hipLaunchKernelGGL((knn_len_small_kernel<MODE, SPLIT>), dim3(mcp_divup(a.q, 64), a.b), dim3(64 * SPLIT), 0, a.s, a.q, a.n, a.k,
                       a.query, a.ref, a.qlen, a.rlen, a.idx, a.dist);
    return mcp_launch_status();
}
template <int K, int MODE, int SPLIT>
int launch_queue(const Args &a) {
    const size_t lds = (size_t)KnnLds<K>::WAVE_BYTES * SPLIT;
    auto kern = knn_len_queue_kernel<K, MODE, SPLIT>;
    static McpPerDeviceOnce attr_once;
    if (attr_once.need()) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return (int)e;
        attr_once.done();
    }
    hipLaunchKernelGGL(kern, dim3(mcp_divup(a.q, 64), a.b), dim3(64 * SPLIT), lds, a.s, a.q, a.n, a.k, a.query, a.ref, a.qlen, a.rlen,
                       a.idx, a.dist);
    return mcp_launch_status();
}
template <int MODE, int SPLIT>
int dispatch_k(const Args &a) {
    if (a.k <= 4) return launch_small<MODE, SPLIT>(a);
    if (a.k <= 16) return launch_queue<16, MODE, SPLIT>(a);
    return launch_queue<32, MODE, SPLIT>(a);
}
template <int MODE>
int dispatch_split(const Args &a) {
    const int split = pick_split(a.b, a.q, a.n);
    if (split == 1) return dispatch_k<MODE, 1>(a);
    if (split == 2) return dispatch_k<MODE, 2>(a);
    if (split == 4) return dispatch_k<MODE, 4>(a);
    return dispatch_k<MODE, 8>(a);
}
int search(int dist_form, const Args &a) {
    mcp_prof_begin(MCP_KERNEL_KNN, a.s);
    const int rc = dist_form == MCP_DIST_EXPANSION ? dispatch_split<MCP_DIST_EXPANSION>(a) : dispatch_split<MCP_DIST_DIRECT>(a);
    mcp_prof_end(MCP_KERNEL_KNN, a.s);
    return rc;
}

}  // namespace

MCP_EXPORT int mcp_knn_lengths(int b, int q, int n, int k, int dist_form, const float *query, const float *ref, const int *qlen,
                               const int *rlen, int *idx, float *dist, mcp_stream_t stream) {
    if (!qlen && !rlen) return mcp_knn(b, q, n, k, dist_form, query, ref, idx, dist, stream);  // the same launch, the same bits
    MCP_CHECK_ARGS(b > 0 && q > 0 && n > 0 && k > 0 && query && ref && idx);
    MCP_CHECK_ARGS(dist_form == MCP_DIST_EXPANSION || dist_form == MCP_DIST_DIRECT);
    if (k > 32) return MCP_ERR_UNSUPPORTED;
    return search(dist_form, Args{b, q, n, k, query, ref, qlen, rlen, idx, dist, (hipStream_t)stream});
}

MCP_EXPORT int mcp_chamfer_nn_lengths(int b, int n, int m, const float *x, const float *y, const int *xlen, const int *ylen, float *dxy,
                                      float *dyx, mcp_stream_t stream) {
    MCP_CHECK_ARGS(b > 0 && n > 0 && m > 0 && x && y && dxy && dyx);
    if (!xlen && !ylen) return mcp_chamfer_nn(b, n, m, x, y, dxy, dyx, stream);
    hipStream_t s = (hipStream_t)stream;
    const int rc = search(MCP_DIST_DIRECT, Args{b, n, m, 1, x, y, xlen, ylen, nullptr, dxy, s});
    if (rc) return rc;
    return search(MCP_DIST_DIRECT, Args{b, m, n, 1, y, x, ylen, xlen, nullptr, dyx, s});
}
