// cross256_grad.hip -- backward of the D = 256 cost volume (cross3, pointconv_util.py:783-791; forward: cross256_stream_kernel in
// cross.hip) for gfx950.  Per point and neighbour j = 0..31
//     u_j = points2[idx_j] + points1 + Wpos (xyz2[idx_j] - xyz1) + bpos,  x_j = LeakyReLU(u_j),  z_j = Wmlp x_j + bmlp,
//     out = max_j LeakyReLU(z_j).
// The D = 64 / 128 kernel (cross_grad.hip) keeps Wmlp, Wmlp^T and the dWmlp accumulators on chip; at 256 the two images are 393 KB
// each and dWmlp is 1024 registers per wave.  What makes 256 cheap instead is that dz is SPARSE: for every (point, channel c) it is
// non-zero at exactly one neighbour j*(c), so with gz[c] = dL/dout[c] LeakyReLU'(z_{j*(c)}[c])
//     dx_j[k]     = sum over {c : j*(c) = j} of gz[c] Wmlp[c][k]          (65 536 multiply-adds per point, not 32 x 65 536)
//     dWmlp[c][:] += gz[c] x_{j*(c)}[:]                                    (likewise)
// are plain fp32 sums: only the recompute of z needs the matrix pipe, and Wmlp^T is never needed as an MFMA image.  Three passes:
//   Z  (cross256_grad_z_kernel): the forward again, bit for bit -- same image (mcp_cross_pack), same streamed 48 KB weight tiles, same
//      MFMA order --, but instead of reducing z to its maximum it finds the arg-max neighbour of every channel (all-reduce max over the
//      32 lanes of a lane half on order-preserving keys; lowest list position among equal maxima) and writes j* and gz (B,N1,256) to
//      the workspace.  x (B,N1,32,256) is parked in the caller's grad_rows buffer, which has exactly that shape and is not yet in use.
//   DX (cross256_grad_dx_kernel, vector only): one workgroup per point at a time, thread = input channel k.  The 256 channels are
//      counting-sorted by j* in LDS, so dx_j is formed neighbour by neighbour in ascending channel order with eight Wmlp rows in
//      flight; du_j = LeakyReLU'(u_j) dx_j overwrites x_j in grad_rows; dL/dpoints1, grad_dir = Wpos^T du_j, dL/dxyz1, and the
//      workgroup's share of dWpos, dbpos, dbmlp follow.
//   W  (cross256_grad_w_kernel, vector only; reads x, so it runs BEFORE DX): workgroup = (64 columns of dWmlp, a slice of the points),
//      thread = row c with 64 accumulators; a point's 32 x 64 block of x goes through LDS, thread c reads row j*(c) of it.
// A last kernel adds the workgroups' partial vectors in workgroup order: every sum has a fixed order, the gradients repeat bit for bit.
#include "common.h"
#include "cross_tile.h"  // KNB, SLOPE, CrossLds<256> and the X256_* constants, cross_nbr, cross_layer1, cross_winner, the entry checks

namespace {

constexpr int D = 256, T = X256_T, WAVES = X256_WAVES, TILE_U4 = X256_TILE_U4, SMALL = X256_SMALL;
using L = CrossLds<D>;  // the image mcp_cross_pack writes
constexpr size_t Z_LDS_BYTES = (size_t)X256_LDS_FLOATS * sizeof(float);
// weight-gradient vector (floats): dWpos (D,3) | dbpos (D) | dWmlp (D,D) | dbmlp (D)
constexpr int G_WM = 4 * D, G_BM = 4 * D + D * D, G_FLOATS = G_BM + D;
// a DX workgroup's partial vector: dWpos | dbpos (the first 4 D floats of the gradient vector as they are) | dbmlp
constexpr int P_WP = 0, P_BP = 3 * D, P_BM = 4 * D, P_FLOATS = 5 * D;
constexpr int DX_GRID = 512, W_SLICES = 64, W_COLS = 64, W_PTS = 4, W_STRIDE = W_COLS + 4, DU_STRIDE = D + 8;

// ---- pass Z: x, z as the forward computes them; j*(c), gz[c] per (point, channel); x parked in x_rows (B,N1,32,256) ----
__global__ __launch_bounds__(64 * WAVES, 1) void cross256_grad_z_kernel(long long total, int n1, int n2, const float *__restrict__ xyz1,
                                                                       const float *__restrict__ xyz2, const float *__restrict__ points1,
                                                                       const float *__restrict__ points2, const int *__restrict__ idx,
                                                                       const int *__restrict__ idx2, const float *__restrict__ packed,
                                                                       const float *__restrict__ gout, float *__restrict__ x_rows,
                                                                       int *__restrict__ jstar, float *__restrict__ gz) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    uint4 *wbuf = reinterpret_cast<uint4 *>(lds);  // [2][TILE_U4]
    float *small = lds + 2 * TILE_U4 * 4;          // pos | bias
    float *row1_all = small + SMALL;               // [WAVES][D]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, col = lane & 31;
    const uint4 *wimg = reinterpret_cast<const uint4 *>(packed);
    for (int e = tid; e < SMALL / 4; e += 64 * WAVES) reinterpret_cast<float4 *>(small)[e] = reinterpret_cast<const float4 *>(packed + L::OFF_POS)[e];
    for (int e = tid; e < TILE_U4; e += 64 * WAVES) wbuf[e] = wimg[e];  // tile 0
    __syncthreads();
    const float *lpos = small, *lbias = small + L::POS_FLOATS;
    float *row1_lds = row1_all + wave * D;
    const uint32_t lower_lanes = (1u << col) - 1u;

    const long long per_round = (long long)gridDim.x * WAVES;
    const long long first = (long long)blockIdx.x * WAVES;
    const int rounds = first < total ? (int)((total - first + per_round - 1) / per_round) : 0;  // the same for the four waves of the workgroup
    int cur = 0;
    for (int g = 0; g < rounds; ++g) {
        const long long pw = first + (long long)g * per_round + wave;
        const bool live = pw < total;
        const long long p = live ? pw : total - 1;  // a wave without a point works on the last one and does not store
        const int bb = (int)(p / n1);
        const int id = cross_nbr(idx, idx2, p, col);
        const float *q2 = xyz2 + ((long long)bb * n2 + id) * 3;
        const float dx = q2[0] - xyz1[p * 3 + 0], dy = q2[1] - xyz1[p * 3 + 1], dz = q2[2] - xyz1[p * 3 + 2];
        const float in0 = h ? dy : dx, in1 = h ? 1.0f : dz;  // k-step 0: (dx,dy); k-step 1: (dz,1)
        const float4 *row2 = reinterpret_cast<const float4 *>(points2 + ((long long)bb * n2 + id) * D);
        const float4 *row1 = reinterpret_cast<const float4 *>(points1 + p * D);
        float4 *xrow = reinterpret_cast<float4 *>(x_rows + (p * KNB + col) * D);
        reinterpret_cast<float4 *>(row1_lds)[lane] = row1[lane];  // D / 4 = 64 float4: one per lane
        __builtin_amdgcn_wave_barrier();
        McpSplit3 xs[2 * T];
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const f32x16 acc = cross_layer1(
                lpos, t, lane, in0, in1, [&](int gq) { return reinterpret_cast<const float4 *>(row1_lds)[cross_at(t, gq, h)]; },
                [&](int gq) { return row2[cross_at(t, gq, h)]; },
                [&](int gq, const f32x16 &x) {
                    if (live) xrow[cross_at(t, gq, h)] = make_float4(x[4 * gq + 0], x[4 * gq + 1], x[4 * gq + 2], x[4 * gq + 3]);
                });
            xs[2 * t + 0] = mcp_split_kstep(acc, 0);
            xs[2 * t + 1] = mcp_split_kstep(acc, 1);
        }
        __builtin_amdgcn_wave_barrier();  // the points1 row has been read: the next round may overwrite it
        const float4 *grow = reinterpret_cast<const float4 *>(gout + p * D);
#pragma unroll 1
        for (int t = 0; t < T; ++t) {
            // the next tile's pieces (the first tile again after the last: the next round starts with it) on their way while this one runs
            const bool more = t + 1 < T || g + 1 < rounds;
            const uint4 *nsrc = wimg + (size_t)((t + 1) & (T - 1)) * TILE_U4 + tid;
            uint4 nx[TILE_U4 / (64 * WAVES)];
#pragma unroll
            for (int i = 0; i < TILE_U4 / (64 * WAVES); ++i) nx[i] = more ? nsrc[i * 64 * WAVES] : make_uint4(0u, 0u, 0u, 0u);
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = lbias[(t * 2 + h) * 16 + r];
            acc = mcp_tile_split<2 * T>(wbuf + (size_t)cur * TILE_U4 + lane, xs, acc);
            // gz[c] = g[c] LeakyReLU'(z_j[c]) at the arg-max neighbour (lowest list position among equals); exactly one lane of a half wins
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                const float4 gv = grow[cross_at(t, gq, h)];
                const float gi[4] = {gv.x, gv.y, gv.z, gv.w};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float zv = acc[4 * gq + i];
                    const bool wins = cross_winner(zv, h, lower_lanes);
                    if (live && wins) {
                        const long long at = p * D + 32 * t + mcp_chan_of(4 * gq + i, h);
                        jstar[at] = col;
                        gz[at] = zv > 0.f ? gi[i] : SLOPE * gi[i];
                    }
                }
            }
            uint4 *ndst = wbuf + (size_t)(cur ^ 1) * TILE_U4 + tid;
#pragma unroll
            for (int i = 0; i < TILE_U4 / (64 * WAVES); ++i) ndst[i * 64 * WAVES] = nx[i];
            __syncthreads();
            cur ^= 1;
        }
    }
}

// ---- pass W: dWmlp[c][cb*64 .. +63] over a slice of the points; thread = row c ----
// a stage = W_PTS points: their (32 x 64) blocks of x (two float4 per thread and point), j* and gz of this thread's row
struct W256Stage {
    float x[W_PTS][8];
    int j[W_PTS];
    float g[W_PTS];
};
__device__ __forceinline__ void w256_fetch(W256Stage &o, long long ps, long long p1, int c, int cb, const float *__restrict__ x_rows,
                                           const int *__restrict__ jstar, const float *__restrict__ gz) {
#pragma unroll
    for (int q = 0; q < W_PTS; ++q) {
        const bool in = ps + q < p1;
        const long long p = in ? ps + q : p1 - 1;  // past the slice: a valid point with a zero weight
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int e = c + 256 * i, j = e >> 4, f = e & 15;
            const float4 v = reinterpret_cast<const float4 *>(x_rows + (p * KNB + j) * D + cb * W_COLS)[f];
            o.x[q][4 * i + 0] = v.x; o.x[q][4 * i + 1] = v.y; o.x[q][4 * i + 2] = v.z; o.x[q][4 * i + 3] = v.w;
        }
        o.j[q] = jstar[p * D + c] & (KNB - 1);
        o.g[q] = in ? gz[p * D + c] : 0.f;
    }
}
__global__ __launch_bounds__(256) void cross256_grad_w_kernel(long long total, int slices, const float *__restrict__ x_rows, const int *__restrict__ jstar,
                                                              const float *__restrict__ gz, float *__restrict__ partial) {
    __shared__ __attribute__((aligned(16))) float xs[W_PTS * KNB * W_STRIDE];
    const int c = threadIdx.x, cb = blockIdx.x & 3, slice = blockIdx.x >> 2;
    const long long per = (total + slices - 1) / slices, p0 = (long long)slice * per, p1 = p0 + per < total ? p0 + per : total;
    float acc[W_COLS];
#pragma unroll
    for (int i = 0; i < W_COLS; ++i) acc[i] = 0.f;
    W256Stage nxt;
    w256_fetch(nxt, p0, p1, c, cb, x_rows, jstar, gz);  // an empty slice reads the last point with zero weights and never uses it
    for (long long ps = p0; ps < p1; ps += W_PTS) {
        int js[W_PTS];
        float g[W_PTS];
#pragma unroll
        for (int q = 0; q < W_PTS; ++q) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int e = c + 256 * i, j = e >> 4, f = e & 15;
                reinterpret_cast<float4 *>(xs + (q * KNB + j) * W_STRIDE)[f] = make_float4(nxt.x[q][4 * i + 0], nxt.x[q][4 * i + 1], nxt.x[q][4 * i + 2], nxt.x[q][4 * i + 3]);
            }
            js[q] = nxt.j[q];
            g[q] = nxt.g[q];
        }
        __syncthreads();
        w256_fetch(nxt, ps + W_PTS, p1, c, cb, x_rows, jstar, gz);  // past the slice's end: zero weights, not used
#pragma unroll
        for (int q = 0; q < W_PTS; ++q) {
            const float4 *row = reinterpret_cast<const float4 *>(xs + (q * KNB + js[q]) * W_STRIDE);
#pragma unroll
            for (int f = 0; f < W_COLS / 4; ++f) {
                const float4 v = row[f];
                acc[4 * f + 0] = __builtin_fmaf(g[q], v.x, acc[4 * f + 0]);
                acc[4 * f + 1] = __builtin_fmaf(g[q], v.y, acc[4 * f + 1]);
                acc[4 * f + 2] = __builtin_fmaf(g[q], v.z, acc[4 * f + 2]);
                acc[4 * f + 3] = __builtin_fmaf(g[q], v.w, acc[4 * f + 3]);
            }
        }
        __syncthreads();  // the stage has been read: the next one may be written over it
    }
    float4 *o = reinterpret_cast<float4 *>(partial + ((size_t)slice * D + c) * D + cb * W_COLS);
#pragma unroll
    for (int f = 0; f < W_COLS / 4; ++f) o[f] = make_float4(acc[4 * f + 0], acc[4 * f + 1], acc[4 * f + 2], acc[4 * f + 3]);
}

// ---- pass DX: dx, du and everything that hangs on du; thread = input channel k; rows holds x on entry and du on exit ----
__global__ __launch_bounds__(256) void cross256_grad_dx_kernel(long long total, int n1, int n2, const float *__restrict__ xyz1,
                                                               const float *__restrict__ xyz2, const int *__restrict__ idx, const int *__restrict__ idx2,
                                                               const float *__restrict__ wpos, const float *__restrict__ wmlp,
                                                               const int *__restrict__ jstar, const float *__restrict__ gz, float *__restrict__ rows,
                                                               float *__restrict__ d_xyz1, float *__restrict__ d_dir, float *__restrict__ d_points1,
                                                               float *__restrict__ partial) {
    __shared__ float tile[KNB * DU_STRIDE];          // [j][k]: x_j[k], then du_j[k]
    __shared__ float wp_s[D * 3], gz_s[D], dir_s[KNB * 4], dd_s[KNB * 4];
    __shared__ unsigned long long mask_s[KNB * 4];   // [j][wave]: the channels 64 wave .. + 63 whose arg-max neighbour is j
    __shared__ int start_s[KNB + 1], order_s[D];     // channels sorted by (j*, channel)
    const int k = threadIdx.x, lane = k & 63, wave = k >> 6;
    for (int e = k; e < D * 3; e += 256) wp_s[e] = wpos[e];
    float dWp[3] = {0.f, 0.f, 0.f}, dbp = 0.f, dbm = 0.f;
    for (long long p = blockIdx.x; p < total; p += gridDim.x) {
        const int js = jstar[p * D + k] & (KNB - 1);
        const float gk = gz[p * D + k];
        float *prow = rows + p * KNB * D + k;
#pragma unroll
        for (int j = 0; j < KNB; ++j) tile[j * DU_STRIDE + k] = prow[j * D];
        gz_s[k] = gk;
        dbm += gk;
        if (k < KNB) {
            const int bb = (int)(p / n1);
            const int id = cross_nbr(idx, idx2, p, k);
            const float *q2 = xyz2 + ((long long)bb * n2 + id) * 3;
            dir_s[k * 4 + 0] = q2[0] - xyz1[p * 3 + 0];
            dir_s[k * 4 + 1] = q2[1] - xyz1[p * 3 + 1];
            dir_s[k * 4 + 2] = q2[2] - xyz1[p * 3 + 2];
        }
        unsigned long long my_mask = 0ull;
#pragma unroll
        for (int j = 0; j < KNB; ++j) {
            const unsigned long long m = __builtin_amdgcn_ballot_w64(js == j);
            if (lane == 0) mask_s[j * 4 + wave] = m;
            if (js == j) my_mask = m;
        }
        __syncthreads();
        if (k < 64) {  // wave 0: bucket sizes and their exclusive prefix
            int cnt = 0;
            if (k < KNB) cnt = __popcll(mask_s[k * 4 + 0]) + __popcll(mask_s[k * 4 + 1]) + __popcll(mask_s[k * 4 + 2]) + __popcll(mask_s[k * 4 + 3]);
            int inc = cnt;
#pragma unroll
            for (int o = 1; o < KNB; o <<= 1) {
                const int up = __shfl_up(inc, o);
                if (k >= o) inc += up;
            }
            if (k < KNB) start_s[k] = inc - cnt;
            if (k == KNB - 1) start_s[KNB] = inc;
        }
        __syncthreads();
        {
            int at = start_s[js] + __popcll(my_mask & ((1ull << lane) - 1ull));
            for (int w = 0; w < wave; ++w) at += __popcll(mask_s[js * 4 + w]);
            order_s[at] = k;
        }
        __syncthreads();
        // the 256 channels in (j*, channel) order, eight Wmlp rows in flight; a neighbour is finished where its bucket ends
        float acc = 0.f, dp1 = 0.f;
        int j = 0;
        auto finish = [&]() {
            const float xv = tile[j * DU_STRIDE + k];
            const float du = xv > 0.f ? acc : SLOPE * acc;  // x = LeakyReLU(u) has u's sign
            tile[j * DU_STRIDE + k] = du;
            prow[j * D] = du;
            dp1 += du;
            dWp[0] = __builtin_fmaf(du, dir_s[j * 4 + 0], dWp[0]);
            dWp[1] = __builtin_fmaf(du, dir_s[j * 4 + 1], dWp[1]);
            dWp[2] = __builtin_fmaf(du, dir_s[j * 4 + 2], dWp[2]);
            acc = 0.f;
            ++j;
        };
        while (j < KNB && __builtin_amdgcn_readfirstlane(start_s[j + 1]) == 0) finish();  // leading empty buckets
#pragma unroll 1
        for (int q0 = 0; q0 < D; q0 += 8) {
            float w[8], g[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int c = __builtin_amdgcn_readfirstlane(order_s[q0 + i]);
                w[i] = wmlp[c * D + k];
                g[i] = gz_s[c];
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                acc = __builtin_fmaf(g[i], w[i], acc);
                while (j < KNB && __builtin_amdgcn_readfirstlane(start_s[j + 1]) == q0 + i + 1) finish();
            }
        }
        d_points1[p * D + k] = dp1;
        dbp += dp1;
        __syncthreads();
        {   // grad_dir_j = Wpos^T du_j: eight threads per neighbour, 32 channels each, then a butterfly over the eight
            const int jj = k >> 3, part = k & 7;
            float sx = 0.f, sy = 0.f, sz = 0.f;
#pragma unroll 8
            for (int i = 0; i < D / 8; ++i) {
                const int ch = part + 8 * i;
                const float du = tile[jj * DU_STRIDE + ch];
                sx = __builtin_fmaf(wp_s[ch * 3 + 0], du, sx);
                sy = __builtin_fmaf(wp_s[ch * 3 + 1], du, sy);
                sz = __builtin_fmaf(wp_s[ch * 3 + 2], du, sz);
            }
#pragma unroll
            for (int o = 1; o < 8; o <<= 1) {
                sx += __shfl_xor(sx, o);
                sy += __shfl_xor(sy, o);
                sz += __shfl_xor(sz, o);
            }
            if (part == 0) {
                float *o = d_dir + (p * KNB + jj) * 3;
                o[0] = sx; o[1] = sy; o[2] = sz;
                dd_s[jj * 4 + 0] = sx; dd_s[jj * 4 + 1] = sy; dd_s[jj * 4 + 2] = sz;
            }
        }
        __syncthreads();
        if (k < 3) {
            float s = 0.f;
            for (int jj = 0; jj < KNB; ++jj) s += dd_s[jj * 4 + k];
            d_xyz1[p * 3 + k] = -s;
        }
    }
    float *o = partial + (size_t)blockIdx.x * P_FLOATS;
    o[P_WP + k * 3 + 0] = dWp[0];
    o[P_WP + k * 3 + 1] = dWp[1];
    o[P_WP + k * 3 + 2] = dWp[2];
    o[P_BP + k] = dbp;
    o[P_BM + k] = dbm;
}

// grad_weights[e] = sum over the workgroups' partial vectors, in workgroup order
__global__ __launch_bounds__(256) void cross256_grad_reduce_kernel(const float *__restrict__ part_dx, int n_dx, const float *__restrict__ part_w, int n_w,
                                                                   float *__restrict__ out) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= G_FLOATS) return;
    const bool is_w = e >= G_WM && e < G_BM;
    const float *src = is_w ? part_w + (e - G_WM) : part_dx + (e < G_WM ? e : P_BM + (e - G_BM));
    const size_t step = is_w ? (size_t)D * D : (size_t)P_FLOATS;
    const int n = is_w ? n_w : n_dx;
    float s = 0.f;
#pragma unroll 8
    for (int g = 0; g < n; ++g) s += src[(size_t)g * step];
    out[e] = s;
}

struct Plan {
    unsigned grid_z, grid_dx, slices;
    size_t off_j, off_gz, off_pdx, off_pw, bytes;
};
Plan plan(long long total) {
    Plan pl;
    const long long want = (total + WAVES - 1) / WAVES;
    pl.grid_z = (unsigned)(want < 256 ? want : 256);  // one resident workgroup per CU
    pl.grid_dx = (unsigned)(total < DX_GRID ? total : DX_GRID);
    const long long sl = (total + 2 * W_PTS - 1) / (2 * W_PTS);
    pl.slices = (unsigned)(sl < W_SLICES ? sl : W_SLICES);
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    pl.off_j = up((size_t)L::FLOATS * 4);  // the packed image comes first
    pl.off_gz = pl.off_j + up((size_t)total * D * 4);
    pl.off_pdx = pl.off_gz + up((size_t)total * D * 4);
    pl.off_pw = pl.off_pdx + up((size_t)pl.grid_dx * P_FLOATS * 4);
    pl.bytes = pl.off_pw + up((size_t)pl.slices * D * D * 4);
    return pl;
}

}  // namespace

MCP_EXPORT int mcp_cross256_grad_floats(void) { return G_FLOATS; }

MCP_EXPORT size_t mcp_cross256_grad_workspace_bytes(int b, int n1) {
    if (b <= 0 || n1 <= 0) return 0;
    return plan((long long)b * n1).bytes;
}

MCP_EXPORT int mcp_cross256_grad(int b, int n1, int n2, int k, const float *xyz1, const float *xyz2, const float *points1, const float *points2,
                                 const int *idx, const int *idx2, const float *wpos, const float *bpos, const float *wmlp, const float *bmlp,
                                 const float *grad_out, float *grad_xyz1, float *grad_dir, float *grad_points1, float *grad_rows, float *grad_weights,
                                 void *workspace, size_t workspace_bytes, mcp_stream_t stream) {
    if (const int rc = cross_grad_check(b, n1, n2, true, k, xyz1, xyz2, points1, points2, idx, wpos, bpos, wmlp, bmlp, grad_out, grad_xyz1, grad_dir,
                                        grad_points1, grad_rows, grad_weights, workspace))
        return rc;
    const long long total = (long long)b * n1;
    const Plan pl = plan(total);
    if (workspace_bytes < pl.bytes) return MCP_ERR_BAD_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (const int rc = mcp_allow_lds<cross256_grad_z_kernel>()) return rc;
    char *ws = static_cast<char *>(workspace);
    float *packed = reinterpret_cast<float *>(ws);
    int *jstar = reinterpret_cast<int *>(ws + pl.off_j);
    float *gz = reinterpret_cast<float *>(ws + pl.off_gz), *part_dx = reinterpret_cast<float *>(ws + pl.off_pdx), *part_w = reinterpret_cast<float *>(ws + pl.off_pw);
    const int rc = mcp_cross_pack(D, wpos, bpos, wmlp, bmlp, packed, stream);
    if (rc != MCP_OK) return rc;
    mcp_prof_begin(MCP_KERNEL_CROSS, s);
    hipLaunchKernelGGL(cross256_grad_z_kernel, dim3(pl.grid_z), dim3(64 * WAVES), Z_LDS_BYTES, s, total, n1, n2, xyz1, xyz2, points1, points2, idx, idx2,
                       packed, grad_out, grad_rows, jstar, gz);
    hipLaunchKernelGGL(cross256_grad_w_kernel, dim3(4 * pl.slices), dim3(256), 0, s, total, (int)pl.slices, grad_rows, jstar, gz, part_w);
    hipLaunchKernelGGL(cross256_grad_dx_kernel, dim3(pl.grid_dx), dim3(256), 0, s, total, n1, n2, xyz1, xyz2, idx, idx2, wpos, wmlp, jstar, gz, grad_rows,
                       grad_xyz1, grad_dir, grad_points1, part_dx);
    hipLaunchKernelGGL(cross256_grad_reduce_kernel, dim3((G_FLOATS + 255) / 256), dim3(256), 0, s, part_dx, (int)pl.grid_dx, part_w, (int)pl.slices,
                       grad_weights);
    mcp_prof_end(MCP_KERNEL_CROSS, s);
    return mcp_launch_status();
}
