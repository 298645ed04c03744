// bn_batch.hip -- BatchNorm on BATCH statistics (net.train()) of a channels-last tensor x (G, F, N, C) whose G groups are normalised
// separately (the reference's per-sample loops over norm1 / norm2 of its attention blocks), forward and backward, with per-group
// lengths: row (f, i) of group g is live iff i < len[g], every statistic and every mean term of the backward runs over the
// m_g = F * len[g] live rows only, padded rows are never read and come out as exact zeros.
//
// A group's F * N padded rows are cut into `parts` chunks of `rows` rows each -- a pure function of (f, n), never of the CU count or of
// a length (bnb_chunking) -- and one workgroup of 256 threads takes one chunk: lane q of C / 4 owns a float4 channel quad, the
// 1024 / C row lanes walk the chunk's rows side by side.  Forward:
//   bnb_sums_kernel<C, STATS>   per part and channel, the sums of (x - s) and (x - s)^2 over the part's live rows, s = x[g,0,0,:] (live
//                               whenever any row is): in double, per thread in row order, then the row lanes in lane order;
//   bnb_stats_merge_kernel      the parts of a group in part order, in double: mean = s + S1 / m, var = S2 / m - (S1 / m)^2, count = m;
//   bnb_apply_kernel<C, FWD>    y = (x - mean) * (gamma * rstd) + beta on live rows, zeros on padded ones.
// Backward (x, mean and var are all that is kept: xhat = (x - mean) * rstd is formed again):
//   bnb_sums_kernel<C, GRAD>    the sums of dy and dy * xhat; bnb_grad_merge_kernel merges the parts in part order;
//   bnb_affine_kernel           grad_beta / grad_gamma = the groups' sums in group order;
//   bnb_apply_kernel<C, BWD>    dx = gamma * rstd * (dy - sum(dy) / m - xhat * sum(dy * xhat) / m) on live rows, zeros on padded ones.
// Every division is by max(m, 1).  No atomics, no allocation, no length read on the host: two calls give identical bits, and
// len[g] == n everywhere walks exactly what len == NULL walks.  Scalar float arithmetic only (see mcp_f2 in common.h).
#include "common.h"

namespace {

constexpr int BNB_THREADS = 256;
constexpr int BNB_PART_ROWS = 256;   // the smallest chunk
constexpr int BNB_MAX_PARTS = 128;   // per group: what the merge kernels walk in sequence
constexpr int BNB_ROW_STEP = 32;     // chunks are multiples of every C's row lanes (1024 / C <= 32)

enum { BNB_STATS = 0, BNB_GRAD = 1, BNB_FWD = 0, BNB_BWD = 1 };

struct BnbChunking {
    int parts, rows;
};
static BnbChunking bnb_chunking(long long total) {
    long long parts = (total + BNB_PART_ROWS - 1) / BNB_PART_ROWS;
    parts = parts < 1 ? 1 : (parts > BNB_MAX_PARTS ? BNB_MAX_PARTS : parts);
    long long rows = (total + parts - 1) / parts;
    rows = (rows + BNB_ROW_STEP - 1) / BNB_ROW_STEP * BNB_ROW_STEP;
    parts = (total + rows - 1) / rows;
    return BnbChunking{(int)(parts < 1 ? 1 : parts), (int)rows};
}

static bool bnb_supported(int c) { return c == 32 || c == 64 || c == 128 || c == 256; }
static bool bnb_sizes_ok(int g, int f, int n, int c) {
    return g > 0 && f > 0 && n > 0 && c > 0 && g <= 65535 && (long long)f * n <= (1LL << 30);   // row indices and a chunk's end fit an int
}
static size_t bnb_workspace_bytes(int g, int parts, int c) {
    return ((size_t)g * parts + (size_t)g) * 2 * c * sizeof(double);   // (G, parts, 2, C) partial sums | (G, 2, C) merged sums
}
static bool bnb_aligned(const void *p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// the one expression of rstd: the backward's xhat is the forward's
__device__ __forceinline__ float bnb_rstd(float var, float eps) { return 1.0f / sqrtf(var + eps); }

struct BnbQuad {
    float v[4];
};
__device__ __forceinline__ BnbQuad bnb_load(const float *p) {
    const float4 t = *reinterpret_cast<const float4 *>(p);
    return BnbQuad{{t.x, t.y, t.z, t.w}};
}
__device__ __forceinline__ void bnb_store(float *p, const BnbQuad &q) { *reinterpret_cast<float4 *>(p) = make_float4(q.v[0], q.v[1], q.v[2], q.v[3]); }

// This thread's rows of chunk [first, last) of a group's f * n rows: fn(row, live) in row order, live = (row mod n) < ln.
template <int C, typename Fn>
__device__ __forceinline__ void bnb_walk(int n, int ln, int first, int last, Fn fn) {
    constexpr int LANES = BNB_THREADS / (C / 4);
    int r = first + (int)threadIdx.x / (C / 4);
    if (r >= last) return;
    int i = r % n;
    const int step = LANES % n;
    for (; r < last; r += LANES) {
        fn(r, i < ln);
        i += step;
        if (i >= n) i -= n;
    }
}

// STATS: sums of (x - s) | (x - s)^2;  GRAD: sums of dy | dy * xhat -- over the live rows of one chunk, per channel, into part (G, parts, 2, C).
template <int C, int MODE>
__global__ __launch_bounds__(BNB_THREADS) void bnb_sums_kernel(int f, int n, int part_rows, const float *__restrict__ x, const int *__restrict__ len,
                                                                 const float *__restrict__ mean, const float *__restrict__ var, float eps,
                                                                 const float *__restrict__ dy, double *__restrict__ part) {
    constexpr int QUADS = C / 4, LANES = BNB_THREADS / QUADS;
    __shared__ double lds[2][LANES][C];
    const int g = blockIdx.y, p = blockIdx.x, parts = gridDim.x;
    const int total = f * n, ln = mcp_clamped_len(len, g, n);
    const int first = p * part_rows, last = first + part_rows < total ? first + part_rows : total;
    const int q = (int)threadIdx.x % QUADS, lane = (int)threadIdx.x / QUADS;
    const size_t base = (size_t)g * total * C + 4 * q;
    double a[4] = {0.0, 0.0, 0.0, 0.0}, b[4] = {0.0, 0.0, 0.0, 0.0};   // double adds run at the float rate here and the kernel waits on memory
    if (ln > 0) {
        BnbQuad s, k;   // STATS: the shift | unused;  GRAD: mean | rstd
        if (MODE == BNB_STATS) {
            s = bnb_load(x + base);
        } else {
            s = bnb_load(mean + (size_t)g * C + 4 * q);
            const BnbQuad v = bnb_load(var + (size_t)g * C + 4 * q);
#pragma unroll
            for (int j = 0; j < 4; ++j) k.v[j] = bnb_rstd(v.v[j], eps);
        }
        bnb_walk<C>(n, ln, first, last, [&](int r, bool live) {
            if (!live) return;
            const BnbQuad xv = bnb_load(x + base + (size_t)r * C);
            if (MODE == BNB_STATS) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const double d = (double)xv.v[j] - (double)s.v[j];
                    a[j] += d;
                    b[j] += d * d;
                }
            } else {
                const BnbQuad gv = bnb_load(dy + base + (size_t)r * C);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float xhat = (xv.v[j] - s.v[j]) * k.v[j];
                    a[j] += (double)gv.v[j];
                    b[j] += (double)gv.v[j] * (double)xhat;
                }
            }
        });
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        lds[0][lane][4 * q + j] = a[j];
        lds[1][lane][4 * q + j] = b[j];
    }
    __syncthreads();
    for (int k = (int)threadIdx.x; k < 2 * C; k += BNB_THREADS) {
        const int which = k / C, ch = k % C;
        double acc = 0.0;
#pragma unroll
        for (int l = 0; l < LANES; ++l) acc += lds[which][l][ch];
        part[(((size_t)g * parts + p) * 2 + which) * C + ch] = acc;
    }
}

// one workgroup per group, one thread per channel: the parts in part order
__global__ void bnb_stats_merge_kernel(int f, int n, int c, int parts, const float *__restrict__ x, const int *__restrict__ len,
                                       const double *__restrict__ part, float *__restrict__ mean, float *__restrict__ var, int *__restrict__ count) {
    const int g = blockIdx.x, ch = threadIdx.x;
    const int m = f * mcp_clamped_len(len, g, n);
    const double *pg = part + (size_t)g * parts * 2 * c + ch;
    double s1 = 0.0, s2 = 0.0;
#pragma unroll 8
    for (int p = 0; p < parts; ++p) {
        s1 += pg[(size_t)p * 2 * c];
        s2 += pg[(size_t)p * 2 * c + c];
    }
    const double dm = m > 1 ? (double)m : 1.0;
    const double shift = m > 0 ? (double)x[(size_t)g * f * n * c + ch] : 0.0;
    const double mu = s1 / dm;
    double v = s2 / dm - mu * mu;
    if (!(v > 0.0)) v = 0.0;
    mean[(size_t)g * c + ch] = (float)(shift + mu);
    var[(size_t)g * c + ch] = (float)v;
    if (ch == 0) count[g] = m;
}

__global__ void bnb_grad_merge_kernel(int c, int parts, const double *__restrict__ part, double *__restrict__ sums) {
    const int g = blockIdx.x, ch = threadIdx.x;
    const double *pg = part + (size_t)g * parts * 2 * c + ch;
    double s1 = 0.0, s2 = 0.0;
#pragma unroll 8
    for (int p = 0; p < parts; ++p) {
        s1 += pg[(size_t)p * 2 * c];
        s2 += pg[(size_t)p * 2 * c + c];
    }
    sums[(size_t)g * 2 * c + ch] = s1;
    sums[(size_t)g * 2 * c + c + ch] = s2;
}

// grad_beta = sum_g sum(dy), grad_gamma = sum_g sum(dy * xhat): the groups in group order
__global__ void bnb_affine_kernel(int g, int c, const double *__restrict__ sums, float *__restrict__ grad_gamma, float *__restrict__ grad_beta) {
    const int ch = threadIdx.x;
    double s1 = 0.0, s2 = 0.0;
    for (int k = 0; k < g; ++k) {
        s1 += sums[(size_t)k * 2 * c + ch];
        s2 += sums[(size_t)k * 2 * c + c + ch];
    }
    grad_beta[ch] = (float)s1;
    grad_gamma[ch] = (float)s2;
}

// FWD: out = y;  BWD: out = dx (in = dy, sums = the group's merged sums).  Padded rows of out are zeros; padded rows of x / in are not read.
template <int C, int MODE>
__global__ __launch_bounds__(BNB_THREADS) void bnb_apply_kernel(int f, int n, int part_rows, const float *__restrict__ x, const int *__restrict__ len,
                                                                  const float *__restrict__ gamma, const float *__restrict__ beta,
                                                                  const float *__restrict__ mean, const float *__restrict__ var, float eps,
                                                                  const float *__restrict__ in, const double *__restrict__ sums, float *__restrict__ out) {
    constexpr int QUADS = C / 4;
    const int g = blockIdx.y, p = blockIdx.x;
    const int total = f * n, ln = mcp_clamped_len(len, g, n);
    const int first = p * part_rows, last = first + part_rows < total ? first + part_rows : total;
    const int q = (int)threadIdx.x % QUADS;
    const size_t base = (size_t)g * total * C + 4 * q;
    const BnbQuad mu = bnb_load(mean + (size_t)g * C + 4 * q), vr = bnb_load(var + (size_t)g * C + 4 * q), ga = bnb_load(gamma + 4 * q);
    BnbQuad rstd, scale, k1, k2;   // FWD: k1 = beta;  BWD: k1 = sum(dy) / m, k2 = sum(dy * xhat) / m
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        rstd.v[j] = bnb_rstd(vr.v[j], eps);
        scale.v[j] = ga.v[j] * rstd.v[j];
    }
    if (MODE == BNB_FWD) {
        k1 = bnb_load(beta + 4 * q);
    } else {
        const int m = f * ln;
        const double dm = m > 1 ? (double)m : 1.0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            k1.v[j] = (float)(sums[(size_t)g * 2 * C + 4 * q + j] / dm);
            k2.v[j] = (float)(sums[(size_t)g * 2 * C + C + 4 * q + j] / dm);
        }
    }
    bnb_walk<C>(n, ln, first, last, [&](int r, bool live) {
        BnbQuad o{{0.f, 0.f, 0.f, 0.f}};
        if (live) {
            const BnbQuad xv = bnb_load(x + base + (size_t)r * C);
            if (MODE == BNB_FWD) {
#pragma unroll
                for (int j = 0; j < 4; ++j) o.v[j] = (xv.v[j] - mu.v[j]) * scale.v[j] + k1.v[j];
            } else {
                const BnbQuad gv = bnb_load(in + base + (size_t)r * C);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float xhat = (xv.v[j] - mu.v[j]) * rstd.v[j];
                    o.v[j] = scale.v[j] * ((gv.v[j] - k1.v[j]) - xhat * k2.v[j]);
                }
            }
        }
        bnb_store(out + base + (size_t)r * C, o);
    });
}

template <int C>
int bnb_forward(int g, int f, int n, const float *x, const int *len, const float *gamma, const float *beta, float eps, float *mean, float *var, int *count,
                float *y, double *part, hipStream_t st) {
    const BnbChunking ck = bnb_chunking((long long)f * n);
    const dim3 grid(ck.parts, g);
    hipLaunchKernelGGL((bnb_sums_kernel<C, BNB_STATS>), grid, dim3(BNB_THREADS), 0, st, f, n, ck.rows, x, len, nullptr, nullptr, eps, nullptr, part);
    hipLaunchKernelGGL(bnb_stats_merge_kernel, dim3(g), dim3(C), 0, st, f, n, C, ck.parts, x, len, part, mean, var, count);
    hipLaunchKernelGGL((bnb_apply_kernel<C, BNB_FWD>), grid, dim3(BNB_THREADS), 0, st, f, n, ck.rows, x, len, gamma, beta, mean, var, eps, nullptr, nullptr, y);
    return mcp_launch_status();
}

template <int C>
int bnb_backward(int g, int f, int n, const float *x, const int *len, const float *gamma, const float *mean, const float *var, float eps, const float *grad_y,
                 float *grad_x, float *grad_gamma, float *grad_beta, double *part, hipStream_t st) {
    const BnbChunking ck = bnb_chunking((long long)f * n);
    const dim3 grid(ck.parts, g);
    double *sums = part + (size_t)g * ck.parts * 2 * C;
    hipLaunchKernelGGL((bnb_sums_kernel<C, BNB_GRAD>), grid, dim3(BNB_THREADS), 0, st, f, n, ck.rows, x, len, mean, var, eps, grad_y, part);
    hipLaunchKernelGGL(bnb_grad_merge_kernel, dim3(g), dim3(C), 0, st, C, ck.parts, part, sums);
    hipLaunchKernelGGL(bnb_affine_kernel, dim3(1), dim3(C), 0, st, g, C, sums, grad_gamma, grad_beta);
    hipLaunchKernelGGL((bnb_apply_kernel<C, BNB_BWD>), grid, dim3(BNB_THREADS), 0, st, f, n, ck.rows, x, len, gamma, nullptr, mean, var, eps, grad_y, sums, grad_x);
    return mcp_launch_status();
}

}  // namespace

// include/mocopci_hip.h
MCP_EXPORT int mcp_bn_batch_parts(int g, int f, int n, int c) {
    MCP_CHECK_ARGS(bnb_sizes_ok(g, f, n, c));
    if (!bnb_supported(c)) return MCP_ERR_UNSUPPORTED;
    return bnb_chunking((long long)f * n).parts;
}

MCP_EXPORT size_t mcp_bn_batch_workspace_bytes(int g, int f, int n, int c) {
    if (!bnb_sizes_ok(g, f, n, c) || !bnb_supported(c)) return 0;
    return bnb_workspace_bytes(g, bnb_chunking((long long)f * n).parts, c);
}

MCP_EXPORT int mcp_bn_batch_forward(int g, int f, int n, int c, const float *x, const int *len, const float *gamma, const float *beta, float eps, float *mean,
                                    float *var, int *count, float *y, void *workspace, size_t workspace_bytes, mcp_stream_t stream) {
    MCP_CHECK_ARGS(bnb_sizes_ok(g, f, n, c) && x && gamma && beta && mean && var && count && y && workspace);
    if (!bnb_supported(c)) return MCP_ERR_UNSUPPORTED;
    MCP_CHECK_ARGS(workspace_bytes >= mcp_bn_batch_workspace_bytes(g, f, n, c) && bnb_aligned(workspace, 8));
    MCP_CHECK_ARGS(bnb_aligned(x, 16) && bnb_aligned(y, 16) && bnb_aligned(gamma, 16) && bnb_aligned(beta, 16) && bnb_aligned(mean, 16) && bnb_aligned(var, 16));
    hipStream_t st = (hipStream_t)stream;
    double *part = (double *)workspace;
    switch (c) {
        case 32: return bnb_forward<32>(g, f, n, x, len, gamma, beta, eps, mean, var, count, y, part, st);
        case 64: return bnb_forward<64>(g, f, n, x, len, gamma, beta, eps, mean, var, count, y, part, st);
        case 128: return bnb_forward<128>(g, f, n, x, len, gamma, beta, eps, mean, var, count, y, part, st);
        default: return bnb_forward<256>(g, f, n, x, len, gamma, beta, eps, mean, var, count, y, part, st);
    }
}

MCP_EXPORT int mcp_bn_batch_backward(int g, int f, int n, int c, const float *x, const int *len, const float *gamma, const float *mean, const float *var,
                                     float eps, const float *grad_y, float *grad_x, float *grad_gamma, float *grad_beta, void *workspace,
                                     size_t workspace_bytes, mcp_stream_t stream) {
    MCP_CHECK_ARGS(bnb_sizes_ok(g, f, n, c) && x && gamma && mean && var && grad_y && grad_x && grad_gamma && grad_beta && workspace);
    if (!bnb_supported(c)) return MCP_ERR_UNSUPPORTED;
    MCP_CHECK_ARGS(workspace_bytes >= mcp_bn_batch_workspace_bytes(g, f, n, c) && bnb_aligned(workspace, 8));
    MCP_CHECK_ARGS(bnb_aligned(x, 16) && bnb_aligned(grad_y, 16) && bnb_aligned(grad_x, 16) && bnb_aligned(gamma, 16) && bnb_aligned(mean, 16) &&
                   bnb_aligned(var, 16));
    hipStream_t st = (hipStream_t)stream;
    double *part = (double *)workspace;
    switch (c) {
        case 32: return bnb_backward<32>(g, f, n, x, len, gamma, mean, var, eps, grad_y, grad_x, grad_gamma, grad_beta, part, st);
        case 64: return bnb_backward<64>(g, f, n, x, len, gamma, mean, var, eps, grad_y, grad_x, grad_gamma, grad_beta, part, st);
        case 128: return bnb_backward<128>(g, f, n, x, len, gamma, mean, var, eps, grad_y, grad_x, grad_gamma, grad_beta, part, st);
        default: return bnb_backward<256>(g, f, n, x, len, gamma, mean, var, eps, grad_y, grad_x, grad_gamma, grad_beta, part, st);
    }
}
