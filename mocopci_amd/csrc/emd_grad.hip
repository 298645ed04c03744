// emd_grad.hip -- backward of the approximate Earth Mover's Distance (emd_cuda.matchcost_backward) for gfx950, and the
// explicit-match matchcost / matchcost_backward of the reference's emd_cuda API.
//
// Reference: models/EMD/cuda/emd_kernel.cu:204-247 (matchcost), matchcostgrad1 / matchcostgrad2.  The reference backward reads
// the materialised match (B,M,N) -- 256 MiB per batch element at 8192 points.  The lean backward here never builds it: the
// forward (mcp_emd_keep, emd.hip) keeps each level's ratioL / ratioR (10 x (N+M) floats per batch element), and every lane
// rebuilds match[l][k] = sum_j __expf(level_j d) ratioL_j[k] ratioR_j[l] for each pair with the forward's own expression and
// level order, so the match it differentiates is bit for bit the one the forward summed.
//   grad1: lane = point k of xyz1, xyz2 streamed through LDS tiles of (x, y, z, ratioR_0..9) (broadcast reads)
//   grad2: the mirror image, lane = point l of xyz2, xyz1 streamed with ratioL_0..9
// A workgroup is eight waves over the same 64 lane points; wave w takes entries [64w, 64w+64) of every 512-entry tile, and
// the eight partial sums are added in wave order at the end (fixed order, no atomics: bit-reproducible).  A level whose
// argument is below -128 for every lane of the wave is skipped: its __expf, and so its share of the match, is exactly 0.
//
// emd_grad_kernel is stated once with a compile-time LEN (emd_lengths.h).  LEN == true (mcp_emd_grad_lengths) bounds the lane
// points and the streamed tiles by the element's two lengths -- the same wave slices [64w, 64w+64) of every 512-entry tile and
// the same wave-order sum as the plain kernel on the prefixes -- and writes exact zeros to the rows beyond a length.
#include "common.h"
#include "emd_lengths.h"

namespace {

constexpr int NLEV = MCP_EMD_LEVELS;
constexpr int WAVES = 8, GBLK = 64 * WAVES, GTILE = 512, GQ = GTILE / WAVES;
// exp2f(-128 * log2(e)) = 2^-184.7: below the smallest float denormal, so __expf of any argument under -128 is exactly 0 and
// the level adds exactly 0 to every match entry of the wave.  Levels run from the steepest (-4^7) to 0, so once a level is
// live for a lane every later one is too.
constexpr float EMD_SKIP = -128.f;

struct Levels {
    float v[NLEV];
};
// level_j = -4^(7-j), j = 0..8, then 0: the values mcp_emd's loop passes its kernels (emd.hip)
Levels emd_levels() {
    Levels lv;
    for (int i = 0; i < NLEV; ++i) lv.v[i] = i == NLEV - 1 ? 0.f : -powf(4.0f, (float)(7 - i));
    return lv;
}

struct alignas(16) GradPt {
    float x, y, z, r[NLEV], pad[3];
};

// SIDE 1: lanes = xyz1 (grad1), streamed = xyz2 with ratioR.  SIDE 2: lanes = xyz2 (grad2), streamed = xyz1 with ratioL.
template <int SIDE, bool LEN>
__global__ __launch_bounds__(GBLK) void emd_grad_kernel(Levels lv, int n, int m, const float *__restrict__ grad_cost,
                                                       const float *__restrict__ xyz1, const float *__restrict__ xyz2,
                                                       const float *__restrict__ levels, float *__restrict__ grad,
                                                       const int *__restrict__ len1, const int *__restrict__ len2) {
    __shared__ GradPt tile[GTILE];
    __shared__ float part[WAVES][64][3];
    const int b = blockIdx.y;
    const int na = SIDE == 1 ? n : m;
    int nl, ml;
    emd_counts<LEN>(len1, len2, b, n, m, nl, ml);
    const int nal = SIDE == 1 ? nl : ml, nb = SIDE == 1 ? ml : nl;  // valid lane points, valid streamed points
    if (LEN && (int)blockIdx.x * 64 >= nal) {  // workgroup-uniform: nothing but padding here
        const int r = blockIdx.x * 64 + (int)threadIdx.x;
        if (threadIdx.x < 64 && r < na) {
            float *o = grad + ((size_t)b * na + r) * 3;
            o[0] = o[1] = o[2] = 0.f;
        }
        return;
    }
    const int offa = SIDE == 1 ? 0 : n, offb = SIDE == 1 ? n : 0;
    const size_t lstride = (size_t)n + m;
    const float *pa = SIDE == 1 ? xyz1 + (size_t)b * n * 3 : xyz2 + (size_t)b * m * 3;
    const float *pb = SIDE == 1 ? xyz2 + (size_t)b * m * 3 : xyz1 + (size_t)b * n * 3;
    const float *lev = levels + (size_t)b * NLEV * lstride;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i = blockIdx.x * 64 + lane;
    const bool live = i < nal;
    const int ii = live ? i : 0;  // dead lanes compute on point 0 (live: nal > 0 here) and store no sum
    const float xa = pa[(size_t)ii * 3], ya = pa[(size_t)ii * 3 + 1], za = pa[(size_t)ii * 3 + 2];
    float ra[NLEV];
#pragma unroll
    for (int j = 0; j < NLEV; ++j) ra[j] = lev[j * lstride + offa + ii];
    float gx = 0.f, gy = 0.f, gz = 0.f;
    for (int t0 = 0; t0 < nb; t0 += GTILE) {
        const int tend = min(nb, t0 + GTILE) - t0;
        __syncthreads();
        for (int t = threadIdx.x; t < tend; t += GBLK) {
            GradPt p;
            p.x = pb[(size_t)(t0 + t) * 3];
            p.y = pb[(size_t)(t0 + t) * 3 + 1];
            p.z = pb[(size_t)(t0 + t) * 3 + 2];
#pragma unroll
            for (int j = 0; j < NLEV; ++j) p.r[j] = lev[j * lstride + offb + t0 + t];
            p.pad[0] = p.pad[1] = p.pad[2] = 0.f;
            tile[t] = p;
        }
        __syncthreads();
        const int tb = wave * GQ, te = min(tend, tb + GQ);
        for (int t = tb; t < te; ++t) {
            const GradPt p = tile[t];
            // d exactly as emd.hip's d2(x1, y1, z1, x2, y2, z2) = mcp_sqdist3(x2, y2, z2, x1, y1, z1)
            const float d = SIDE == 1 ? mcp_sqdist3(p.x, p.y, p.z, xa, ya, za) : mcp_sqdist3(xa, ya, za, p.x, p.y, p.z);
            // match[l][k]: the forward's ((0 + w_0) + w_1) + ..., w_j = (__expf(level_j d) * ratioL_j) * ratioR_j.  A level that is
            // dead for every lane of the wave adds exactly 0 and is skipped (level 0, the last, is always live).
            float mt = 0.f;
#pragma unroll
            for (int j = 0; j < NLEV; ++j) {
                const float a = lv.v[j] * d;
                if (j == NLEV - 1 || __builtin_amdgcn_ballot_w64(a >= EMD_SKIP) != 0)
                    mt += __expf(a) * (SIDE == 1 ? ra[j] : p.r[j]) * (SIDE == 1 ? p.r[j] : ra[j]);
            }
            gx += (xa - p.x) * mt;
            gy += (ya - p.y) * mt;
            gz += (za - p.z) * mt;
        }
    }
    part[wave][lane][0] = gx;
    part[wave][lane][1] = gy;
    part[wave][lane][2] = gz;
    __syncthreads();
    if (wave == 0 && live) {
        const float g2 = 2.f * grad_cost[b];
        float *o = grad + ((size_t)b * na + i) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float s = part[0][lane][c];
#pragma unroll
            for (int w = 1; w < WAVES; ++w) s += part[w][lane][c];
            o[c] = s * g2;
        }
    }
    if (LEN && wave == 0 && !live && i < na) {  // a padded row beside live ones
        float *o = grad + ((size_t)b * na + i) * 3;
        o[0] = o[1] = o[2] = 0.f;
    }
}

// ---- explicit match (B,M,N) ----

// cost[b] = sum_{l,k} match[l][k] d(l,k): lane t sums k = t, t+1024, ... over ascending l, then a fixed tree over the lanes.
// The float products are summed in double: one lane adds up to n*m/1024 of them (65536 at 8192 points), and a float
// accumulator drifts by a few 1e-6 over that many terms.
constexpr int CBLK = 1024;
__global__ __launch_bounds__(CBLK) void matchcost_kernel(int n, int m, const float *__restrict__ xyz1, const float *__restrict__ xyz2,
                                                         const float *__restrict__ match, float *__restrict__ cost) {
    __shared__ double red[CBLK];
    const int b = blockIdx.x;
    const float *p1 = xyz1 + (size_t)b * n * 3, *p2 = xyz2 + (size_t)b * m * 3;
    const float *mb = match + (size_t)b * m * n;
    double s = 0.0;
    for (int k = threadIdx.x; k < n; k += CBLK) {
        const float x1 = p1[(size_t)k * 3], y1 = p1[(size_t)k * 3 + 1], z1 = p1[(size_t)k * 3 + 2];
        for (int l = 0; l < m; ++l) {
            const float d = mcp_sqdist3(p2[(size_t)l * 3], p2[(size_t)l * 3 + 1], p2[(size_t)l * 3 + 2], x1, y1, z1);
            s += (double)(d * mb[(size_t)l * n + k]);
        }
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int h = CBLK / 2; h > 0; h >>= 1) {
        if (threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) cost[b] = (float)red[0];
}

// grad1[k]: lane = k (each match row read along k), wave w sums l in the w-th contiguous eighth of [0, m), added in order
__global__ __launch_bounds__(GBLK) void matchcost_grad1_kernel(int n, int m, const float *__restrict__ grad_cost,
                                                               const float *__restrict__ xyz1, const float *__restrict__ xyz2,
                                                               const float *__restrict__ match, float *__restrict__ grad1) {
    __shared__ float part[WAVES][64][3];
    const int b = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int k = blockIdx.x * 64 + lane;
    const bool live = k < n;
    const int kk = live ? k : 0;
    const float *p1 = xyz1 + ((size_t)b * n + kk) * 3, *p2 = xyz2 + (size_t)b * m * 3;
    const float *mcol = match + (size_t)b * m * n + kk;
    const float x1 = p1[0], y1 = p1[1], z1 = p1[2];
    const int lb = (int)((long long)m * wave / WAVES), le = (int)((long long)m * (wave + 1) / WAVES);
    float gx = 0.f, gy = 0.f, gz = 0.f;
    for (int l = lb; l < le; ++l) {
        const float mv = mcol[(size_t)l * n];
        gx += (x1 - p2[(size_t)l * 3]) * mv;
        gy += (y1 - p2[(size_t)l * 3 + 1]) * mv;
        gz += (z1 - p2[(size_t)l * 3 + 2]) * mv;
    }
    part[wave][lane][0] = gx;
    part[wave][lane][1] = gy;
    part[wave][lane][2] = gz;
    __syncthreads();
    if (wave == 0 && live) {
        const float g2 = 2.f * grad_cost[b];
        float *o = grad1 + ((size_t)b * n + k) * 3;
        for (int c = 0; c < 3; ++c) {
            float s = part[0][lane][c];
            for (int w = 1; w < WAVES; ++w) s += part[w][lane][c];
            o[c] = s * g2;
        }
    }
}

// grad2[l]: a workgroup per ROWS rows l; lane t sums k = t, t+256, ... (coalesced along k), then a fixed tree over the 256 lanes
constexpr int ROWS = 8, RBLK = 256;
__global__ __launch_bounds__(RBLK) void matchcost_grad2_kernel(int n, int m, const float *__restrict__ grad_cost,
                                                               const float *__restrict__ xyz1, const float *__restrict__ xyz2,
                                                               const float *__restrict__ match, float *__restrict__ grad2) {
    __shared__ float red[ROWS * 3][RBLK];
    const int b = blockIdx.y, l0 = blockIdx.x * ROWS;
    const int rows = min(ROWS, m - l0);
    const float *p1 = xyz1 + (size_t)b * n * 3, *p2 = xyz2 + ((size_t)b * m + l0) * 3;
    const float *mrow = match + ((size_t)b * m + l0) * n;
    float x2[ROWS], y2[ROWS], z2[ROWS], acc[ROWS][3];
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        const int rr = r < rows ? r : 0;
        x2[r] = p2[rr * 3];
        y2[r] = p2[rr * 3 + 1];
        z2[r] = p2[rr * 3 + 2];
        acc[r][0] = acc[r][1] = acc[r][2] = 0.f;
    }
    for (int k = threadIdx.x; k < n; k += RBLK) {
        const float x1 = p1[(size_t)k * 3], y1 = p1[(size_t)k * 3 + 1], z1 = p1[(size_t)k * 3 + 2];
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            const float mv = r < rows ? mrow[(size_t)r * n + k] : 0.f;
            acc[r][0] += (x2[r] - x1) * mv;
            acc[r][1] += (y2[r] - y1) * mv;
            acc[r][2] += (z2[r] - z1) * mv;
        }
    }
#pragma unroll
    for (int r = 0; r < ROWS; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) red[r * 3 + c][threadIdx.x] = acc[r][c];
    __syncthreads();
    for (int h = RBLK / 2; h > 0; h >>= 1) {
        if (threadIdx.x < h)
#pragma unroll
            for (int q = 0; q < ROWS * 3; ++q) red[q][threadIdx.x] += red[q][threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x < rows * 3) grad2[((size_t)b * m + l0) * 3 + threadIdx.x] = red[threadIdx.x][0] * (2.f * grad_cost[b]);
}

}  // namespace

namespace {
template <bool LEN>
int emd_grad_run(int b, int n, int m, const float *grad_cost, const float *xyz1, const float *xyz2, const int *len1, const int *len2,
                 const float *levels, float *grad1, float *grad2, hipStream_t s) {
    const Levels lv = emd_levels();
    if (grad1)
        hipLaunchKernelGGL((emd_grad_kernel<1, LEN>), dim3(mcp_divup(n, 64), b), dim3(GBLK), 0, s, lv, n, m, grad_cost, xyz1, xyz2, levels,
                           grad1, len1, len2);
    if (grad2)
        hipLaunchKernelGGL((emd_grad_kernel<2, LEN>), dim3(mcp_divup(m, 64), b), dim3(GBLK), 0, s, lv, n, m, grad_cost, xyz1, xyz2, levels,
                           grad2, len1, len2);
    return mcp_launch_status();
}
}  // namespace

MCP_EXPORT int mcp_emd_grad(int b, int n, int m, const float *grad_cost, const float *xyz1, const float *xyz2, const float *levels,
                            float *grad1, float *grad2, mcp_stream_t stream) {
    MCP_CHECK_ARGS(b > 0 && n > 0 && m > 0 && grad_cost && xyz1 && xyz2 && levels);
    return emd_grad_run<false>(b, n, m, grad_cost, xyz1, xyz2, nullptr, nullptr, levels, grad1, grad2, (hipStream_t)stream);
}

MCP_EXPORT int mcp_emd_grad_lengths(int b, int n, int m, const float *grad_cost, const float *xyz1, const float *xyz2, const int *len1,
                                    const int *len2, const float *levels, float *grad1, float *grad2, mcp_stream_t stream) {
    MCP_CHECK_ARGS(b > 0 && n > 0 && m > 0 && grad_cost && xyz1 && xyz2 && levels);
    if (!len1 && !len2)
        return emd_grad_run<false>(b, n, m, grad_cost, xyz1, xyz2, nullptr, nullptr, levels, grad1, grad2, (hipStream_t)stream);
    return emd_grad_run<true>(b, n, m, grad_cost, xyz1, xyz2, len1, len2, levels, grad1, grad2, (hipStream_t)stream);
}

MCP_EXPORT int mcp_matchcost(int b, int n, int m, const float *xyz1, const float *xyz2, const float *match, float *cost,
                             mcp_stream_t stream) {
    MCP_CHECK_ARGS(b > 0 && n > 0 && m > 0 && xyz1 && xyz2 && match && cost);
    hipLaunchKernelGGL(matchcost_kernel, dim3(b), dim3(CBLK), 0, (hipStream_t)stream, n, m, xyz1, xyz2, match, cost);
    return mcp_launch_status();
}

MCP_EXPORT int mcp_matchcost_grad(int b, int n, int m, const float *grad_cost, const float *xyz1, const float *xyz2, const float *match,
                                  float *grad1, float *grad2, mcp_stream_t stream) {
    MCP_CHECK_ARGS(b > 0 && n > 0 && m > 0 && grad_cost && xyz1 && xyz2 && match);
    hipStream_t s = (hipStream_t)stream;
    if (grad1)
        hipLaunchKernelGGL(matchcost_grad1_kernel, dim3(mcp_divup(n, 64), b), dim3(GBLK), 0, s, n, m, grad_cost, xyz1, xyz2, match, grad1);
    if (grad2)
        hipLaunchKernelGGL(matchcost_grad2_kernel, dim3(mcp_divup(m, ROWS), b), dim3(RBLK), 0, s, n, m, grad_cost, xyz1, xyz2, match, grad2);
    return mcp_launch_status();
}
