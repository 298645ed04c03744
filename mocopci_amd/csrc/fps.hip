// fps.hip -- furthest point sampling for gfx950 (replaces pointnet2/src/sampling_gpu.cu:93-253).
//
// The reference runs one 1024-thread block per batch element that re-streams xyz and temp
// from global memory on each of the M-1 dependent iterations (20 B/point/iteration) and
// reduces through a 10-level LDS tree with 10 barriers.  Here one workgroup per batch
// element keeps its points AND their running min-distances in VGPRs for the whole call
// (N=8192: 8 points x 4 floats per lane), stages xyz once in LDS so the next centre is an
// LDS broadcast read, and reduces with DPP row ops + one LDS hop + ONE barrier per
// iteration (double-buffered slots).  HBM traffic is the compulsory 12N+4N+4M bytes.
//
// Index parity with the reference, including ties.  The reference's per-thread scan uses a
// strict '>' over k = tid, tid+bs, ... and its tree keeps the lower slot on equal values,
// so among equal distances the winner minimises (bitrev_L(k mod bs), k div bs) with
// bs = 2^L the reference block size (cuda_utils.h:10-14).  That is a total order on points,
// so any reduction shape gives the same answer: we reduce the pair
//   (ord(d2), ~sec(k)),  sec(k) = bitrev_L(k mod bs) << (32-L) | (k >> L)
// by max.  Distances use the canon of common.h (= oracle/pointset_oracle.c).
//
// The two spatially pruned kernels (fps_spatial_kernel, fps_tiled_kernel), their launchers and fps_emit_points are stated in
// fps_pruned.h, shared with the per-cloud-length forms of fps_lengths.hip; FPS_LEN 0: every element is a whole cloud.
#include <math.h>
#include <stdlib.h>

#define FPS_LEN 0
#include "fps_pruned.h"

// workgroup shape for 4 / 8 points per reference thread (T = 1024 >> J, P points per physical thread)
#ifndef MCP_FPS_J8
#define MCP_FPS_J8 1
#endif
#ifndef MCP_FPS_J4
#define MCP_FPS_J4 1
#endif
#define MCP_FPS_T8 (1024 >> MCP_FPS_J8)
#define MCP_FPS_P8 (8 << MCP_FPS_J8)
#define MCP_FPS_T4 (1024 >> MCP_FPS_J4)
#define MCP_FPS_P4 (4 << MCP_FPS_J4)

namespace {

__device__ __forceinline__ uint32_t fps_sec(uint32_t k, int L) {
    if (L == 0) return k;
    uint32_t vt = k & ((1u << L) - 1u);
    return (__brev(vt) & ~((1u << (32 - L)) - 1u)) | (k >> L);  // brev puts the L bits at the top
}
__device__ __forceinline__ uint32_t fps_unsec(uint32_t sec, int L) {
    if (L == 0) return sec;
    uint32_t vt = __brev(sec & ~((1u << (32 - L)) - 1u));
    return vt | ((sec & ((1u << (32 - L)) - 1u)) << L);
}

// T threads, P points per thread (k = tid + T*p).  The reference block has bs = 2^L threads; T = bs >> J.
// J == 0: a physical thread is exactly one reference thread and its strict-'>' scan returns the first
// maximum in ascending p.  J == 1 (T = bs/2): a thread holds two reference threads (even p -> tid,
// odd p -> tid + T); bitrev_L(tid + T) = bitrev_L(tid) + 1, so among equal values the even-p points win,
// each group in ascending p.  GENERIC (n < 64): every compare uses the full (ord, ~sec) pair.
template <int T, int P, int J, bool GENERIC, bool LDS_XYZ>
__global__ __launch_bounds__(T) void fps_resident_kernel(int n, int m, int L, const float *__restrict__ xyz,
                                                         float *__restrict__ temp, int *__restrict__ idxs, float *__restrict__ pts) {
    constexpr int W = T / 64;
    extern __shared__ float4 smem_f4[];
    unsigned long long *slots = reinterpret_cast<unsigned long long *>(smem_f4);  // [3] rotating max slots (+pad to 64 B)
    float *sxyz = reinterpret_cast<float *>(smem_f4) + 16;                        // [n*3] when LDS_XYZ
    // [m] selected indices, written out once at the end: a global store per iteration would sit in front of every barrier
    int *sidx = reinterpret_cast<int *>(sxyz + (LDS_XYZ ? n * 3 : 0));

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    xyz += (size_t)blockIdx.x * n * 3;
    if (temp) temp += (size_t)blockIdx.x * n;  // NULL: a fresh sampling -- every running distance starts at 1e10 and is not stored
    idxs += (size_t)blockIdx.x * m;
    if (pts) pts += (size_t)blockIdx.x * m * 3;

    float px[P], py[P], pz[P], pt[P];
    uint32_t nsec[P];
#pragma unroll
    for (int j = 0; j < P; ++j) {
        int k = tid + T * j;
        bool ok = k < n;
        int kk = ok ? k : 0;
        px[j] = xyz[kk * 3 + 0];
        py[j] = xyz[kk * 3 + 1];
        pz[j] = xyz[kk * 3 + 2];
        pt[j] = ok ? (temp ? temp[kk] : 1e10f) : -INFINITY;  // padding: never selected, never stored
        nsec[j] = ~fps_sec((uint32_t)kk, L);
    }
    if (LDS_XYZ) {
        for (int i = tid; i < n * 3; i += T) sxyz[i] = xyz[i];
    }
    if (tid < 3) slots[tid] = 0ull;
    if (tid == 0) sidx[0] = 0;
    __syncthreads();

    int old = 0;
    int s_cur = 0, s_nxt = 1;
#ifdef MCP_FPS_DIAG
    unsigned long long t_prev = 0;
    FPS_STAMP(7);
#endif
    for (int j = 1; j < m; ++j) {
        float x1, y1, z1;
        if (LDS_XYZ) {
            x1 = sxyz[old * 3 + 0]; y1 = sxyz[old * 3 + 1]; z1 = sxyz[old * 3 + 2];
        } else {
            x1 = xyz[old * 3 + 0]; y1 = xyz[old * 3 + 1]; z1 = xyz[old * 3 + 2];
        }
        FPS_STAMP(0);  // centre read
        uint32_t hi, lo;
        if (!GENERIC) {
            // track only the maximum VALUE in the scan (packed fp32 math); which point holds it is found afterwards
            float best;
            if constexpr (P >= 2) {
                const f2 c0 = {x1, x1}, c1 = {y1, y1}, c2 = {z1, z1};
                f2 m2 = {-1.0f, -1.0f};
#pragma unroll
                for (int p = 0; p < P; p += 2) {
                    const f2 dx = f2{px[p], px[p + 1]} - c0, dy = f2{py[p], py[p + 1]} - c1, dz = f2{pz[p], pz[p + 1]} - c2;
                    const f2 d = f2_fma(dz, dz, f2_fma(dy, dy, dx * dx));
                    pt[p] = mcp_min_raw(d.x, pt[p]);  // raw v_min / v_max: fminf / fmaxf first canonicalise an operand (an extra
                    pt[p + 1] = mcp_min_raw(d.y, pt[p + 1]);  // instruction each); nothing here is ever NaN
                    m2.x = mcp_max_raw(m2.x, pt[p]);
                    m2.y = mcp_max_raw(m2.y, pt[p + 1]);
                }
                best = mcp_max_raw(m2.x, m2.y);
            } else {
                pt[0] = fminf(mcp_sqdist3(px[0], py[0], pz[0], x1, y1, z1), pt[0]);
                best = fmaxf(-1.0f, pt[0]);
            }
            hi = mcp_ord(best);
            FPS_STAMP(1);  // scan
            const uint32_t whi = mcp_wave_max_u32(hi);
            // tie order inside the thread: reverse-priority assignment chain, highest priority assigned last.
            // (An independent-select + max-tree form was measured 4 % SLOWER: this phase is bound by instruction
            // count -- about 12 cycles per instruction with the DPP / SGPR-mask hazards -- not by the chain's depth.)
            uint32_t bsec = 0;
            if constexpr (J == 1) {
#pragma unroll
                for (int p = P - 1; p >= 1; p -= 2) bsec = pt[p] == best ? nsec[p] : bsec;  // odd p (reference thread tid+T)
#pragma unroll
                for (int p = P - 2; p >= 0; p -= 2) bsec = pt[p] == best ? nsec[p] : bsec;  // even p (reference thread tid)
            } else {
#pragma unroll
                for (int p = P - 1; p >= 0; --p) bsec = pt[p] == best ? nsec[p] : bsec;
            }
            lo = hi == whi ? bsec : 0u;
            hi = whi;
        } else {
            hi = 0; lo = 0;
#pragma unroll
            for (int p = 0; p < P; ++p) {
                float d = mcp_sqdist3(px[p], py[p], pz[p], x1, y1, z1);
                float d2 = fminf(d, pt[p]);
                pt[p] = d2;
                uint32_t h = mcp_ord(d2);
                bool gt = (h > hi) || (h == hi && nsec[p] > lo);
                lo = gt ? nsec[p] : lo;
                hi = gt ? h : hi;
            }
            const uint32_t whi = mcp_wave_max_u32(hi);
            lo = hi == whi ? lo : 0u;
            hi = whi;
        }
        uint32_t wlo = mcp_wave_max_u32(lo);
        FPS_STAMP(2);  // wave reductions + index select
        if (W > 1) {
            // cross-wave: one LDS atomic max per wave on a rotating slot, one barrier, one broadcast read
            if (lane == 0) __hip_atomic_fetch_max(&slots[s_cur], ((unsigned long long)hi << 32) | wlo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (tid == 0) slots[s_nxt] = 0ull;
            __syncthreads();
            FPS_STAMP(3);  // LDS atomic + barrier
            wlo = (uint32_t)slots[s_cur];
            const int s_new = 3 - s_cur - s_nxt;
            s_cur = s_nxt;
            s_nxt = s_new;
        }
        old = (int)fps_unsec(~wlo, L);
        if (tid == 0) sidx[j] = old;
        FPS_STAMP(4);  // slot read + decode + store
    }
    __syncthreads();
    for (int j = tid; j < m; j += T) idxs[j] = sidx[j];
#pragma unroll
    for (int p = 0; p < P; ++p) {
        int k = tid + T * p;
        if (temp && k < n) temp[k] = pt[p];
    }
    fps_emit_points<T>(xyz, idxs, pts, m, tid);
}

// Large-N fallback (N > 16 points per lane at 1024 threads): temp stays in global memory,
// xyz is re-read from L2 each iteration, same (ord, ~sec) reduction.  Correct for any N.
__global__ __launch_bounds__(1024) void fps_stream_kernel(int n, int m, int L, const float *__restrict__ xyz,
                                                          float *__restrict__ temp, int *__restrict__ idxs, float *__restrict__ pts) {
    __shared__ uint2 slots[2][16];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    xyz += (size_t)blockIdx.x * n * 3;
    if (temp) temp += (size_t)blockIdx.x * n;  // NULL: a fresh sampling -- every running distance starts at 1e10 and is not stored
    idxs += (size_t)blockIdx.x * m;
    if (pts) pts += (size_t)blockIdx.x * m * 3;
    if (tid < 32) (&slots[0][0])[tid] = make_uint2(0u, 0u);
    if (tid == 0) idxs[0] = 0;
    __syncthreads();
    int old = 0;
    for (int j = 1; j < m; ++j) {
        float x1 = xyz[old * 3 + 0], y1 = xyz[old * 3 + 1], z1 = xyz[old * 3 + 2];
        uint32_t hi = 0, lo = 0;
        for (int k = tid; k < n; k += 1024) {
            float d = mcp_sqdist3(xyz[k * 3 + 0], xyz[k * 3 + 1], xyz[k * 3 + 2], x1, y1, z1);
            float d2 = fminf(d, temp[k]);
            temp[k] = d2;
            uint32_t h = mcp_ord(d2), s = ~fps_sec((uint32_t)k, L);
            bool gt = (h > hi) || (h == hi && s > lo);
            lo = gt ? s : lo;
            hi = gt ? h : hi;
        }
        uint32_t whi = mcp_wave_max_u32(hi);
        uint32_t wlo = mcp_wave_max_u32(hi == whi ? lo : 0u);
        uint2 *sl = slots[j & 1];
        if (lane == 0) sl[wave] = make_uint2(wlo, whi);
        __syncthreads();
        uint2 e = sl[lane & 15];
        uint32_t ghi = mcp_row_max_u32(e.y);
        uint32_t glo = mcp_row_max_u32(e.y == ghi ? e.x : 0u);
        wlo = __builtin_amdgcn_readfirstlane((int)glo);
        old = (int)fps_unsec(~wlo, L);
        if (tid == 0) idxs[j] = old;
    }
    fps_emit_points<1024>(xyz, idxs, pts, m, tid);
}

int ref_block_log2(int n) {
    // cuda_utils.h:10-14, same double arithmetic
    int pow_2 = (int)(log((double)n) / log(2.0));
    if (pow_2 > 10) pow_2 = 10;
    if (pow_2 < 0) pow_2 = 0;
    return pow_2;
}

template <int T, int P, int J, bool GENERIC>
int launch_resident(int b, int n, int m, int L, const float *xyz, float *temp, int *idx, float *pts, hipStream_t s) {
    const size_t slot_bytes = 64;
    const size_t xyz_bytes = (size_t)n * 3 * sizeof(float);
    const size_t idx_bytes = (size_t)(m > 0 ? m : 1) * sizeof(int);  // the selected indices are buffered in LDS (m <= n)
    if (xyz_bytes + slot_bytes + idx_bytes <= 150 * 1024) {
        constexpr auto kern = fps_resident_kernel<T, P, J, GENERIC, true>;
        if (const int rc = mcp_allow_lds<kern>()) return rc;
        hipLaunchKernelGGL(kern, dim3(b), dim3(T), slot_bytes + xyz_bytes + idx_bytes, s, n, m, L, xyz, temp, idx, pts);
    } else {
        if (slot_bytes + idx_bytes > 150 * 1024) return MCP_ERR_UNSUPPORTED;
        constexpr auto kern = fps_resident_kernel<T, P, J, GENERIC, false>;
        if (const int rc = mcp_allow_lds<kern>()) return rc;
        hipLaunchKernelGGL(kern, dim3(b), dim3(T), slot_bytes + idx_bytes, s, n, m, L, xyz, temp, idx, pts);
    }
    return mcp_launch_status();
}

// tuning hooks exist only in -DMCP_AB builds; the shipped library reads no environment variable
int env_int(const char *name, int dflt) {
#ifdef MCP_AB
    const char *v = getenv(name);
    return v && *v ? atoi(v) : dflt;
#else
    (void)name;
    return dflt;
#endif
}

// workgroup size for the spatial kernel by sort size (tuning override: MCP_FPS_T)
int launch_spatial_any(int b, int n, int m, int L, const float *xyz, float *temp, int *idx, float *pts, hipStream_t s) {
    static const int force_t = env_int("MCP_FPS_T", 0);
    int ns = 2048;
    while (ns < n) ns <<= 1;
    const int t = force_t ? force_t : 1024;
    switch (ns / t) {
        case 2: if (t == 1024) return launch_spatial<1024, 2>(b, n, m, L, xyz, temp, idx, pts, s); break;
        case 4:
            if (t == 1024) return launch_spatial<1024, 4>(b, n, m, L, xyz, temp, idx, pts, s);
            if (t == 512) return launch_spatial<512, 4>(b, n, m, L, xyz, temp, idx, pts, s);
            break;
        case 8:
            if (t == 1024) return launch_spatial<1024, 8>(b, n, m, L, xyz, temp, idx, pts, s);
            if (t == 512) return launch_spatial<512, 8>(b, n, m, L, xyz, temp, idx, pts, s);
            if (t == 256) return launch_spatial<256, 8>(b, n, m, L, xyz, temp, idx, pts, s);
            break;
        case 16:
            if (t == 1024) return launch_spatial<1024, 16>(b, n, m, L, xyz, temp, idx, pts, s);
            if (t == 512) return launch_spatial<512, 16>(b, n, m, L, xyz, temp, idx, pts, s);
            if (t == 256) return launch_spatial<256, 16>(b, n, m, L, xyz, temp, idx, pts, s);
            break;
        case 32:
            if (t == 512) return launch_spatial<512, 32>(b, n, m, L, xyz, temp, idx, pts, s);
            if (t == 256) return launch_spatial<256, 32>(b, n, m, L, xyz, temp, idx, pts, s);
            break;
    }
    return MCP_ERR_UNSUPPORTED;
}

}  // namespace

#ifdef MCP_FPS_DIAG
extern "C" __attribute__((visibility("default"))) int mcp_fps_diag_read(unsigned long long *out8) {
    hipError_t e = hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_fps_diag), sizeof(unsigned long long) * 8);
    unsigned long long z[8] = {0};
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_fps_diag), z, sizeof(z));
    return (int)e;
}
#endif

namespace {

int fps_dispatch(int b, int n, int m, const float *xyz, float *temp, int *idx, float *pts, char *ws, size_t ws_bytes, hipStream_t s) {
    const int L = ref_block_log2(n);
    const int bs = 1 << L;
    int rc;
    mcp_prof_begin(MCP_KERNEL_FPS, s);
    static const int spatial_min = env_int("MCP_FPS_SPATIAL_MIN", 1024);
    if (n >= spatial_min && L == 10 && n <= 16384 && m > 1) {
        rc = launch_spatial_any(b, n, m, L, xyz, temp, idx, pts, s);
    } else if (bs >= 64) {
        const int P = (n + bs - 1) / bs;
        if (bs == 1024) {
            // half-size workgroups (J = 1) from 4 points per reference thread up: fewer waves in the reduction
            if (P <= 1) rc = launch_resident<1024, 1, 0, false>(b, n, m, L, xyz, temp, idx, pts, s);
            else if (P <= 2) rc = launch_resident<1024, 2, 0, false>(b, n, m, L, xyz, temp, idx, pts, s);
            else if (P <= 4) rc = launch_resident<MCP_FPS_T4, MCP_FPS_P4, MCP_FPS_J4, false>(b, n, m, L, xyz, temp, idx, pts, s);
            else if (P <= 8) rc = launch_resident<MCP_FPS_T8, MCP_FPS_P8, MCP_FPS_J8, false>(b, n, m, L, xyz, temp, idx, pts, s);
            else if (P <= 16) rc = launch_resident<1024, 16, 0, false>(b, n, m, L, xyz, temp, idx, pts, s);
            else {
                // the tiled kernel needs scratch for the sorted cloud; without it (or beyond its range): plain streaming, any N
                rc = (tiled_range(n) && ws && ws_bytes >= tiled_workspace_bytes(b, n)) ? launch_tiled(b, n, m, xyz, temp, idx, pts, ws, s)
                                                                                      : MCP_ERR_UNSUPPORTED;
                if (rc == MCP_ERR_UNSUPPORTED && temp) {  // (the streaming kernel keeps its running distances IN temp)
                    hipLaunchKernelGGL(fps_stream_kernel, dim3(b), dim3(1024), 0, s, n, m, L, xyz, temp, idx, pts);
                    rc = mcp_launch_status();
                }
            }
        } else if (bs == 512) rc = launch_resident<512, 2, 0, false>(b, n, m, L, xyz, temp, idx, pts, s);
        else if (bs == 256) rc = launch_resident<256, 2, 0, false>(b, n, m, L, xyz, temp, idx, pts, s);
        else if (bs == 128) rc = launch_resident<128, 2, 0, false>(b, n, m, L, xyz, temp, idx, pts, s);
        else rc = launch_resident<64, 2, 0, false>(b, n, m, L, xyz, temp, idx, pts, s);
    } else {
        rc = launch_resident<64, 1, 0, true>(b, n, m, L, xyz, temp, idx, pts, s);  // n < 64
    }
    mcp_prof_end(MCP_KERNEL_FPS, s);
    return rc;
}
}  // namespace

MCP_EXPORT size_t mcp_fps_workspace_bytes(int b, int n, int m) {
    (void)m;
    return (b > 0 && tiled_range(n)) ? tiled_workspace_bytes(b, n) : 0;
}

MCP_EXPORT int mcp_furthest_point_sampling(int b, int n, int m, const float *xyz, float *temp, int *idx, mcp_stream_t stream) {
    MCP_CHECK_ARGS(b > 0 && n > 0 && xyz && temp && idx);
    if (m <= 0) return MCP_OK;  // sampling_gpu.cu:100
    return fps_dispatch(b, n, m, xyz, temp, idx, nullptr, nullptr, 0, (hipStream_t)stream);
}

MCP_EXPORT int mcp_furthest_point_sampling_ws(int b, int n, int m, const float *xyz, float *temp, int *idx, void *workspace,
                                              size_t workspace_bytes, mcp_stream_t stream) {
    MCP_CHECK_ARGS(b > 0 && n > 0 && xyz && temp && idx);
    if (m <= 0) return MCP_OK;
    return fps_dispatch(b, n, m, xyz, temp, idx, nullptr, static_cast<char *>(workspace), workspace_bytes, (hipStream_t)stream);
}

/* A fresh sampling (every call of the caller graph is one): the running distances start at 1e10 inside the kernel and are not
 * returned, so the caller neither fills nor allocates the (b,n) temp buffer of the reference interface; sampled_xyz (b,m,3),
 * optional, receives the coordinates of the selected points (the index_points_gather the callers run next, mocopci.py:1379).
 * Same indices as mcp_furthest_point_sampling_ws with temp = 1e10.  MCP_ERR_UNSUPPORTED where only the streaming kernel applies
 * (n > 65536, or 16384 < n <= 65536 without workspace): use the temp interface there. */
MCP_EXPORT int mcp_furthest_point_sampling_fresh(int b, int n, int m, const float *xyz, int *idx, float *sampled_xyz, void *workspace,
                                                 size_t workspace_bytes, mcp_stream_t stream) {
    MCP_CHECK_ARGS(b > 0 && n > 0 && xyz && idx);
    if (m <= 0) return MCP_OK;
    return fps_dispatch(b, n, m, xyz, nullptr, idx, sampled_xyz, static_cast<char *>(workspace), workspace_bytes, (hipStream_t)stream);
}
