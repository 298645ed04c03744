// fps_lengths.hip -- furthest point sampling over the valid prefixes of a padded batch (pytorch3d's
// sample_farthest_points(points, lengths, K)).  Element bb of xyz (B,N,3) is the cloud xyz[bb, :len[bb]]; rows at or beyond the
// length are never read.  fps.hip is not touched by this file: without lengths the entry point below IS
// mcp_furthest_point_sampling_fresh.
//
// One tie key for every length.  The reference's tie rule depends on its block size bs = 2^L, L = min(10, floor(log2 n)): among
// equal distances the winner minimises (bitrev_L(k mod bs), k div bs) (fps.hip:11-17), and with per-element lengths L would differ
// per element.  But for n < 1024 every k < 2^(L+1), so that key orders the points exactly as bitrev_(L+1)(k) does, which orders
// them exactly as bitrev_10(k) does; and for n >= 1024, L is 10.  So the L = 10 key, (bitrev_10(k mod 1024), k div 1024), is the
// reference's order for every length, and a length only decides which points take part.
//
// Four forms, chosen from the PADDED shape and the workspace size alone (mcp_fps_lengths_form; the host never reads a length):
//   resident  (n < 1024, or m <= 1 up to n = 16384; everything up to 16384 in the unpruned entry point): one 1024-thread workgroup
//             per element; thread t keeps points t, t + 1024, ... and their running distances in registers for the whole call
//             (register slice p = points [1024 p, 1024 p + 1024)), as fps_resident_kernel does.  A thread is one reference thread of
//             the 1024-thread block, so inside a thread ties go to the lowest p.  Points at k >= len start at -INFINITY (never
//             selected); slices that lie wholly beyond the length are skipped by a scalar test, and so are the waves of slice 0 that
//             hold no point, so a short element does less vector work.
//   spatial   (1024 <= n <= 16384, m > 1) and
//   tiled     (16384 < n <= 65536 with the tiled workspace): the Morton-sorted, box-pruned kernels of fps_pruned.h under FPS_LEN 1.
//   streaming (n > 16384 otherwise): a streaming kernel bounded by the length, its running distances in the caller's workspace.
#include <math.h>

#include "common.h"

namespace {

constexpr int LT = 1024;  // workgroup size of every kernel here = the reference block at L = 10

__device__ __forceinline__ uint32_t len_sec(uint32_t k) { return (__brev(k & 1023u) & 0xFFC00000u) | (k >> 10); }
__device__ __forceinline__ uint32_t len_unsec(uint32_t sec) { return __brev(sec & 0xFFC00000u) | ((sec & 0x3FFFFFu) << 10); }

// the element's length as the kernels use it: clamped to [0, n], wave-uniform (a scalar load)
__device__ __forceinline__ int len_clamped(const int *__restrict__ len, int n) {
    const int l = len[blockIdx.x];
    return l < 0 ? 0 : (l > n ? n : l);
}

// an empty element: index row 0, coordinate row 0.0
__device__ __forceinline__ void len_emit_empty(int *__restrict__ idxs, float *__restrict__ pts, int m, int tid) {
    for (int i = tid; i < m; i += LT) idxs[i] = 0;
    if (pts)
        for (int i = tid; i < m * 3; i += LT) pts[i] = 0.0f;
}

}  // namespace

// the pruned kernels in their length forms (fps_len_spatial_kernel, fps_len_tiled_kernel); they use the three names above
#define FPS_LEN 1
#include "fps_pruned.h"

namespace {

// optional last step: the coordinates of the selected points (fps_emit_points of fps_pruned.h); every index is below the length
__device__ __forceinline__ void len_emit_points(const float *__restrict__ xyz, const int *idxs, float *__restrict__ pts, int m, int tid) {
    if (!pts) return;
    __syncthreads();
    for (int i = tid; i < m * 3; i += LT) {
        const int j = i / 3;
        pts[i] = xyz[idxs[j] * 3 + (i - j * 3)];
    }
}

template <int P, bool LDS_XYZ>
__global__ __launch_bounds__(LT) void fps_lengths_resident_kernel(int n, int m, const float *__restrict__ xyz, const int *__restrict__ len,
                                                                  int *__restrict__ idxs, float *__restrict__ pts) {
    extern __shared__ float4 smem_f4[];
    unsigned long long *slots = reinterpret_cast<unsigned long long *>(smem_f4);  // [3] rotating max slots (+pad to 64 B)
    float *sxyz = reinterpret_cast<float *>(smem_f4) + 16;                        // [n*3] when LDS_XYZ (the first l*3 are filled)
    int *sidx = reinterpret_cast<int *>(sxyz + (LDS_XYZ ? n * 3 : 0));            // [m] selected indices, written out once at the end

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l = len_clamped(len, n);
    xyz += (size_t)blockIdx.x * n * 3;
    idxs += (size_t)blockIdx.x * m;
    if (pts) pts += (size_t)blockIdx.x * m * 3;
    if (l == 0) {  // the whole workgroup leaves before the first barrier; nothing of xyz is read
        len_emit_empty(idxs, pts, m, tid);
        return;
    }
    const bool wave_live = wave * 64 < l;  // a wave beyond the length holds no point in any slice (then l < 1024)

    float px[P], py[P], pz[P], pt[P];
    uint32_t nsec[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
        px[p] = 0.0f; py[p] = 0.0f; pz[p] = 0.0f;
        pt[p] = -INFINITY;  // padding: never selected
        nsec[p] = 0u;
        if (LT * p < l) {   // a slice wholly beyond the length loads nothing
            const int k = tid + LT * p;
            if (k < l) {
                px[p] = xyz[k * 3 + 0];
                py[p] = xyz[k * 3 + 1];
                pz[p] = xyz[k * 3 + 2];
                pt[p] = 1e10f;
                nsec[p] = ~len_sec((uint32_t)k);
            }
        }
    }
    if (LDS_XYZ) {
        for (int i = tid; i < l * 3; i += LT) sxyz[i] = xyz[i];
    }
    if (tid < 3) slots[tid] = 0ull;
    if (tid == 0) sidx[0] = 0;
    __syncthreads();

    int old = 0;
    int s_cur = 0, s_nxt = 1;
    for (int j = 1; j < m; ++j) {
        float x1, y1, z1;
        if (LDS_XYZ) {
            x1 = sxyz[old * 3 + 0]; y1 = sxyz[old * 3 + 1]; z1 = sxyz[old * 3 + 2];
        } else {
            x1 = xyz[old * 3 + 0]; y1 = xyz[old * 3 + 1]; z1 = xyz[old * 3 + 2];
        }
        uint32_t hi = 0, wlo = 0;
        if (wave_live) {
            // the maximum VALUE first (distances in the canon of common.h), then which point holds it
            float best = -1.0f;
#pragma unroll
            for (int p = 0; p < P; ++p) {
                if (LT * p < l) {
                    pt[p] = mcp_min_raw(mcp_sqdist3(px[p], py[p], pz[p], x1, y1, z1), pt[p]);  // nothing here is ever NaN
                    best = mcp_max_raw(best, pt[p]);
                }
            }
            hi = mcp_ord(best);
            const uint32_t whi = mcp_wave_max_u32(hi);
            uint32_t bsec = 0;  // ties inside the thread go to the lowest p: assigned last
#pragma unroll
            for (int p = P - 1; p >= 0; --p) {
                if (LT * p < l) bsec = pt[p] == best ? nsec[p] : bsec;
            }
            wlo = mcp_wave_max_u32(hi == whi ? bsec : 0u);
            hi = whi;
        }
        // cross-wave: one LDS atomic max per live wave on a rotating slot, one barrier, one broadcast read
        if (lane == 0 && wave_live)
            __hip_atomic_fetch_max(&slots[s_cur], ((unsigned long long)hi << 32) | wlo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (tid == 0) slots[s_nxt] = 0ull;
        __syncthreads();
        wlo = (uint32_t)slots[s_cur];
        const int s_new = 3 - s_cur - s_nxt;
        s_cur = s_nxt;
        s_nxt = s_new;
        old = (int)len_unsec(~wlo);
        if (tid == 0) sidx[j] = old;
    }
    __syncthreads();
    for (int j = tid; j < m; j += LT) idxs[j] = sidx[j];
    len_emit_points(xyz, idxs, pts, m, tid);
}

// n > 16384: the running distances live in the caller's workspace ((b,n) floats, first written in iteration 1), the points are
// re-read from L2 on every iteration, and every loop stops at the length.
__global__ __launch_bounds__(LT) void fps_lengths_stream_kernel(int n, int m, const float *__restrict__ xyz, const int *__restrict__ len,
                                                                float *__restrict__ temp, int *__restrict__ idxs, float *__restrict__ pts) {
    __shared__ uint2 slots[2][16];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int l = len_clamped(len, n);
    xyz += (size_t)blockIdx.x * n * 3;
    temp += (size_t)blockIdx.x * n;
    idxs += (size_t)blockIdx.x * m;
    if (pts) pts += (size_t)blockIdx.x * m * 3;
    if (l == 0) {
        len_emit_empty(idxs, pts, m, tid);
        return;
    }
    if (tid < 32) (&slots[0][0])[tid] = make_uint2(0u, 0u);
    if (tid == 0) idxs[0] = 0;
    __syncthreads();
    int old = 0;
    for (int j = 1; j < m; ++j) {
        const float x1 = xyz[old * 3 + 0], y1 = xyz[old * 3 + 1], z1 = xyz[old * 3 + 2];
        uint32_t hi = 0, lo = 0;
        for (int k = tid; k < l; k += LT) {  // a thread only ever touches its own temp entries
            const float d = mcp_sqdist3(xyz[k * 3 + 0], xyz[k * 3 + 1], xyz[k * 3 + 2], x1, y1, z1);
            const float d2 = fminf(d, j == 1 ? 1e10f : temp[k]);
            temp[k] = d2;
            const uint32_t h = mcp_ord(d2), s = ~len_sec((uint32_t)k);
            const bool gt = (h > hi) || (h == hi && s > lo);
            lo = gt ? s : lo;
            hi = gt ? h : hi;
        }
        const uint32_t whi = mcp_wave_max_u32(hi);
        uint32_t wlo = mcp_wave_max_u32(hi == whi ? lo : 0u);
        uint2 *sl = slots[j & 1];
        if (lane == 0) sl[wave] = make_uint2(wlo, whi);
        __syncthreads();
        const uint2 e = sl[lane & 15];
        const uint32_t ghi = mcp_row_max_u32(e.y);
        const uint32_t glo = mcp_row_max_u32(e.y == ghi ? e.x : 0u);
        wlo = __builtin_amdgcn_readfirstlane((int)glo);
        old = (int)len_unsec(~wlo);
        if (tid == 0) idxs[j] = old;
    }
    len_emit_points(xyz, idxs, pts, m, tid);
}

constexpr int LEN_RESIDENT_MAX = 16 * LT;  // 16 points per thread

template <int P>
int launch_resident(int b, int n, int m, const float *xyz, const int *len, int *idx, float *pts, hipStream_t s) {
    const size_t slot_bytes = 64;
    const size_t xyz_bytes = (size_t)n * 3 * sizeof(float);
    const size_t idx_bytes = (size_t)m * sizeof(int);  // the selected indices are buffered in LDS
    const bool lds_xyz = xyz_bytes + slot_bytes + idx_bytes <= 150 * 1024;
    if (!lds_xyz && slot_bytes + idx_bytes > 150 * 1024) return MCP_ERR_UNSUPPORTED;
    if (const int rc = mcp_allow_lds<fps_lengths_resident_kernel<P, true>>()) return rc;
    if (const int rc = mcp_allow_lds<fps_lengths_resident_kernel<P, false>>()) return rc;
    if (lds_xyz) hipLaunchKernelGGL((fps_lengths_resident_kernel<P, true>), dim3(b), dim3(LT), slot_bytes + xyz_bytes + idx_bytes, s, n, m, xyz, len, idx, pts);
    else hipLaunchKernelGGL((fps_lengths_resident_kernel<P, false>), dim3(b), dim3(LT), slot_bytes + idx_bytes, s, n, m, xyz, len, idx, pts);
    return mcp_launch_status();
}

size_t stream_workspace_bytes(int b, int n) { return (size_t)b * (size_t)n * sizeof(float); }

// the spatial kernel's points per thread by the padded n (a 1024-thread workgroup sorts 1024 P >= n keys, P >= 2)
int launch_spatial_len(int b, int n, int m, const float *xyz, const int *len, int *idx, float *pts, hipStream_t s) {
    if (n <= 2 * LT) return launch_spatial<LT, 2>(b, n, m, 10, xyz, len, idx, pts, s);
    if (n <= 4 * LT) return launch_spatial<LT, 4>(b, n, m, 10, xyz, len, idx, pts, s);
    if (n <= 8 * LT) return launch_spatial<LT, 8>(b, n, m, 10, xyz, len, idx, pts, s);
    return launch_spatial<LT, 16>(b, n, m, 10, xyz, len, idx, pts, s);
}

// the form the unpruned dispatch takes (resident / streaming), and the one the pruned dispatch takes: pure functions of the padded
// shape and the workspace size
int unpruned_form(int b, int n, size_t ws_bytes) {
    if (n <= LEN_RESIDENT_MAX) return MCP_FPS_LENGTHS_RESIDENT;
    return ws_bytes >= stream_workspace_bytes(b, n) ? MCP_FPS_LENGTHS_STREAMING : MCP_ERR_UNSUPPORTED;
}

int pruned_form(int b, int n, int m, size_t ws_bytes) {
    if (n <= LEN_RESIDENT_MAX) return n >= LT && m > 1 ? MCP_FPS_LENGTHS_SPATIAL : MCP_FPS_LENGTHS_RESIDENT;
    if (tiled_range(n) && ws_bytes >= tiled_workspace_bytes(b, n)) return MCP_FPS_LENGTHS_TILED;
    return unpruned_form(b, n, ws_bytes);
}

int dispatch(int form, int b, int n, int m, const float *xyz, const int *len, int *idx, float *pts, void *ws, hipStream_t s) {
    if (form < 0 || form > MCP_FPS_LENGTHS_STREAMING) return form;  // MCP_ERR_UNSUPPORTED: nothing is launched
    int rc;
    mcp_prof_begin(MCP_KERNEL_FPS, s);
    if (form == MCP_FPS_LENGTHS_SPATIAL) rc = launch_spatial_len(b, n, m, xyz, len, idx, pts, s);
    else if (form == MCP_FPS_LENGTHS_TILED) rc = launch_tiled(b, n, m, xyz, len, idx, pts, static_cast<char *>(ws), s);
    else if (form == MCP_FPS_LENGTHS_STREAMING) {
        hipLaunchKernelGGL(fps_lengths_stream_kernel, dim3(b), dim3(LT), 0, s, n, m, xyz, len, static_cast<float *>(ws), idx, pts);
        rc = mcp_launch_status();
    } else if (n <= LT) rc = launch_resident<1>(b, n, m, xyz, len, idx, pts, s);
    else if (n <= 2 * LT) rc = launch_resident<2>(b, n, m, xyz, len, idx, pts, s);
    else if (n <= 4 * LT) rc = launch_resident<4>(b, n, m, xyz, len, idx, pts, s);
    else if (n <= 8 * LT) rc = launch_resident<8>(b, n, m, xyz, len, idx, pts, s);
    else rc = launch_resident<16>(b, n, m, xyz, len, idx, pts, s);
    mcp_prof_end(MCP_KERNEL_FPS, s);
    return rc;
}

}  // namespace

MCP_EXPORT size_t mcp_fps_lengths_workspace_bytes(int b, int n, int m) {
    (void)m;
    return (b > 0 && n > LEN_RESIDENT_MAX) ? stream_workspace_bytes(b, n) : 0;
}

MCP_EXPORT size_t mcp_fps_lengths_pruned_workspace_bytes(int b, int n, int m) {
    return (b > 0 && tiled_range(n)) ? tiled_workspace_bytes(b, n) : mcp_fps_lengths_workspace_bytes(b, n, m);
}

MCP_EXPORT int mcp_fps_lengths_form(int b, int n, int m, size_t workspace_bytes) {
    MCP_CHECK_ARGS(b > 0 && n > 0);
    return pruned_form(b, n, m, workspace_bytes);
}

MCP_EXPORT int mcp_furthest_point_sampling_lengths(int b, int n, int m, const float *xyz, const int *len, int *idx, float *sampled_xyz,
                                                   void *workspace, size_t workspace_bytes, mcp_stream_t stream) {
    MCP_CHECK_ARGS(b > 0 && n > 0 && xyz && idx);
    if (m <= 0) return MCP_OK;
    if (!len) return mcp_furthest_point_sampling_fresh(b, n, m, xyz, idx, sampled_xyz, workspace, workspace_bytes, stream);
    return dispatch(mcp_fps_lengths_form(b, n, m, workspace ? workspace_bytes : 0), b, n, m, xyz, len, idx, sampled_xyz, workspace,
                    (hipStream_t)stream);
}

MCP_EXPORT int mcp_furthest_point_sampling_lengths_unpruned(int b, int n, int m, const float *xyz, const int *len, int *idx,
                                                            float *sampled_xyz, void *workspace, size_t workspace_bytes, mcp_stream_t stream) {
    MCP_CHECK_ARGS(b > 0 && n > 0 && xyz && idx);
    if (m <= 0) return MCP_OK;
    if (!len) return mcp_furthest_point_sampling_fresh(b, n, m, xyz, idx, sampled_xyz, workspace, workspace_bytes, stream);
    return dispatch(unpruned_form(b, n, workspace ? workspace_bytes : 0), b, n, m, xyz, len, idx, sampled_xyz, workspace, (hipStream_t)stream);
}
