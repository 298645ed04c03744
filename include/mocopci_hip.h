/*
 * mocopci_hip.h -- C ABI of libmocopci_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for the point-set hot path of icdm-adteam/MoCoPCI.
 * Part 1 replaces, one for one, the nine functions the reference registers in its
 * pybind11 module `pointnet2_cuda` (pointnet2/src/pointnet2_api.cpp:10-24); the
 * integer argument order of every entry point is the reference wrapper's.
 * Part 2 is the Python-level second boundary (knn_point, index_points_group,
 * UpsampleFlow, ... in models/pointconv_util.py and models/m_models/mocopci.py)
 * expressed as fused kernels.
 *
 * Conventions (same contract as the reference extension):
 *   - all pointers are DEVICE pointers into contiguous fp32 / int32 buffers owned by
 *     the caller; the library never allocates or frees, reads no environment variable, and keeps no
 *     state between calls except two per-process conveniences: the per-device "kernel attribute set"
 *     flags (marked after the attribute call) and the opt-in launch timers of mcp_prof_*;
 *   - every call is enqueued asynchronously on `stream` (a hipStream_t passed as
 *     void*; NULL = the null stream) and returns without synchronising;
 *   - re-entrant and thread-safe; the device is the calling thread's current device;
 *   - return value: 0 on success, otherwise a hipError_t value (launch failure) or
 *     MCP_ERR_* (argument validation).  The reference calls exit(-1) on launch
 *     failure (pointnet2/src/sampling_gpu.cu:248-252); this library never exits.
 */
#ifndef MOCOPCI_HIP_H
#define MOCOPCI_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *mcp_stream_t; /* hipStream_t */

#define MCP_OK 0
#define MCP_ERR_BAD_ARG 10001     /* null pointer, non-positive dimension */
#define MCP_ERR_UNSUPPORTED 10002 /* a size outside what the kernels are built for (e.g. K > 32) */

#define MCP_ABI_VERSION 1

int mcp_abi_version(void);
/* Static string for a code returned by any mcp_* call. */
const char *mcp_error_string(int code);

/* ---------------- Part 1: pointnet2_cuda replacements ------------------------------ */

/* furthest_point_sampling_wrapper(b,n,m,points,temp,idx)   pointnet2/src/sampling.cpp:38-49,
 * kernel sampling_gpu.cu:93-253.  xyz (B,N,3); temp (B,N) scratch pre-filled with 1e10 by the
 * caller (pointnet2_utils.py:26), holds the final min-distances on return; idx (B,M) int32.
 * Bit-exact with the reference kernel's index sequence including its tie rule.
 * No memory beyond the arguments is used.  For 16384 < N <= 65536 the fast (tiled, spatially pruned) kernel needs scratch
 * for a sorted copy of the cloud: pass it through mcp_furthest_point_sampling_ws; this entry point, which keeps the reference
 * wrapper's exact argument list, then runs the plain streaming kernel (same indices, ~9x slower at 8 x 65536 -> 2048). */
int mcp_furthest_point_sampling(int b, int n, int m, const float *xyz, float *temp, int *idx, mcp_stream_t stream);

/* Same operation with caller-provided scratch (any workspace is a caller pointer + a size query).
 * mcp_fps_workspace_bytes returns how many bytes this (b, n, m) can use -- 0 when the size needs none -- and
 * mcp_furthest_point_sampling_ws takes a device buffer of at least that size (NULL / too small: behaves like
 * mcp_furthest_point_sampling).  The buffer is only used during the call (stream-ordered). */
size_t mcp_fps_workspace_bytes(int b, int n, int m);
int mcp_furthest_point_sampling_ws(int b, int n, int m, const float *xyz, float *temp, int *idx, void *workspace,
                                   size_t workspace_bytes, mcp_stream_t stream);

/* The same sampling for a fresh start (temp = 1e10 everywhere, which is what every caller of the reference passes:
 * pointnet2_utils.py:24): the running distances live and die in the kernel, so no (b,n) buffer is filled or allocated.
 * sampled_xyz (b,m,3), optional (NULL to skip): the coordinates of the selected points -- the index_points_gather the callers
 * run next (mocopci.py:1378-1379) -- written by the same launch.
 * MCP_ERR_UNSUPPORTED where only the streaming kernel applies (n > 65536, or 16384 < n <= 65536 without workspace). */
int mcp_furthest_point_sampling_fresh(int b, int n, int m, const float *xyz, int *idx, float *sampled_xyz, void *workspace,
                                      size_t workspace_bytes, mcp_stream_t stream);

/* A fresh sampling of a padded batch of clouds of different sizes (pytorch3d.ops.sample_farthest_points' lengths): len (B) is an
 * int32 DEVICE array, read by the kernel with no host synchronisation and clamped there to [0, n].  len == NULL: the call IS
 * mcp_furthest_point_sampling_fresh (same dispatch, same launch, same bits; workspace as described there).  Otherwise, per
 * element bb with l = len[bb]:
 *   l >= 1:  idx[bb, 0..m-1] is bit for bit what mcp_furthest_point_sampling returns for the cloud xyz[bb, :l] alone with the same
 *            m and temp = 1e10, including m > l, where the reference simply keeps selecting; sampled_xyz[bb, j] = xyz[bb, idx[bb, j]]
 *            for every j (sampled_xyz (b,m,3) is optional: NULL to skip);
 *   l == 0:  the idx row is all 0 and the sampled_xyz row is all 0.0;
 *   rows at or beyond l are never read: their contents reach no output bit.
 * The tie rule needs no per-element block size: the reference's order for a cloud of ANY length is the one of its 1024-thread block,
 * (bitrev_10(k mod 1024), k div 1024) (csrc/fps_lengths.hip).
 * Four kernel forms give those same bits; which one runs is a pure function of the PADDED shape and the workspace size
 * (mcp_fps_lengths_form; no length is read by the host):
 *   n < 1024, or m <= 1 (n <= 16384)    resident: one workgroup per element, points and running distances in registers, register
 *                                       slices and waves wholly beyond l skipped; no workspace
 *   1024 <= n <= 16384, m > 1           spatial: the Morton-sorted, box-pruned kernel of the length-free call over the l live
 *                                       points; no workspace
 *   16384 < n <= 65536                  tiled (the length-free call's tiled kernel over ceil(l / 64) live tiles) when workspace_bytes
 *                                       >= mcp_fps_lengths_pruned_workspace_bytes (20 bytes per point of the cloud padded to 64, the
 *                                       figure of mcp_fps_workspace_bytes); else streaming (bounded by l, running distances in the
 *                                       workspace) when workspace_bytes >= mcp_fps_lengths_workspace_bytes = b*n*4; else
 *                                       MCP_ERR_UNSUPPORTED, as with a NULL workspace: nothing is launched
 *   n > 65536                           streaming, workspace b*n*4 as above
 * mcp_fps_lengths_workspace_bytes is the least a call needs (0 for n <= 16384), mcp_fps_lengths_pruned_workspace_bytes what the
 * fastest form uses (the same value outside 16384 < n <= 65536).  The buffer is only used during the call (stream-ordered) and needs
 * no initialisation.
 * mcp_fps_lengths_form: host only, launches nothing; the form (MCP_FPS_LENGTHS_*) a call of mcp_furthest_point_sampling_lengths with a
 * non-NULL len and a non-NULL workspace of that size takes, or MCP_ERR_UNSUPPORTED.  The call dispatches through this function.
 * mcp_furthest_point_sampling_lengths_unpruned: the same arguments and results from the resident (n <= 16384) and streaming forms
 * alone -- the cross-check of the pruned forms and their timing baseline (tools/fps_lengths_times.py).
 * Error codes as for the length-free calls (MCP_ERR_BAD_ARG: b <= 0, n <= 0, NULL xyz or idx; nothing is launched); m <= 0
 * returns MCP_OK. */
#define MCP_FPS_LENGTHS_RESIDENT 0
#define MCP_FPS_LENGTHS_SPATIAL 1
#define MCP_FPS_LENGTHS_TILED 2
#define MCP_FPS_LENGTHS_STREAMING 3
size_t mcp_fps_lengths_workspace_bytes(int b, int n, int m);
size_t mcp_fps_lengths_pruned_workspace_bytes(int b, int n, int m);
int mcp_fps_lengths_form(int b, int n, int m, size_t workspace_bytes);
int mcp_furthest_point_sampling_lengths(int b, int n, int m, const float *xyz, const int *len, int *idx, float *sampled_xyz,
                                        void *workspace, size_t workspace_bytes, mcp_stream_t stream);
int mcp_furthest_point_sampling_lengths_unpruned(int b, int n, int m, const float *xyz, const int *len, int *idx, float *sampled_xyz,
                                                 void *workspace, size_t workspace_bytes, mcp_stream_t stream);

/* gather_points_wrapper(b,c,n,npoints,points,idx,out)     sampling.cpp:11-22, sampling_gpu.cu:8-44
 * points (B,C,N), idx (B,npoints) -> out (B,C,npoints). */
int mcp_gather_points(int b, int c, int n, int npoints, const float *points, const int *idx, float *out, mcp_stream_t stream);

/* gather_points_grad_wrapper(b,c,n,npoints,grad_out,idx,grad_points)  sampling.cpp:25-35,
 * sampling_gpu.cu:46-83.  grad_points (B,C,N) must be zeroed by the caller (pointnet2_utils.py:67). */
int mcp_gather_points_grad(int b, int c, int n, int npoints, const float *grad_out, const int *idx, float *grad_points,
                           mcp_stream_t stream);

/* group_points_wrapper(b,c,n,npoints,nsample,points,idx,out)  group_points.cpp:26-37,
 * group_points_gpu.cu:47-86.  points (B,C,N), idx (B,npoints,nsample) -> out (B,C,npoints,nsample). */
int mcp_group_points(int b, int c, int n, int npoints, int nsample, const float *points, const int *idx, float *out,
                     mcp_stream_t stream);

/* group_points_grad_wrapper(b,c,n,npoints,nsample,grad_out,idx,grad_points)  group_points.cpp:11-23,
 * group_points_gpu.cu:8-44.  grad_points pre-zeroed by the caller (pointnet2_utils.py:190). */
int mcp_group_points_grad(int b, int c, int n, int npoints, int nsample, const float *grad_out, const int *idx,
                          float *grad_points, mcp_stream_t stream);

/* Deterministic forms of the three scatter-add backwards (the reference's kernels -- and the three *_grad entry
 * points above and below, which keep its exact argument lists -- use atomicAdd: sampling_gpu.cu:46-83, group_points_gpu.cu:8-44,
 * interpolate_gpu.cu:120-161).  The caller passes, per batch element, the stable sort of the T scatter positions by destination:
 * order (B,T) int32 = positions in sorted order, seg (B,N+1) int32 = CSR offsets of each destination in it.  Each destination's
 * addends are summed in ascending position order (a sequential loop's order): the same bits on every run; grad_points needs no
 * zero-fill.
 *   mcp_group_points_grad_sorted: grad_out (B,C,T) -> grad_points (B,C,N).  K6 with T = npoints*nsample, K3 with T = npoints.
 *   mcp_three_interpolate_grad_sorted: grad_out (B,C,n), weight (B,n,3), positions t = 3*p + k of idx (B,n,3) sorted by idx value
 *     (order (B,3n), seg (B,m+1)) -> grad_points (B,C,m). */
int mcp_group_points_grad_sorted(int b, int c, int n, int t, const float *grad_out, const int *order, const int *seg,
                                 float *grad_points, mcp_stream_t stream);
int mcp_three_interpolate_grad_sorted(int b, int c, int n, int m, const float *grad_out, const int *order, const int *seg,
                                      const float *weight, float *grad_points, mcp_stream_t stream);

/* ball_query_wrapper(b,n,m,radius,nsample,new_xyz,xyz,idx)   ball_query.cpp:16-28, ball_query_gpu.cu:9-67
 * new_xyz (B,M,3) centres, xyz (B,N,3) -> idx (B,M,nsample), pre-zeroed by the caller
 * (pointnet2_utils.py:218): first nsample hits in index order, padded with the first hit. */
int mcp_ball_query(int b, int n, int m, float radius, int nsample, const float *new_xyz, const float *xyz, int *idx,
                   mcp_stream_t stream);

/* QueryAndGroup.forward as one launch                         pointnet2/pointnet2_utils.py:231-264
 * (= ball_query_wrapper + a transposed copy of xyz + 2 x group_points_wrapper + subtraction + cat in the reference).
 * xyz (B,N,3), new_xyz (B,M,3) centres, features (B,C,N) or NULL -> out (B, CT, M, nsample), CT = (use_xyz or no features ? 3 : 0) +
 * (features ? C : 0): channels 0..2 = neighbour coordinates relative to the centre, then the grouped feature channels; neighbours =
 * the first nsample points within `radius` in index order, padded with the first hit; a centre with no hit groups point 0
 * (the reference's pre-zeroed idx).  nsample <= 64 (MCP_ERR_UNSUPPORTED above); features NULL needs use_xyz. */
int mcp_query_and_group(int b, int n, int m, int c, float radius, int nsample, int use_xyz, const float *xyz, const float *new_xyz,
                        const float *features, float *out, mcp_stream_t stream);

/* Ball query on a padded batch of clouds of different sizes.  qlen, rlen: (B) int32 DEVICE arrays, read by the kernels and clamped
 * there to [0,M] / [0,N]; either may be NULL = every row live.  One result definition for the three entry points, with
 * rl = clamp(rlen[bb]), ql = clamp(qlen[bb]):
 *   live centres (p < ql):    the first nsample indices k < rl, ascending, with d2(centre, xyz[bb,k]) < radius*radius (the float
 *                             expression and host-side radius*radius of mcp_ball_query); slots beyond the hit count hold the first
 *                             hit; no hit, or rl == 0: zeros.  Bit for bit what mcp_ball_query returns for xyz[bb,:rl] and
 *                             new_xyz[bb,:ql] alone on a pre-zeroed idx;
 *   padded centres (p >= ql): zeros;
 *   cnt (B,M) int32, may be NULL: min(hits, nsample) for live centres, 0 for padded ones -- what tells a row of zeros
 *                             "no hit" from "only point 0 hit".
 * Every slot of idx and cnt is written (no pre-zeroing by the caller); no row at or beyond a length -- of xyz, new_xyz, features, a
 * sorted cloud, its perm or its boxes -- is read.  An argument error launches nothing.
 *   mcp_ball_query_lengths:      any nsample.
 *   mcp_query_and_group_lengths: mcp_query_and_group on the two prefixes for live centres (nsample <= 64; a live centre with no hit
 *                                groups point 0, which is live since rl > 0); padded centres, and every centre of an element
 *                                with rl == 0, write zeros to all their output channels.
 *   mcp_ball_query_pruned:       the idx and cnt of mcp_ball_query_lengths, bit for bit, from a Morton-sorted cloud with tile boxes
 *                                (ref_sorted, rperm, boxes: mcp_build_cloud / mcp_morton_codes + sort + mcp_tile_boxes below, or
 *                                their _lengths forms under the same rlen), reading only the tiles whose box the ball reaches.
 *                                Centres in the caller's order.  nsample <= 64 and N <= 65536 (MCP_ERR_UNSUPPORTED above). */
int mcp_ball_query_lengths(int b, int n, int m, float radius, int nsample, const float *new_xyz, const float *xyz, const int *qlen,
                           const int *rlen, int *idx, int *cnt, mcp_stream_t stream);
int mcp_query_and_group_lengths(int b, int n, int m, int c, float radius, int nsample, int use_xyz, const float *xyz,
                                const float *new_xyz, const float *features, const int *rlen, const int *qlen, float *out,
                                mcp_stream_t stream);
int mcp_ball_query_pruned(int b, int n, int m, float radius, int nsample, const float *new_xyz, const float *ref_sorted,
                          const int *rperm, const float *boxes, const int *qlen, const int *rlen, int *idx, int *cnt,
                          mcp_stream_t stream);

/* three_nn_wrapper(b,n,m,unknown,known,dist2,idx)            interpolate.cpp:14-24, interpolate_gpu.cu:9-74
 * unknown (B,n,3), known (B,m,3) -> dist2 (B,n,3) SQUARED distances, idx (B,n,3). */
int mcp_three_nn(int b, int n, int m, const float *unknown, const float *known, float *dist2, int *idx, mcp_stream_t stream);

/* three_interpolate_wrapper(b,c,m,n,points,idx,weight,out)   interpolate.cpp:27-39, interpolate_gpu.cu:77-117
 * points (B,C,M), idx/weight (B,n,3) -> out (B,C,n). */
int mcp_three_interpolate(int b, int c, int m, int n, const float *points, const int *idx, const float *weight, float *out,
                          mcp_stream_t stream);

/* three_interpolate_grad_wrapper(b,c,n,m,grad_out,idx,weight,grad_points)  interpolate.cpp:42-56,
 * interpolate_gpu.cu:120-161.  grad_points (B,C,M) pre-zeroed by the caller (pointnet2_utils.py:146). */
int mcp_three_interpolate_grad(int b, int c, int n, int m, const float *grad_out, const int *idx, const float *weight,
                               float *grad_points, mcp_stream_t stream);

/* ---------------- Part 2: fused layer operators ------------------------------------ */

/* Distance forms for mcp_knn. */
#define MCP_DIST_EXPANSION 0 /* -2 q.r + |q|^2 + |r|^2 : square_distance, mocopci.py:1130-1155 */
#define MCP_DIST_DIRECT 1    /* sum (q-r)^2 : pytorch3d.ops.knn_points (pointconv_util.py:910) */

/* knn_point(nsample, xyz, new_xyz) (mocopci.py:1158-1169 = pointconv_util.py:129-140) and
 * pytorch3d.ops.knn_points(p1,p2,K) fused: never materialises the (B,Q,N) distance matrix.
 * query (B,Q,3), ref (B,N,3) -> idx (B,Q,K) int32 and, if dist != NULL, dist (B,Q,K):
 * the K smallest under the lexicographic order (distance, index), ascending.  1 <= K <= 32.
 * If N < K the tail repeats the last valid entry. */
int mcp_knn(int b, int q, int n, int k, int dist_form, const float *query, const float *ref, int *idx, float *dist,
            mcp_stream_t stream);

/* mcp_knn on a padded batch of clouds of different sizes (pytorch3d.ops.knn_points' lengths1 / lengths2): element bb searches
 * only the first rlen[bb] rows of ref and only its first qlen[bb] query rows are live.  qlen, rlen: (B) int32 DEVICE arrays,
 * read by the kernel (no synchronisation) and clamped there to [0,Q] / [0,N]; either may be NULL = every row valid, and with
 * both NULL the call IS mcp_knn (same launch, same bits).  Same distance forms, 1 <= K <= 32, any N.
 *   live rows (i < qlen[bb]):    the K smallest under (distance, index) among references 0 .. rlen[bb]-1, ascending -- what
 *                                mcp_knn returns for the two valid prefixes on their own; if rlen[bb] < K the tail repeats the
 *                                last valid entry; if rlen[bb] == 0, index 0 and distance 0;
 *   padded rows (i >= qlen[bb]): index 0, distance 0.
 * Rows beyond a length are never read: their contents influence no output bit.  Errors as mcp_knn (nothing is launched). */
int mcp_knn_lengths(int b, int q, int n, int k, int dist_form, const float *query, const float *ref, const int *qlen,
                    const int *rlen, int *idx, float *dist, mcp_stream_t stream);

/* Spatially pruned variant of mcp_knn for large clouds: identical results (same definition, same fp32
 * canon), but queries and references are given in Morton order and each tile of consecutive sorted references
 * has a bounding box, so a wave visits tiles by ascending lower bound and stops early.
 *   mcp_morton_codes: xyz (B,N,3), box (B,6) = per-batch (min xyz, max xyz) -> codes (B,N) int32 (30 bit);
 *                     the caller sorts by code (any stable or unstable sort) to get a permutation.
 *   mcp_tile_boxes:   sorted_xyz (B,N,3) -> boxes (B,ceil(N/tile),6), tile = mcp_knn_tile_size().
 *   mcp_knn_pruned:   query_sorted (B,Q,3) with qperm (B,Q) = original row of each sorted query (NULL = identity),
 *                     ref_sorted (B,N,3) with rperm (B,N) = original index of each sorted reference, boxes as above
 *                     -> idx (B,Q,K) ORIGINAL reference indices at ORIGINAL query rows (+ dist).  1 <= K <= 32, N <= 65536.
 *   mcp_build_cloud:  all of the above in one launch for N <= 16384 (bbox, isotropic Morton keys, block radix sort, gather,
 *                     tile boxes): xyz (B,N,3) -> sorted_xyz (B,N,3), perm (B,N) int32, boxes (B,ceil(N/tile),6). */
int mcp_knn_tile_size(void); /* references per box tile (64): boxes arrays have ceil(N / tile) rows */
int mcp_build_cloud(int b, int n, const float *xyz, float *sorted_xyz, int *perm, float *boxes, mcp_stream_t stream);
int mcp_morton_codes(int b, int n, const float *xyz, const float *box, int *codes, mcp_stream_t stream);
int mcp_tile_boxes(int b, int n, const float *sorted_xyz, float *boxes, mcp_stream_t stream);
int mcp_knn_pruned(int b, int q, int n, int k, int dist_form, const float *query_sorted, const int *qperm,
                   const float *ref_sorted, const int *rperm, const float *boxes, int *idx, float *dist, mcp_stream_t stream);

/* The pruned search on a padded batch of clouds of different sizes: the result of mcp_knn_lengths, bit for bit (live rows: the K
 * smallest under (distance, original index) among references 0 .. rlen[bb]-1, ascending, the tail repeating the last valid entry
 * if rlen[bb] < K, index 0 / distance 0 if rlen[bb] == 0; rows at or beyond qlen[bb]: index 0 / distance 0), visiting only the
 * tiles the pruning keeps.  Lengths are (B) int32 DEVICE arrays, read and clamped to [0, N] (or [0, Q]) by the kernels; grids,
 * strides and the boxes' ceil(N/tile) rows per element keep the padded sizes.  A NULL length means every row is valid, and with
 * every length NULL each entry point IS its original above (same launch, same bits).  Same limits and error codes as the
 * originals; an argument error launches nothing.  No row beyond a length -- of a cloud, a sorted cloud, a perm or the boxes --
 * is ever read.
 *   mcp_build_cloud_lengths:  N <= 16384.  sorted_xyz[bb, :len], perm[bb, :len] and boxes[bb, :ceil(len/tile)] are what
 *                             mcp_build_cloud returns for xyz[bb, :len] on its own; beyond them perm[bb, s] = s and the
 *                             coordinates and boxes are zero.
 *   mcp_morton_codes_lengths: box (B,6) = (min xyz, max xyz) over each element's LIVE rows; codes[bb, :len] are mcp_morton_codes'
 *                             for the prefix with that box, codes[bb, len:] = 0x7fffffff (above every live code), so a STABLE
 *                             sort by code leaves the padding where it is: perm[bb, s] = s for s >= len, which the search
 *                             relies on.
 *   mcp_tile_boxes_lengths:   boxes over the first len rows of sorted_xyz; tiles beyond them are zero.
 *   mcp_knn_pruned_lengths:   clouds as built by the entry points above with the same lengths (a cloud whose length is NULL
 *                             here: by the plain ones).  A padded query's zeros go to the row of its sorted position. */
int mcp_build_cloud_lengths(int b, int n, const float *xyz, const int *len, float *sorted_xyz, int *perm, float *boxes,
                            mcp_stream_t stream);
int mcp_morton_codes_lengths(int b, int n, const float *xyz, const float *box, const int *len, int *codes, mcp_stream_t stream);
int mcp_tile_boxes_lengths(int b, int n, const float *sorted_xyz, const int *len, float *boxes, mcp_stream_t stream);
int mcp_knn_pruned_lengths(int b, int q, int n, int k, int dist_form, const float *query_sorted, const int *qperm,
                           const float *ref_sorted, const int *rperm, const float *boxes, const int *qlen, const int *rlen,
                           int *idx, float *dist, mcp_stream_t stream);

/* knn_point_cosine(nsample, xyz, new_xyz) (pointconv_util.py:111-153) on channel-last features:
 * qfeat (B,Q,C), rfeat (B,N,C) -> idx (B,Q,K) (and dist if non-NULL): the K smallest of
 * d = 1 - <q^,r^>, x^ = x / sqrt(sum x^2 + 1e-8), under the order (d, index), ascending.
 * C in {64,128,256}, 1 <= K <= 16.  workspace: B*(Q+N)*C floats (normalised copies), caller-owned. */
int mcp_knn_cosine(int b, int q, int n, int c, int k, const float *qfeat, const float *rfeat, int *idx, float *dist,
                   float *workspace, mcp_stream_t stream);

/* mcp_knn_cosine on a padded batch of feature sets of different sizes: element bb searches only the first rlen[bb] rows of rfeat
 * and only its first qlen[bb] query rows are live.  qlen, rlen: (B) int32 DEVICE arrays, read by the kernels (no synchronisation)
 * and clamped there to [0,Q] / [0,N]; either may be NULL = every row valid, and with both NULL the call IS mcp_knn_cosine (same
 * launches, same bits).  C in {64,128,256}, 1 <= K <= 16, workspace B*(Q+N)*C floats as there; the rows of the workspace that
 * belong to padded rows are left unwritten and nothing depends on them.  The search is split from the padded sizes; the result
 * does not depend on the split.
 *   live rows (i < qlen[bb]):    the K smallest under (1 - cosine, index) among references 0 .. rlen[bb]-1, ascending -- what
 *                                mcp_knn_cosine returns for the two valid prefixes on their own; if rlen[bb] < K the tail repeats
 *                                the last valid entry; if rlen[bb] == 0, index 0 and distance 0;
 *   padded rows (i >= qlen[bb]): index 0, distance 0.
 * Rows of qfeat and rfeat beyond a length are never read: their contents influence no output bit.  Errors as mcp_knn_cosine
 * (nothing is launched): K > 16 or another C is MCP_ERR_UNSUPPORTED; a null qfeat, rfeat, idx or workspace, a non-positive
 * dimension or a pointer that is not 16-byte aligned is MCP_ERR_BAD_ARG.  Profiled as MCP_KERNEL_KNN_COSINE. */
int mcp_knn_cosine_lengths(int b, int q, int n, int c, int k, const float *qfeat, const float *rfeat, const int *qlen,
                           const int *rlen, int *idx, float *dist, float *workspace, mcp_stream_t stream);

/* index_points_group / index_points_gather (mocopci.py:1190-1215) without the permute copies:
 * points (B,N,C) channel-last, idx (B,T) -> out (B,T,C) (T = S*K or S), whole C*4-byte rows. */
int mcp_group_rows(int b, int n, int c, int t, const float *points, const int *idx, float *out, mcp_stream_t stream);
/* grouping + centre offset + LeakyReLU, the first layer of cross() when it is not fused into mcp_cross_volume
 * (pointconv_util.py:762-770): points (B,N,C), idx (B,S,K), centre (B,S,C) -> out (B,S,K,C) = leaky(points[idx] + centre).
 * C % 4 == 0, 16-byte aligned pointers. */
int mcp_group_rows_add_leaky(int b, int n, int c, int s, int k, float slope, const float *points, const int *idx,
                             const float *centre, float *out, mcp_stream_t stream);
/* its backward (channel-last counterpart of group_points_grad, group_points_gpu.cu:49-75): grad_out (B,T,C), idx (B,T)
 * -> grad_points (B,N,C) += scatter; the caller zero-initialises grad_points. */
int mcp_group_rows_grad(int b, int n, int c, int t, const float *grad_out, const int *idx, float *grad_points, mcp_stream_t stream);

/* The same gradient as a DETERMINISTIC segmented reduction: the caller sorts the T gather positions of each batch
 * element by destination row with a stable sort and passes the permutation order (B,T) int32 and the CSR offsets seg (B,N+1)
 * int32 (seg[b][d] .. seg[b][d+1] = the slice of order[b] that gathers row d).  grad_points (B,N,C) is fully written (rows
 * nobody gathered are zero), summed in the sorted order: bit-identical from run to run, no atomics. */
int mcp_group_rows_grad_sorted(int b, int n, int c, int t, const float *grad_out, const int *order, const int *seg,
                               float *grad_points, mcp_stream_t stream);

/* The operands of the *_grad_sorted entry points from a gather list: idx (B,T) int32 with values in [0,n) -> order (B,T) = the gather
 * positions 0..T-1 of each batch element sorted by (destination, position) -- a stable sort's result, whatever order the kernel's
 * atomics are served in -- and seg (B,n+1) = the CSR offsets.  A counting sort (count / scan / fill / per-row rank: five launches)
 * in place of a general key-value sort; positions whose value is outside [0,n) are left out (seg[b][n] = the number kept).
 * workspace: mcp_scatter_segments_workspace_bytes(b,t,n) caller-owned bytes. */
size_t mcp_scatter_segments_workspace_bytes(int b, int t, int n);
int mcp_scatter_segments(int b, int t, int n, const int *idx, int *order, int *seg, void *workspace, size_t workspace_bytes,
                         mcp_stream_t stream);

/* UpsampleFlow.forward (mocopci.py:1485-1502) / the interpolation half of PointWarping (:1472-1479):
 * dense (B,N,3), sparse (B,S,3), feat (B,S,C) channel-last -> out (B,N,C);
 * 3-NN in expansion form, weights 1/max(||d||,1e-10) normalised.  idx3 (int32) and w3 (B,N,3) are
 * caller-provided outputs (the library holds no workspace); callers can reuse them for further
 * feature tensors on the same (dense, sparse) pair via mcp_interp3_apply.  mcp_interp3_weights is the middle step on
 * its own: idx3 (B,N,3) from any exact 3-NN search (mcp_knn or mcp_knn_pruned, expansion form) -> w3 (B,N,3). */
int mcp_interp3(int b, int n, int s, int c, const float *dense, const float *sparse, const float *feat, float *out, int *idx3,
                float *w3, mcp_stream_t stream);
int mcp_interp3_weights(int b, int n, int s, const float *dense, const float *sparse, const int *idx3, float *w3,
                        mcp_stream_t stream);
int mcp_interp3_apply(int b, int n, int s, int c, const float *feat, const int *idx3, const float *w3, float *out,
                      mcp_stream_t stream);
/* backward of mcp_interp3_weights: grad_w3 (B,N,3) = dL/dw3 -> grad_dense (B,N,3) and grad_nb (B,N,3,3) = dL/d(sparse[idx3_j]) per
 * gathered neighbour, which the caller scatters with mcp_group_rows_grad_sorted (C = 3, the (order, seg) pair of idx3 viewed as
 * (B,3N)).  The three distances are recomputed; a neighbour whose distance was clamped to 1e-10 gets a zero gradient (as torch's
 * norm + clamp), grad_dense = -((g_0 + g_1) + g_2).  Either output may be NULL, not both.  Bit-reproducible. */
int mcp_interp3_weights_grad(int b, int n, int s, const float *dense, const float *sparse, const int *idx3, const float *grad_w3,
                             float *grad_dense, float *grad_nb, mcp_stream_t stream);
/* backward of mcp_interp3_apply w.r.t. feat (channel-last counterpart of three_interpolate_grad, interpolate_gpu.cu:126-150):
 * grad_out (B,N,C) -> grad_feat (B,S,C) += w3 * grad_out at idx3; the caller zero-initialises grad_feat. */
int mcp_interp3_apply_grad(int b, int n, int s, int c, const float *grad_out, const int *idx3, const float *w3, float *grad_feat,
                           mcp_stream_t stream);

/* Deterministic backward of mcp_interp3_apply (autograd over the blend of UpsampleFlow / PointWarping, mocopci.py:1480-1481,
 * :1500-1501; the reference's K9, interpolate_gpu.cu:120-161, adds with atomicAdd): grad_w3 (B,N,3) = <grad_out[b,p,:],
 * feat[b, idx3[b,p,j], :]> and grad_feat (B,S,C) = the w3-weighted scatter of grad_out, every destination row's addends in ascending
 * position 3p + j -- (order (B,3N), seg (B,S+1)) = mcp_scatter_segments of idx3 viewed as (B, 3N) with n = S.  Either output may be
 * NULL (then feat / order / seg are not read).  Sums in a fixed order: bit-reproducible; no (B,N,3,C) intermediate. */
int mcp_interp3_apply_grad_sorted(int b, int n, int s, int c, const float *feat, const int *idx3, const float *w3, const float *grad_out,
                                  const int *order, const int *seg, float *grad_feat, float *grad_w3, mcp_stream_t stream);

/* MultiFrameEstimatier.knn_group + fusion (mocopci.py:798-819) after the two neighbour searches:
 * p1 (B,N,3) centres, p2 (B,N,3) gathered set, idx (B,N,64) int32 into p2 (32 self-neighbours of p1
 * followed by 32 neighbours of p1 in p2); per neighbour [d, |d|] -> 4->64->64->128 (1x1 conv + eval
 * BatchNorm folded into w,b by the caller + ReLU) -> channel max -> softmax over the 64 neighbours ->
 * weighted sum of neighbour coordinates -> out (B,N,3).  w1 (64,4), w2 (64,64), w3 (128,64) row-major.
 * nb must be 64 (the reference's fixed k = 32 + 32).  idx2 == NULL: idx is the (B,N,64) list; otherwise idx and idx2 are its
 * two halves as separate (B,N,32) lists, exactly as the two searches produce them (no concatenation pass). */
int mcp_fusion(int b, int n, int nb, const float *p1, const float *p2, const int *idx, const int *idx2, const float *w1, const float *b1,
               const float *w2, const float *b2, const float *w3, const float *b3, float *out, mcp_stream_t stream);

/* Backward of mcp_fusion (the reference differentiates mocopci.py:803-819 with autograd over the materialised (B,128,N,64)
 * activations; its only hand-written backward pieces are the atomicAdd scatters of group_points_gpu.cu:8-44).  Same arguments as
 * mcp_fusion, plus grad_out (B,N,3) = dL/dout.  Writes
 *   grad_p1 (B,N,3)       dL/dp1;
 *   grad_nb (B,N,64,3)    dL/d(p2[idx]) per gathered neighbour, in the order of the neighbour list(s) -- the caller scatters it into
 *                         dL/dp2 with mcp_group_rows_grad_sorted (deterministic) or any scatter-add of its own;
 *   grad_weights          mcp_fusion_grad_floats() = 12800 floats: dW1 (64,4) | db1 (64) | dW2 (64,64) | db2 (64) | dW3 (128,64) | db3 (128),
 *                         with respect to the (BatchNorm-folded) w, b the caller passed.
 * The layer is re-evaluated inside the kernel (nothing of size B x N x 64 x C is read or written except grad_nb); weight
 * gradients are summed per wave, per workgroup and over workgroups in fixed orders: results repeat bit for bit.
 * workspace: mcp_fusion_grad_workspace_bytes(b, n) bytes of device memory (the workgroups' partial weight gradients); w3 16-byte
 * aligned.  ReLU and the channel max take torch's subgradients (0 at 0; one arg-max channel), |r| has gradient 0 at r = 0. */
int mcp_fusion_grad_floats(void);
size_t mcp_fusion_grad_workspace_bytes(int b, int n);
int mcp_fusion_grad(int b, int n, int nb, const float *p1, const float *p2, const int *idx, const int *idx2, const float *w1, const float *b1,
                    const float *w2, const float *b2, const float *w3, const float *b3, const float *grad_out, float *grad_p1, float *grad_nb,
                    float *grad_weights, void *workspace, size_t workspace_bytes, mcp_stream_t stream);

/* mcp_fusion / mcp_fusion_grad on a padded batch of clouds of different sizes (csrc/fusion_lengths.hip: kernels of their own, stated
 * once with the dense ones in csrc/fusion_tile.h / fusion_grad_tile.h).
 *   len     (B) device int32, clamped to [0, n] inside the kernels: point p of element bb is live iff p < len[bb].  NULL: the call is
 *           the dense entry point itself.
 * One wave owns one point, so liveness is wave-uniform: the length is a scalar load and a padded point costs one branch and the
 * store of its zeros.  A padded point, forward: none of its row of p1, idx, idx2 is read and nothing is gathered through those lists
 * (they may hold NaN and out-of-range indices); its row of out is written as exact zeros.  Backward: its row of grad_out is not read
 * either, its row of grad_p1 and its 64 rows of grad_nb are exact zeros and it adds nothing to any accumulator of grad_weights (the
 * caller's mcp_scatter_segments still walks its row of idx and leaves out-of-range values out).  The indices of live points are
 * trusted; the caller makes them point at live rows of p2.  A live point gets the bits of the dense call.
 * No length is read on the host, nothing is allocated, no atomics.  The grids are those of b * n points and the points are dealt to
 * workgroups and waves in padded order, exactly as the dense kernels deal them, so grad_weights is the dense call's sum with the
 * padded points' terms left out -- bit-identical to mcp_fusion_grad on the batch with zeroed padding and zero upstream rows -- and
 * with every len[bb] == n every output is bit-identical to the dense entry point.  Argument checks and error codes are the dense
 * entries'; workspace: mcp_fusion_grad_workspace_bytes(b, n), as dense. */
int mcp_fusion_lengths(int b, int n, int nb, const float *p1, const float *p2, const int *idx, const int *idx2, const int *len, const float *w1,
                       const float *b1, const float *w2, const float *b2, const float *w3, const float *b3, float *out, mcp_stream_t stream);
int mcp_fusion_grad_lengths(int b, int n, int nb, const float *p1, const float *p2, const int *idx, const int *idx2, const int *len, const float *w1,
                            const float *b1, const float *w2, const float *b2, const float *w3, const float *b3, const float *grad_out, float *grad_p1,
                            float *grad_nb, float *grad_weights, void *workspace, size_t workspace_bytes, mcp_stream_t stream);

/* The fusion layer in net.train() mode (train.py:130): its three Conv2d + BatchNorm2d + ReLU layers (mocopci.py:749-755, :810-816)
 * normalise with the statistics of the batch they are given -- one call here = one reference call = one set of statistics over
 * all b * n * 64 (point, neighbour) rows.  Arguments as mcp_fusion with the RAW conv weights (w, b), then
 *   bn    mcp_fusion_bn_floats() = 1024 floats, per layer (64, 64, 128 channels) mean | rstd | gamma | beta: the caller fills gamma
 *         and beta (the BatchNorm weight / bias), this call fills mean and rstd = 1 / sqrt(var + eps);
 *   var   64 + 64 + 128 floats: the biased batch variances (the caller's running-estimate update scales them by n / (n - 1)).
 * Four passes (statistics of layer 1, 2, 3, then the layer itself), nothing of size rows x channels is written.
 * workspace: mcp_fusion_bn_workspace_bytes(b, n) bytes. */
int mcp_fusion_bn_floats(void);
size_t mcp_fusion_bn_workspace_bytes(int b, int n);
int mcp_fusion_bn_forward(int b, int n, int nb, const float *p1, const float *p2, const int *idx, const int *idx2, const float *w1, const float *b1,
                          const float *w2, const float *b2, const float *w3, const float *b3, float eps, float *bn, float *var, float *out,
                          void *workspace, size_t workspace_bytes, mcp_stream_t stream);

/* Backward of mcp_fusion_bn_forward (one reference call; bn as that call left it).  grad_out (B,N,3).  The BatchNorm terms
 * dz = (gamma / sigma)(dy' - mean(dy') - zhat mean(dy' zhat)) need sums over all rows between the layers: four passes, the layer
 * re-evaluated in each as far as it is needed; dy2' and dy1' (rows x 64) pass through caller-provided scratch.  Scratch, rows = b n 64:
 * row_c (rows int32), row_dy, row_a (rows floats), dy2, dy1 (rows x 64 floats, 16-byte aligned).  Writes grad_p1 (B,N,3), grad_nb (B,N,64,3)
 * (scattered into dL/dp2 by the caller, as for mcp_fusion_grad), grad_weights (12800 floats in mcp_fusion_grad's layout; the conv
 * biases' entries are 0: a bias in front of a batch-statistics BatchNorm has no gradient) and grad_affine (512 floats: dgamma1 |
 * dbeta1 | dgamma2 | dbeta2 | dgamma3 | dbeta3).  All sums in fixed orders.  workspace: mcp_fusion_bn_grad_workspace_bytes(b, n). */
size_t mcp_fusion_bn_grad_workspace_bytes(int b, int n);
int mcp_fusion_bn_backward(int b, int n, int nb, const float *p1, const float *p2, const int *idx, const int *idx2, const float *w1, const float *b1,
                           const float *w2, const float *b2, const float *w3, const float *b3, const float *bn, const float *grad_out, int *row_c,
                           float *row_dy, float *row_a, float *dy2, float *dy1, float *grad_p1, float *grad_nb, float *grad_weights,
                           float *grad_affine, void *workspace, size_t workspace_bytes, mcp_stream_t stream);

/* The pair that keeps what the backward's first pass would otherwise re-evaluate the whole layer for: per (point, neighbour) row
 * (rows = b * n * 64) the neighbour's score (the maximum over the layer-3 channels, floored at 0), the channel it sits at and zhat3 there
 * -- save_c (int32), save_z, save_s (floats), caller-owned, 12 bytes per row.  mcp_fusion_bn_forward_save = mcp_fusion_bn_forward + these
 * outputs (same out / bn / var bit for bit); mcp_fusion_bn_backward_saved = mcp_fusion_bn_backward with a first pass that reads them
 * (same gradients bit for bit). */
int mcp_fusion_bn_forward_save(int b, int n, int nb, const float *p1, const float *p2, const int *idx, const int *idx2, const float *w1, const float *b1,
                               const float *w2, const float *b2, const float *w3, const float *b3, float eps, float *bn, float *var, float *out, int *save_c,
                               float *save_z, float *save_s, void *workspace, size_t workspace_bytes, mcp_stream_t stream);
int mcp_fusion_bn_backward_saved(int b, int n, int nb, const float *p1, const float *p2, const int *idx, const int *idx2, const float *w1, const float *b1,
                                 const float *w2, const float *b2, const float *w3, const float *b3, const float *bn, const float *grad_out,
                                 const int *save_c, const float *save_z, const float *save_s, int *row_c, float *row_dy, float *row_a, float *dy2, float *dy1,
                                 float *grad_p1, float *grad_nb, float *grad_weights, float *grad_affine, void *workspace, size_t workspace_bytes,
                                 mcp_stream_t stream);

/* mcp_fusion_bn_forward / mcp_fusion_bn_backward on a padded batch of clouds of different sizes (csrc/fusion_bn_lengths.hip).
 *   len     (B) device int32, clamped to [0, n] inside the kernels: point p of element bb is live iff p < len[bb].  NULL: the call is
 *           the dense entry point, bit for bit (count then receives b * n).
 *   count   (forward; may be NULL) one device int32 that receives the LIVE POINTS of the call, sum of the clamped lengths (saturated
 *           at 2^31 - 1).  The statistics run over m = 64 * count rows; the caller's running-variance update scales by m / (m - 1).
 * Statistics: the live rows are R = {(bb, p, j): p live, j < 64}; every mean and variance of the three layers, every mean term of the
 * backward and every entry of grad_weights / grad_affine runs over R only.  The variance is formed as in the dense call (sums of
 * z - s and (z - s)^2, merged in double); the shift s is the conv output at the first row of the first LIVE point.  m < 2 (no live
 * point): every division is by max(m, 1), there is no shift, nothing is NaN or Inf and the statistics mean nothing.
 * A padded point, forward: its row of out is zero; none of its rows of p1, idx, idx2 is read.  Backward: its row of grad_out is not
 * read, its row of grad_p1 and its 64 rows of grad_nb are exact zeros, its rows of row_c / row_dy / row_a / dy2 / dy1 are
 * UNSPECIFIED (not written, and no pass reads them), it adds nothing to grad_weights, grad_affine or any partial sum, and its row
 * of idx is not read by these kernels (the caller's mcp_scatter_segments still walks it and leaves out-of-range values out).
 * The indices of live points are trusted; the caller makes them point at live rows of p2.
 * No length is read on the host, nothing is allocated, no atomics: every sum runs in a fixed order and two calls give identical
 * bits.  The grids are those of b * n points and live points are dealt in padded order, so with every len[bb] == n every output is
 * bit-identical to the dense entry point.  Workspaces: mcp_fusion_bn_workspace_bytes / mcp_fusion_bn_grad_workspace_bytes (b, n), as
 * dense.
 * mcp_fusion_bn_forward_save_lengths / mcp_fusion_bn_backward_saved_lengths: the pair that keeps the forward's scores (save_c, save_z,
 * save_s as for mcp_fusion_bn_forward_save), with lengths.  A padded point's rows of save_c / save_z / save_s are UNSPECIFIED: the
 * forward does not write them and the backward does not read them.  Otherwise the pair is mcp_fusion_bn_forward_lengths /
 * mcp_fusion_bn_backward_lengths bit for bit (out / bn / var / count; grad_p1 / grad_nb / grad_weights / grad_affine), as the dense pair
 * is mcp_fusion_bn_forward / mcp_fusion_bn_backward; len == NULL: the dense pair itself (count then receives b * n). */
int mcp_fusion_bn_forward_lengths(int b, int n, int nb, const float *p1, const float *p2, const int *idx, const int *idx2, const int *len,
                                  const float *w1, const float *b1, const float *w2, const float *b2, const float *w3, const float *b3, float eps,
                                  float *bn, float *var, float *out, int *count, void *workspace, size_t workspace_bytes, mcp_stream_t stream);
int mcp_fusion_bn_backward_lengths(int b, int n, int nb, const float *p1, const float *p2, const int *idx, const int *idx2, const int *len,
                                   const float *w1, const float *b1, const float *w2, const float *b2, const float *w3, const float *b3, const float *bn,
                                   const float *grad_out, int *row_c, float *row_dy, float *row_a, float *dy2, float *dy1, float *grad_p1,
                                   float *grad_nb, float *grad_weights, float *grad_affine, void *workspace, size_t workspace_bytes,
                                   mcp_stream_t stream);
int mcp_fusion_bn_forward_save_lengths(int b, int n, int nb, const float *p1, const float *p2, const int *idx, const int *idx2, const int *len,
                                       const float *w1, const float *b1, const float *w2, const float *b2, const float *w3, const float *b3, float eps,
                                       float *bn, float *var, float *out, int *count, int *save_c, float *save_z, float *save_s, void *workspace,
                                       size_t workspace_bytes, mcp_stream_t stream);
int mcp_fusion_bn_backward_saved_lengths(int b, int n, int nb, const float *p1, const float *p2, const int *idx, const int *idx2, const int *len,
                                         const float *w1, const float *b1, const float *w2, const float *b2, const float *w3, const float *b3,
                                         const float *bn, const float *grad_out, const int *save_c, const float *save_z, const float *save_s, int *row_c,
                                         float *row_dy, float *row_a, float *dy2, float *dy1, float *grad_p1, float *grad_nb, float *grad_weights,
                                         float *grad_affine, void *workspace, size_t workspace_bytes, mcp_stream_t stream);

/* BatchNorm on BATCH statistics of a channels-last tensor, forward and backward, with per-group lengths (csrc/bn_batch.hip): what
 * nn.BatchNorm1d / 2d in training mode computes when the reference's blocks call it once per sample (mocopci.py:503-506, :554-561).
 *   x       (G, F, N, C) float32, contiguous, 16-byte aligned: G groups normalised separately, F frames that share a group's length.
 *   len     (G) device int32, clamped to [0, n] inside the kernels: row (f, i) of group gg is live iff i < len[gg], so the group has
 *           m = F * len[gg] live rows.  NULL: every row is live.
 *   gamma, beta (C); mean, var (G, C): the batch mean and the BIASED batch variance; count (G) int32 receives m.
 *   y       (G, F, N, C) = (x - mean) * (gamma * rstd) + beta on live rows, rstd = 1 / sqrt(var + eps); exact zeros on padded rows.
 * Backward: grad_x = gamma * rstd * (grad_y - sum(grad_y) / m - xhat * sum(grad_y * xhat) / m) on live rows, xhat = (x - mean) * rstd
 * formed again from x, mean and var (nothing of size rows x C is kept besides x); exact zeros on padded rows.  grad_gamma, grad_beta
 * (C): the groups' sums of grad_y * xhat and of grad_y, added in group order.
 * Statistics: a group's F * N padded rows are cut into mcp_bn_batch_parts(g, f, n, c) chunks -- a pure function of its arguments, never
 * of the device or of a length -- one workgroup each; the variance comes from the sums of x - s and (x - s)^2 with the shift
 * s = x[gg,0,0,:] (live whenever any row is), the chunks merged in chunk order in double.  m == 0: mean 0, var 0, y all zero; m == 1:
 * var 0; every division is by max(m, 1), nothing is NaN or Inf.  Padded rows of x and of grad_y are never read.
 * No length is read on the host, nothing is allocated, no atomics: every sum runs in a fixed order and two calls give identical bits;
 * with every len[gg] == n every output is bit-identical to len == NULL.
 * c in {32, 64, 128, 256}: anything else MCP_ERR_UNSUPPORTED (workspace size 0).  A non-positive dimension, g > 65535, f * n > 2^30, a
 * NULL pointer (len excepted), a short workspace or a pointer that is not 16-byte aligned (workspace: 8): MCP_ERR_BAD_ARG.  Nothing is
 * launched on an error.  workspace: mcp_bn_batch_workspace_bytes(g, f, n, c) caller-owned bytes, for either direction. */
int mcp_bn_batch_parts(int g, int f, int n, int c);
size_t mcp_bn_batch_workspace_bytes(int g, int f, int n, int c);
int mcp_bn_batch_forward(int g, int f, int n, int c, const float *x, const int *len, const float *gamma, const float *beta, float eps, float *mean,
                         float *var, int *count, float *y, void *workspace, size_t workspace_bytes, mcp_stream_t stream);
int mcp_bn_batch_backward(int g, int f, int n, int c, const float *x, const int *len, const float *gamma, const float *mean, const float *var, float eps,
                          const float *grad_y, float *grad_x, float *grad_gamma, float *grad_beta, void *workspace, size_t workspace_bytes,
                          mcp_stream_t stream);

/* Cost-volume cross() after its neighbour searches (pointconv_util.py:750-781, :894-922, :1126-1161):
 * xyz1 (B,N1,3), xyz2 (B,N2,3), points1 (B,N1,D), points2 (B,N2,D) channel-last (16-byte aligned),
 * idx (B,N1,32) int32 into set 2 (16 feature-cosine + 16 xyz neighbours) -> out (B,N1,D) = max over the 32
 * neighbours of LeakyReLU(wmlp . LeakyReLU(points2[idx] + points1 + wpos.(xyz2[idx]-xyz1) + bpos) + bmlp).
 * The layer's weights -- wpos (D,3), bpos (D) = the Conv2d 3->D; wmlp (D,D), bmlp (D) = the single Conv2d D->D of
 * the mlp list (every layer MoCoPCI builds has exactly one) -- are packed ONCE per layer by mcp_cross_pack into
 * the MFMA-operand image (mcp_cross_packed_floats(D) floats, 16-byte aligned, caller-owned).  D in {64,128,256}, k = 32.  Neighbour lists: idx (B,N1,32), or with idx2 != NULL
 * the 16 + 16 halves as two (B,N1,16) lists (feature-space neighbours, then coordinate-space neighbours).  bmap != NULL (B int32):
 * the batch replicates / selects a smaller one -- element bb of the tensors flagged in `shared` (1 points1, 2 points2, 4 the
 * first index list) is read from element bmap[bb] of the unreplicated tensor (Multiframe_Attention's three flow iterations share
 * their features, mocopci.py:191-197); xyz1, xyz2 and idx2 are per element.  The map is kept in LDS: b <= 1024 when one is passed
 * (MCP_ERR_UNSUPPORTED beyond). */
int mcp_cross_packed_floats(int d);
int mcp_cross_pack(int d, const float *wpos, const float *bpos, const float *wmlp, const float *bmlp, float *packed,
                   mcp_stream_t stream);
int mcp_cross_volume(int b, int n1, int n2, int d, int k, const float *xyz1, const float *xyz2, const float *points1,
                     const float *points2, const int *idx, const int *idx2, const int *bmap, int shared, const float *packed, float *out, mcp_stream_t stream);

/* Set-abstraction layer of pointnet2 after its neighbour search (PointnetSAModule[MSG], pointnet2_modules.py; SetConv and
 * FlowEmbedding, models/layers.py:76-117): grouping, shared per-pair MLP and the pool over the neighbours in one kernel.
 * xyz (B,N,3), new_xyz (B,M,3), features (B,N,C) channel-last or NULL (c = 0), idx (B,M,nsample) int32 into the N points
 * -> out (B,M,widths[L-1]).  For a live centre p of element bb, with k_j = idx[bb,p,j]:
 *     x_j = [xyz[bb,k_j] - new_xyz[bb,p] (if use_xyz) | features[bb,k_j]],
 *     h1_j = ReLU(W1 x_j + b1 (+ row_bias[bb,p])),  hl_j = ReLU(Wl h(l-1)_j + bl),
 *     out[bb,p] = max_j hL_j (pool 0) or the mean over all nsample slots (pool 1);
 * repeated indices count as often as they appear (the ball query's "repeat the first hit" padding needs no count).
 * W_l (widths[l], cin_l) row-major and b_l (widths[l]) -- eval-mode BatchNorm already folded in by the caller -- are packed ONCE by
 * mcp_group_mlp_pack into the MFMA-operand image (mcp_group_mlp_packed_floats floats, 16-byte aligned, caller-owned; w and b are
 * host arrays of `layers` device pointers, widths a host array).  row_bias (B,M,widths[0]) or NULL is added before the first ReLU:
 * with the centre's own features sent through mcp_linear it expresses FlowEmbedding's concatenation.  qlen (B) device int32 or
 * NULL, as in mcp_ball_query_lengths (clamped to [0, m] in the kernel, NULL = every centre live): a centre at or beyond qlen[bb]
 * writes zeros and none of its rows of new_xyz, idx or row_bias is read.
 * Supported: 1 <= nsample <= 64; c a multiple of 4, 0 <= c <= 128 (c = 0 needs use_xyz); 1 to 3 layers; hidden widths in
 * {32, 64, 128}, last width in {32, 64, 128, 256}.  Anything else: MCP_ERR_UNSUPPORTED (mcp_group_mlp_packed_floats: 0), nothing
 * is launched.  features, row_bias, packed, out 16-byte aligned (MCP_ERR_BAD_ARG).  Indices are trusted.  No allocation, no
 * environment variable, no host read of a length. */
int mcp_group_mlp_packed_floats(int c, int layers, const int *widths);
int mcp_group_mlp_pack(int c, int use_xyz, int layers, const int *widths, const float *const *w, const float *const *b, float *packed,
                       mcp_stream_t stream);
int mcp_group_mlp(int b, int n, int m, int c, int nsample, int use_xyz, int pool, int layers, const int *widths, const float *xyz,
                  const float *new_xyz, const float *features, const int *idx, const int *qlen, const float *row_bias, const float *packed,
                  float *out, mcp_stream_t stream);

/* Feature-propagation layer of pointnet2 after its three-neighbour search (PointnetFPModule, pointnet2_modules.py:116-156;
 * FeaturePropagation, models/layers.py:150-178): blend of the three known rows, concatenation with the skip row and the shared
 * per-point MLP in one kernel.  Channel-last known_feats (B,m,C2), skip (B,n,C1) or NULL (c1 = 0), idx (B,n,3) int32 into the m
 * known points, dist (B,n,3) as three_nn returns it (square roots) -> out (B,n,widths[L-1]).  For a live row p of element bb:
 *     weights by `rule`: 0: w = w3 (B,n,3) as given (dist is not read, may be NULL);
 *                        1: r_j = 1 / (dist_j + 1e-8),                 w_j = r_j / ((r_0 + r_1) + r_2)   (pointnet2);
 *                        2: r_j = 1 / max(dist_j * dist_j, 1e-10),     the same normalisation             (layers.py);
 *     x = [(w0 f[i0] + w1 f[i1]) + w2 f[i2] | skip[bb,p]],   h1 = ReLU(W1 x + b1), ..., out[bb,p] = ReLU(WL h(L-1) + bL).
 * Under rules 1 and 2 a slot whose dist is +inf (fewer than three known points) has weight exactly 0 and its row of known_feats
 * is not read; three such slots give an interpolated part of exact zeros, never a NaN.  W_l (widths[l], cin_l) row-major and b_l
 * -- eval-mode BatchNorm already folded in by the caller -- are packed ONCE by mcp_fp_mlp_pack (mcp_fp_mlp_packed_floats floats,
 * 16-byte aligned, caller-owned; w and b are host arrays of `layers` device pointers, widths a host array).  ulen (B) device int32
 * or NULL (clamped to [0, n] in the kernel, NULL = every row live): a row at or beyond ulen[bb] writes zeros and none of its rows
 * of idx, dist, w3 or skip is read.  Every output element is written.
 * Supported: c2 a multiple of 4 in 4 .. 512; 0 <= c1 <= 512 (any value); c1 + c2 <= 768; 1 to 3 layers of width 32, 64, 128 or
 * 256.  Anything else: MCP_ERR_UNSUPPORTED (mcp_fp_mlp_packed_floats: 0), nothing is launched.  known_feats, packed, out -- and
 * skip when c1 is a multiple of 4 -- 16-byte aligned (MCP_ERR_BAD_ARG).  Indices are trusted.  No allocation, no environment
 * variable, no host read of a length. */
int mcp_fp_mlp_packed_floats(int c2, int c1, int layers, const int *widths);
int mcp_fp_mlp_pack(int c2, int c1, int layers, const int *widths, const float *const *w, const float *const *b, float *packed,
                    mcp_stream_t stream);
int mcp_fp_mlp(int b, int n, int m, int c2, int c1, int rule, int layers, const int *widths, const float *known_feats, const float *skip,
               const int *idx, const float *dist, const float *w3, const int *ulen, const float *packed, float *out, mcp_stream_t stream);

/* Backward of mcp_fp_mlp (csrc/fp_mlp_grad.hip).  Inputs, rules, ulen and infinite slots as mcp_fp_mlp; grad_out (B,n,widths[L-1]) =
 * dL/dout.  With gz_L = grad_out . [out > 0], gz_(l-1) = (W_l^T gz_l) . [h_(l-1) > 0] and dx = W_1^T gz_1 it writes
 *   grad_skip (B,n,C1) = dx[C2:] (NULL with c1 = 0);
 *   grad_known_feats (B,m,C2) += w_j dx[:C2] at idx_j, every destination row's addends in ascending position 3 p + j -- (order
 *       (B,3n), seg (B,m+1)) = mcp_scatter_segments of idx viewed as (B,3n) with n = m; NULL: not computed, order / seg not read;
 *   grad_w[l] (widths[l], cin_l) and grad_b[l] (widths[l]): host arrays of `layers` device pointers, of the FOLDED weights' shapes;
 *   out (B,n,widths[L-1]) or NULL: the forward's result again, bit for bit.
 * dist, w3 and the coordinates get NO gradient, as in the reference (its ThreeNN and ThreeInterpolate return none for them).
 * A padded row has none of its float inputs read, grad_out included, writes zeros to grad_skip and adds nothing anywhere else; its
 * row of idx must be readable (mcp_scatter_segments and the scatter walk every position; out-of-range values are left out).  Rows of
 * known_feats that no live slot gathers get exactly zero; an infinite slot weighs exactly 0.  No atomics: every sum runs in a fixed
 * order (mcp_interp3_apply_grad_sorted, mcp_linear_wgrad), two calls give identical bits.  packed: the image of
 * mcp_fp_mlp_grad_pack (mcp_fp_mlp_grad_packed_floats floats: mcp_fp_mlp_pack's image followed by the slabs of the transposed
 * weights), rebuilt whenever a weight changes.  workspace: mcp_fp_mlp_grad_workspace_bytes(b, n, ...) caller-owned bytes; it receives
 * x (rows, C2+C1), h_l for l < L, gz_l for every l, dx[:C2] and the weights the blend used.  Supported shapes: those of mcp_fp_mlp;
 * anything else MCP_ERR_UNSUPPORTED (sizes: 0), nothing launched.  known_feats, packed, grad_out, out, workspace -- and skip,
 * grad_skip when c1 is a multiple of 4 -- 16-byte aligned.  No allocation, no environment variable, no host read of a length. */
int mcp_fp_mlp_grad_packed_floats(int c2, int c1, int layers, const int *widths);
int mcp_fp_mlp_grad_pack(int c2, int c1, int layers, const int *widths, const float *const *w, const float *const *b, float *packed,
                         mcp_stream_t stream);
size_t mcp_fp_mlp_grad_workspace_bytes(int b, int n, int c2, int c1, int layers, const int *widths);
int mcp_fp_mlp_grad(int b, int n, int m, int c2, int c1, int rule, int layers, const int *widths, const float *known_feats,
                    const float *skip, const int *idx, const float *dist, const float *w3, const int *ulen, const float *packed,
                    const float *grad_out, const int *order, const int *seg, float *grad_known_feats, float *grad_skip,
                    float *const *grad_w, float *const *grad_b, float *out, void *workspace, size_t workspace_bytes, mcp_stream_t stream);

/* mcp_fp_mlp's layer with TRAINING-MODE BatchNorm behind every product (csrc/fp_mlp_bn.hip).  Inputs, rules, ulen and infinite slots
 * as mcp_fp_mlp.  Over the live rows R (count m), for l = 1 .. L:  z_l = W_l h_(l-1) + b_l,  mu_l = mean_R z_l,  v_l = mean_R (z_l -
 * mu_l)^2 (biased),  rstd_l = 1 / sqrt(v_l + eps_l),  y_l = gamma_l (z_l - mu_l) rstd_l + beta_l,  h_l = ReLU(y_l),  out = h_L.
 * mcp_fp_mlp_bn_forward writes out (B,n,widths[L-1]; zeros in padded rows), mean[l], var[l], rstd[l] (widths[l] floats each: host
 * arrays of `layers` device pointers) and the live count m as one device int32.  gamma / beta: host arrays of `layers` device
 * pointers, a NULL entry is ones / zeros; eps: a host array of `layers` floats, each > 0.  packed: mcp_fp_mlp_pack's image of the
 * UNFOLDED (W_l, b_l) (zeros for an absent bias), or mcp_fp_mlp_grad_pack's, which begins with it.
 * mcp_fp_mlp_bn_backward takes the forward's inputs again, mean and rstd as the forward wrote them, grad_out = dL/dout and
 * mcp_fp_mlp_grad_pack's image, and writes -- with gy_L = grad_out . [y_L > 0], dbeta_l = sum_R gy_l, dgamma_l = sum_R gy_l zhat_l,
 * gz_l = gamma_l rstd_l (gy_l - dbeta_l / m - zhat_l dgamma_l / m), gy_(l-1) = (W_l^T gz_l) . [y_(l-1) > 0], dx = W_1^T gz_1 --
 *   grad_skip (B,n,C1) = dx[C2:] (NULL with c1 = 0), zeros in padded rows;
 *   grad_known_feats (B,m,C2) through (order, seg) as mcp_fp_mlp_grad (NULL: not computed);
 *   grad_w[l] (widths[l], cin_l); grad_b[l], grad_gamma[l], grad_beta[l] (widths[l]): host arrays of `layers` device pointers, a NULL
 *       entry of the last three is not written (grad_b is zero in exact arithmetic: the statistics absorb a bias).
 * It keeps no activation: the forward passes run again with the statistics given, so every ReLU mask is the forward's.  dist, w3,
 * the coordinates and the lengths get no gradient.  A padded row has none of its float inputs read (grad_out included), takes part
 * in no statistic and adds nothing to any sum.  No atomics: every per-channel sum is a fixed butterfly over a wave's rows, waves in
 * wave order, workgroups in workgroup order; two calls give identical bits.  The variance is merged from (count, mean, M2) triples,
 * never formed as E[z^2] - E[z]^2.  With m < 2 every division is by max(m, 1): nothing is NaN or Inf, the statistics are meaningless.
 * workspace: mcp_fp_mlp_bn_workspace_bytes(b, n, ..., backward) caller-owned bytes (backward = 0: z_l and the partials; 1: also x, h_l,
 * gy_l, gz_l, dx[:C2], the blend's weights and mcp_linear_wgrad's sums).  Supported shapes: those of mcp_fp_mlp; anything else
 * MCP_ERR_UNSUPPORTED (size: 0), nothing launched.  known_feats, packed, out, grad_out, workspace -- and skip, grad_skip when c1 is a
 * multiple of 4 -- 16-byte aligned.  No allocation, no environment variable, no host read of a length. */
size_t mcp_fp_mlp_bn_workspace_bytes(int b, int n, int c2, int c1, int layers, const int *widths, int backward);
int mcp_fp_mlp_bn_forward(int b, int n, int m, int c2, int c1, int rule, int layers, const int *widths, const float *known_feats,
                          const float *skip, const int *idx, const float *dist, const float *w3, const int *ulen, const float *packed,
                          const float *const *gamma, const float *const *beta, const float *eps, float *out, float *const *mean,
                          float *const *var, float *const *rstd, int *count, void *workspace, size_t workspace_bytes, mcp_stream_t stream);
int mcp_fp_mlp_bn_backward(int b, int n, int m, int c2, int c1, int rule, int layers, const int *widths, const float *known_feats,
                           const float *skip, const int *idx, const float *dist, const float *w3, const int *ulen, const float *packed,
                           const float *const *gamma, const float *const *beta, const float *const *mean, const float *const *rstd,
                           const float *grad_out, const int *order, const int *seg, float *grad_known_feats, float *grad_skip,
                           float *const *grad_w, float *const *grad_b, float *const *grad_gamma, float *const *grad_beta, void *workspace,
                           size_t workspace_bytes, mcp_stream_t stream);

/* Backward of mcp_group_mlp (csrc/group_mlp_grad.hip).  Inputs, use_xyz, pool, row_bias and qlen as mcp_group_mlp; grad_out
 * (B,M,widths[L-1]) = dL/dout.  For a live centre p, slots j < nsample, k_j = idx[p,j]:
 *     max:  gy_j[ch] = grad_out[p,ch] for the lowest j with hL_j[ch] == out[p,ch], 0 for every other slot (F.max_pool2d's rule);
 *     mean: gy_j = grad_out[p] / nsample;
 *     gz_L = gy . [hL > 0],  gz_l = (W_(l+1)^T gz_(l+1)) . [h_l > 0],  dx_j = W_1^T gz_(1,j).
 * It writes, each only when its pointer is not NULL,
 *   grad_features (B,N,c) += dx_j[3:] and grad_xyz (B,N,3) += dx_j[:3] at row k_j, every destination row's addends in ascending
 *       position p nsample + j -- (order (B, M nsample), seg (B, N+1)) = mcp_scatter_segments of idx viewed as (B, M nsample) with
 *       n = N; rows that no slot gathers get exact zeros; order / seg are read only when one of the two is wanted;
 *   grad_new_xyz (B,M,3) = -sum_j dx_j[:3];   grad_row_bias (B,M,widths[0]) = sum_j gz_(1,j) (needs row_bias);
 *   grad_w[l] (widths[l], cin_l) and grad_b[l] (widths[l]): host arrays of `layers` device pointers (required), of the FOLDED
 *       weights' shapes; grad_w[0] covers the three position columns when use_xyz;
 *   out (B,M,widths[L-1]): the forward's result again, bit for bit.
 * idx gets no gradient.  The columns of a group beyond nsample take part in no sum.  A padded centre has none of its float inputs
 * read, grad_out included; it writes zeros to its rows of grad_new_xyz and grad_row_bias and adds nothing anywhere else; its row of
 * idx must be readable (mcp_scatter_segments and the scatter walk every position; out-of-range values are left out).  With
 * nsample > 32 the two column tiles of a centre agree on the winner through a first pooling pass over the recomputed values: the
 * forward's out is not an input.  No atomics: every sum runs in a fixed order (mcp_group_rows_grad_sorted, mcp_linear_wgrad, the
 * forward's butterfly inside a group), two calls give identical bits.  packed: the image of mcp_group_mlp_grad_pack
 * (mcp_group_mlp_grad_packed_floats floats: mcp_group_mlp_pack's image followed by the pieces of the transposed weights), rebuilt
 * whenever a weight changes.  workspace: mcp_group_mlp_grad_workspace_bytes(b, m, ...) caller-owned bytes; it receives, per
 * (centre, slot) pair, x, h_l for l < L, gz_l for every l and dx -- the dense intermediate the forward avoids -- and the partial
 * sums of mcp_linear_wgrad.  Supported shapes: those of mcp_group_mlp; anything else MCP_ERR_UNSUPPORTED (sizes: 0), nothing
 * launched.  features, row_bias, packed, grad_out, out, grad_features, grad_row_bias, workspace 16-byte aligned.  No allocation, no
 * environment variable, no host read of a length. */
int mcp_group_mlp_grad_packed_floats(int c, int use_xyz, int layers, const int *widths);
int mcp_group_mlp_grad_pack(int c, int use_xyz, int layers, const int *widths, const float *const *w, const float *const *b, float *packed,
                            mcp_stream_t stream);
size_t mcp_group_mlp_grad_workspace_bytes(int b, int m, int c, int nsample, int use_xyz, int layers, const int *widths);
int mcp_group_mlp_grad(int b, int n, int m, int c, int nsample, int use_xyz, int pool, int layers, const int *widths, const float *xyz,
                       const float *new_xyz, const float *features, const int *idx, const int *qlen, const float *row_bias,
                       const float *packed, const float *grad_out, const int *order, const int *seg, float *grad_features, float *grad_xyz,
                       float *grad_new_xyz, float *grad_row_bias, float *const *grad_w, float *const *grad_b, float *out, void *workspace,
                       size_t workspace_bytes, mcp_stream_t stream);

/* mcp_group_mlp's layer with TRAINING-MODE BatchNorm behind every product (csrc/group_mlp_bn.hip).  Inputs, use_xyz, pool and qlen as
 * mcp_group_mlp (no row_bias).  Over the live pairs R = {(p, j): p a live centre, j < nsample} (count m; every slot counts, the ones
 * that repeat the ball query's first hit included), k = idx[p,j], for l = 1 .. L:  x = [xyz[k] - new_xyz[p] (use_xyz) | features[k]],
 * z_l = W_l h_(l-1) + b_l,  mu_l = mean_R z_l,  v_l = mean_R (z_l - mu_l)^2 (biased),  rstd_l = 1 / sqrt(v_l + eps_l),
 * y_l = gamma_l (z_l - mu_l) rstd_l + beta_l,  h_l = ReLU(y_l),  out[p] = max_j h_(L,j) (pool 0) or (sum_j h_(L,j)) / nsample (pool 1).
 * mcp_group_mlp_bn_forward writes out (B,M,widths[L-1]; zeros for padded centres), mean[l], var[l], rstd[l] (widths[l] floats each:
 * host arrays of `layers` device pointers) and the live count m as one device int32.  gamma / beta: host arrays of `layers` device
 * pointers, a NULL entry is ones / zeros; eps: a host array of `layers` floats, each > 0.  packed: mcp_group_mlp_bn_pack's image
 * (mcp_group_mlp_bn_packed_floats floats), ONE image for both directions, built from the UNFOLDED (W_l, b_l) (zeros for an absent
 * bias), W_1 (widths[0], 3 + c) in the module's order with the position columns first; rebuilt whenever a weight changes.
 * mcp_group_mlp_bn_backward takes the forward's inputs again, mean and rstd as the forward wrote them and grad_out (B,M,widths[L-1]) =
 * dL/dout, and writes -- with gy_L the pool's gradient through [y_L > 0] (max: grad_out[p,ch] to the LOWEST j with h_(L,j)[ch] ==
 * out[p,ch], F.max_pool2d's rule, nothing for a pooled value <= 0; mean: grad_out[p] / nsample to every slot), dbeta_l, dgamma_l,
 * gz_l, gy_(l-1) as mcp_fp_mlp_bn_backward and dx = W_1^T gz_1 per pair -- each only when its pointer is not NULL,
 *   grad_features (B,N,c) += dx[3:] and grad_xyz (B,N,3) += dx[:3] at row k through (order, seg) as mcp_group_mlp_grad; rows that no
 *       slot gathers get exact zeros;
 *   grad_new_xyz (B,M,3) = -sum_j dx[:3] in slot order, zeros for padded centres;
 *   grad_w[l] (widths[l], cin_l; required); grad_b[l], grad_gamma[l], grad_beta[l] (widths[l]): host arrays of `layers` device
 *       pointers, a NULL entry of the last three is not written (grad_b is zero in exact arithmetic: the statistics absorb a bias).
 * It keeps no activation: the forward passes run again with the statistics given, so every ReLU mask and every pool winner is the
 * forward's.  idx and the lengths get no gradient.  A padded centre has none of its float inputs read (grad_out included), takes
 * part in no statistic and adds nothing to any sum; its row of idx must be readable.  No atomics: every sum runs in a fixed order, two
 * calls give identical bits.  The variance is merged from (count, mean, M2) triples.  With m < 2 every division is by max(m, 1).
 * workspace: mcp_group_mlp_bn_workspace_bytes(b, m, ..., backward) caller-owned bytes (backward = 0: z_l per pair and the partials;
 * 1: also x, h_l, gy_l, gz_l, dx and mcp_linear_wgrad's sums).  Supported shapes: those of mcp_group_mlp; anything else
 * MCP_ERR_UNSUPPORTED (sizes: 0), nothing launched.  features, packed, out, grad_out, grad_features, workspace 16-byte aligned.  No
 * allocation, no environment variable, no host read of a length. */
int mcp_group_mlp_bn_packed_floats(int c, int use_xyz, int layers, const int *widths);
int mcp_group_mlp_bn_pack(int c, int use_xyz, int layers, const int *widths, const float *const *w, const float *const *b, float *packed,
                          mcp_stream_t stream);
size_t mcp_group_mlp_bn_workspace_bytes(int b, int m, int c, int nsample, int use_xyz, int layers, const int *widths, int backward);
int mcp_group_mlp_bn_forward(int b, int n, int m, int c, int nsample, int use_xyz, int pool, int layers, const int *widths, const float *xyz,
                             const float *new_xyz, const float *features, const int *idx, const int *qlen, const float *packed,
                             const float *const *gamma, const float *const *beta, const float *eps, float *out, float *const *mean,
                             float *const *var, float *const *rstd, int *count, void *workspace, size_t workspace_bytes, mcp_stream_t stream);
int mcp_group_mlp_bn_backward(int b, int n, int m, int c, int nsample, int use_xyz, int pool, int layers, const int *widths, const float *xyz,
                              const float *new_xyz, const float *features, const int *idx, const int *qlen, const float *packed,
                              const float *const *gamma, const float *const *beta, const float *const *mean, const float *const *rstd,
                              const float *grad_out, const int *order, const int *seg, float *grad_features, float *grad_xyz,
                              float *grad_new_xyz, float *const *grad_w, float *const *grad_b, float *const *grad_gamma,
                              float *const *grad_beta, void *workspace, size_t workspace_bytes, mcp_stream_t stream);

/* Backward of mcp_cross_volume for one cross layer given by its own weights (the reference differentiates pointconv_util.py:765-781
 * with autograd over three materialised (B,D,32,N1) tensors; its hand-written backward pieces are the atomicAdd scatters of
 * group_points_gpu.cu:8-44).  xyz1, xyz2, points1, points2, idx / idx2 as mcp_cross_volume (no batch map); wpos (D,3), bpos (D),
 * wmlp (D,D), bmlp (D) row-major; grad_out (B,N1,D) = dL/dout.  Writes
 *   grad_xyz1 (B,N1,3), grad_points1 (B,N1,D);
 *   grad_dir (B,N1,32,3) and grad_rows (B,N1,32,D): dL/d(xyz2[idx]) and dL/d(points2[idx]) per gathered neighbour, in the order of
 *       the neighbour list(s) -- the caller scatters them with mcp_group_rows_grad_sorted (deterministic);
 *   grad_weights: mcp_cross_grad_floats(d) floats = dWpos (D,3) | dbpos (D) | dWmlp (D,D) | dbmlp (D).
 * The layer is re-evaluated in the kernel; the arg-max neighbour of a channel is the lowest list position among equal maxima;
 * all sums run in fixed orders (results repeat bit for bit).  workspace: mcp_cross_grad_workspace_bytes(b, n1, d) bytes.
 * D = 64 and 128 (the level-1 and level-2 cost volumes, 97 % of the layer's backward time at the training shape); D = 256:
 * MCP_ERR_UNSUPPORTED and mcp_cross_grad_floats returns 0 here -- that width has its own entry, mcp_cross256_grad below.
 * workspace 16-byte aligned. */
int mcp_cross_grad_floats(int d);
size_t mcp_cross_grad_workspace_bytes(int b, int n1, int d);
int mcp_cross_grad(int b, int n1, int n2, int d, int k, const float *xyz1, const float *xyz2, const float *points1, const float *points2,
                   const int *idx, const int *idx2, const float *wpos, const float *bpos, const float *wmlp, const float *bmlp,
                   const float *grad_out, float *grad_xyz1, float *grad_dir, float *grad_points1, float *grad_rows, float *grad_weights,
                   void *workspace, size_t workspace_bytes, mcp_stream_t stream);

/* Backward of mcp_cross_volume at D = 256 (cross3, pointconv_util.py:783-791).  Arguments, outputs (grad_dir (B,N1,32,3), grad_rows
 * (B,N1,32,256), grad_weights = dWpos (256,3) | dbpos (256) | dWmlp (256,256) | dbmlp (256): mcp_cross256_grad_floats() floats), tie
 * rule (lowest list position among equal maxima) and errors (k != 32: MCP_ERR_UNSUPPORTED; short workspace, null or misaligned
 * pointer: MCP_ERR_BAD_ARG; nothing is launched) as mcp_cross_grad; both index forms.  z is recomputed with the forward's own kernel
 * arithmetic (same weight image, same MFMA order), so the arg-max neighbours are the forward's.  The gradient of z is non-zero at
 * one neighbour per (point, channel): dx and dWmlp are exact fp32 sums over those entries, every sum in a fixed order (results repeat
 * bit for bit, no atomics).  grad_rows doubles as scratch for the layer's hidden activations while the call runs.
 * workspace: mcp_cross256_grad_workspace_bytes(b, n1) bytes, 16-byte aligned (2 KB per point + up to about 20 MB). */
int mcp_cross256_grad_floats(void);
size_t mcp_cross256_grad_workspace_bytes(int b, int n1);
int mcp_cross256_grad(int b, int n1, int n2, int k, const float *xyz1, const float *xyz2, const float *points1, const float *points2,
                      const int *idx, const int *idx2, const float *wpos, const float *bpos, const float *wmlp, const float *bmlp,
                      const float *grad_out, float *grad_xyz1, float *grad_dir, float *grad_points1, float *grad_rows, float *grad_weights,
                      void *workspace, size_t workspace_bytes, mcp_stream_t stream);

/* PointConv / PointConvD up to the final Linear (mocopci.py:1218-1266, :1289-1300, :1330-1335):
 * s_xyz (B,N,3), new_xyz (B,S,3) centres, s_points (B,N,D) channel-last, idx (B,S,32) int32 into the
 * N source points; WeightNet Conv2d 3->8->8->8 + ReLU as w0 (8,3), w1 (8,8), w2 (8,8) and biases.
 * out (B,S,(3+D)*8), 16-byte aligned: out[b,s,c*8+m] = sum_k [dxyz|feat][k][c] * weightnet(dxyz[k])[m],
 * i.e. the tensor the reference feeds to self.linear.  k must be 32. */
int mcp_pointconv_agg(int b, int n, int s, int d, int k, const float *s_xyz, const float *new_xyz, const float *s_points,
                      const int *idx, const float *w0, const float *b0, const float *w1, const float *b1, const float *w2,
                      const float *b2, float *out, mcp_stream_t stream);

/* Backward of mcp_pointconv_agg (the reference differentiates mocopci.py:1330-1335 with autograd over the materialised (B,S,32,3+D)
 * grouping; its hand-written backward pieces are the atomicAdd scatters of group_points_gpu.cu:8-44).  Arguments as
 * mcp_pointconv_agg, plus grad_out (B,S,(3+D)*8) = dL/dout, 16-byte aligned.  Writes
 *   grad_new_xyz (B,S,3);
 *   grad_gxyz (B,S,32,3) and grad_rows (B,S,32,D): dL/d(s_xyz[idx]) and dL/d(s_points[idx]) per gathered neighbour -- the caller
 *       scatters them with mcp_group_rows_grad_sorted (deterministic);
 *   grad_weights: mcp_pointconv_agg_grad_floats() = 176 floats: dW0 (8,3) | db0 (8) | dW1 (8,8) | db1 (8) | dW2 (8,8) | db2 (8).
 * The WeightNet is re-evaluated per (centre, neighbour) pair; all sums run in fixed orders (results repeat bit for bit).
 * workspace: mcp_pointconv_agg_grad_workspace_bytes(b, s) bytes.  k = 32; d a multiple of 4, 4 <= d <= 256. */
int mcp_pointconv_agg_grad_floats(void);
size_t mcp_pointconv_agg_grad_workspace_bytes(int b, int s);
int mcp_pointconv_agg_grad(int b, int n, int s, int d, int k, const float *s_xyz, const float *new_xyz, const float *s_points, const int *idx,
                           const float *w0, const float *b0, const float *w1, const float *b1, const float *w2, const float *b2,
                           const float *grad_out, float *grad_new_xyz, float *grad_gxyz, float *grad_rows, float *grad_weights,
                           void *workspace, size_t workspace_bytes, mcp_stream_t stream);

/* PointConv / PointConvD after the sampling as ONE launch (models/m_models/mocopci.py:1330-1342 and :1381-1393: group + WeightNet +
 * matmul + Linear((3+D)*8 -> C_out) + LeakyReLU): the (B,S,(3+D)*8) aggregate stays on the compute unit.  Arguments as
 * mcp_pointconv_agg, then `packed`: the mcp_linear_pack image of the Linear's (C_out, (3+D)*8) weight (one piece) with its bias;
 * `slope`: the activation's negative slope (0.1 in the reference; 1 = none); out (B,S,C_out).
 * (D, C_out) = (32, 32) or (64, 64), k = 32; anything else returns MCP_ERR_UNSUPPORTED (use mcp_pointconv_agg + mcp_linear).
 * From 16384 rows (B*S) up the result is bit-identical to mcp_pointconv_agg followed by mcp_linear (same operand split, same
 * summation order); below that mcp_linear sums K in four parts and the two differ in the last bits. */
int mcp_pointconv_linear(int b, int n, int s, int d, int k, const float *s_xyz, const float *new_xyz, const float *s_points,
                         const int *idx, const float *w0, const float *b0, const float *w1, const float *b1, const float *w2,
                         const float *b2, const float *packed, int c_out, float slope, float *out, mcp_stream_t stream);

/* PointConv on a padded batch whose elements have their own number of centres: mcp_pointconv_agg, mcp_pointconv_linear and
 * mcp_pointconv_agg_grad with per-element centre lengths.  Arguments as the dense entry points, plus qlen behind idx: a (B,) int32
 * DEVICE array that the kernels clamp to [0, s]; the host never reads it (no synchronisation).  qlen == NULL is the dense entry
 * point: same dispatch, same launch, same bits.
 *   - Centre i of element bb is live iff i < qlen[bb].
 *   - Live centres get the dense call's bits; the kernel form is a function of the padded shape alone, as in the dense dispatch.
 *   - A padded centre has none of its inputs read -- its idx row, new_xyz, the gathered rows, grad_out --, so padding may hold
 *     anything (NaN, inf, out-of-range indices).  Its output rows are exact zeros: the aggregate; the fused Linear's output row
 *     (zero, NOT leaky(bias)); grad_new_xyz, grad_gxyz and grad_rows.
 *   - A padded centre adds nothing to the 176 WeightNet weight gradients: its lanes work on zeros in place of their loads (never on
 *     padding times a zero gradient), and every sum keeps its fixed order, so full lengths give the dense call's bits.
 *   - A workgroup (forward) or wave (backward) whose centres are all padded writes its zeros and skips the loads.
 * The source points (s_xyz, s_points) have no length here: a live centre's idx row names the rows it gathers, and the search that
 * made it (mcp_knn_lengths, ...) keeps those below the element's reference length. */
int mcp_pointconv_agg_lengths(int b, int n, int s, int d, int k, const float *s_xyz, const float *new_xyz, const float *s_points,
                              const int *idx, const int *qlen, const float *w0, const float *b0, const float *w1, const float *b1,
                              const float *w2, const float *b2, float *out, mcp_stream_t stream);
int mcp_pointconv_linear_lengths(int b, int n, int s, int d, int k, const float *s_xyz, const float *new_xyz, const float *s_points,
                                 const int *idx, const int *qlen, const float *w0, const float *b0, const float *w1, const float *b1,
                                 const float *w2, const float *b2, const float *packed, int c_out, float slope, float *out,
                                 mcp_stream_t stream);
int mcp_pointconv_agg_grad_lengths(int b, int n, int s, int d, int k, const float *s_xyz, const float *new_xyz, const float *s_points,
                                   const int *idx, const int *qlen, const float *w0, const float *b0, const float *w1, const float *b1,
                                   const float *w2, const float *b2, const float *grad_out, float *grad_new_xyz, float *grad_gxyz,
                                   float *grad_rows, float *grad_weights, void *workspace, size_t workspace_bytes, mcp_stream_t stream);

/* Multi-head attention with a tiny head dim (8 or 16) in exact fp32, flash style (no (N,N) score tensor):
 * the attention core of InterFrameAttentionInterpretation (mocopci.py:650-667) and CrossAttention (:72-86).
 * q (BF,Nq,*), k/v (BF,Nk,*) are read in place from the projection outputs: element [bf, token, head*hd + d]
 * at ptr + (bf*N + token)*stride + head*hd + d (strides in floats, multiples of 4; pointers 16-byte aligned);
 * out (BF,Nq,*) likewise.  softmax(q.k^T * scale) . v per (bf, head). */
int mcp_attention_small(int bf, int nq, int nk, int heads, int hd, const float *q, int q_stride, const float *k, int k_stride,
                        const float *v, int v_stride, float scale, float *out, int out_stride, mcp_stream_t stream);

/* Same contract for wide heads, hd in {32, 64, 256} (EI cross-former of level 3, mocopci.py:72-86 at dim 256 / 8 heads;
 * Cross_Frame_Att, mocopci.py:499-522, whose head slots are C = 256 wide): S = QK^T and PV both on fp32 MFMA, online softmax,
 * K/V streamed through LDS in 32-key tiles; nothing of size Nq x Nk is written. */
int mcp_attention_wide(int bf, int nq, int nk, int heads, int hd, const float *q, int q_stride, const float *k, int k_stride,
                        const float *v, int v_stride, float scale, float *out, int out_stride, mcp_stream_t stream);

/* Both kernels behind one entry point (hd in {8, 16, 32, 64, 256}), with a rotation of the key / value batch: batch element bf of
 * the queries attends to keys / values of batch element (bf + kv_batch_shift) mod BF (0 <= kv_batch_shift < BF).  EI_Crossformer
 * (mocopci.py:147-151) runs Injector(x1 -> x2) and Extractor(x2 -> x1) on the two halves of one stacked batch: one launch with
 * kv_batch_shift = BF / 2 instead of two. */
int mcp_attention(int bf, int nq, int nk, int heads, int hd, const float *q, int q_stride, const float *k, int k_stride,
                  const float *v, int v_stride, int kv_batch_shift, float scale, float *out, int out_stride, mcp_stream_t stream);

/* mcp_attention_small with attention dropout (net.train(): mocopci.py:660-662 / :80-82 drop entries of the softmax matrix): out =
 * dropout(softmax(q k^T scale), drop_p) v per head; the softmax is normalised before the mask, kept entries are scaled by
 * 1 / (1 - drop_p).  The mask is a counter-based hash of (seed, batch, head, query, key): the caller draws `seed` from its generator
 * per call; the backward regenerates the mask from the same seed.  Not the reference generator's mask for a given torch seed (no
 * kernel can be: the reference materialises the matrix and draws it with torch's Philox stream), the same distribution. */
int mcp_attention_small_dropout(int bf, int nq, int nk, int heads, int hd, const float *q, int q_stride, const float *k, int k_stride, const float *v,
                                int v_stride, float scale, float drop_p, unsigned seed, float *out, mcp_stream_t stream);

/* The same forward that also writes the rows' log-sum-exp (log2 domain; lse (BF, heads, Nq) floats) for mcp_attention_small_grad_lse: a
 * training forward keeps it and the backward skips the statistics pass (the Q K^T products and exponentials of the whole score matrix a
 * second time).  drop_p = 0: no mask, the result of mcp_attention_small bit for bit. */
int mcp_attention_small_lse(int bf, int nq, int nk, int heads, int hd, const float *q, int q_stride, const float *k, int k_stride, const float *v,
                            int v_stride, float scale, float drop_p, unsigned seed, float *out, float *lse, mcp_stream_t stream);

/* Backward of mcp_attention_small / mcp_attention_small_dropout (head_dim 8 / 16; the reference differentiates the materialised
 * softmax of mocopci.py:72-86, :650-667 with autograd).  q, k, v, strides, scale as the forward (no key / value batch shift);
 * drop_p, seed as the forward's (0: no dropout); out (BF,Nq,heads*hd) the forward's output, grad_out its gradient, both dense.
 * Writes grad_q (BF,Nq,heads*hd) and grad_kv (BF,Nk,2*heads*hd) laid out [dK | dV] like the reference's kv projection.  Three
 * kernels (row statistics, dQ, dK/dV); nothing of size Nq x Nk is written; fixed summation orders.
 * workspace: mcp_attention_small_grad_workspace_bytes(bf, nq, heads) bytes. */
size_t mcp_attention_small_grad_workspace_bytes(int bf, int nq, int heads);
int mcp_attention_small_grad(int bf, int nq, int nk, int heads, int hd, const float *q, int q_stride, const float *k, int k_stride, const float *v,
                             int v_stride, float scale, float drop_p, unsigned seed, const float *out, const float *grad_out, float *grad_q,
                             float *grad_kv, void *workspace, size_t workspace_bytes, mcp_stream_t stream);
/* mcp_attention_small_grad with the log-sum-exp the forward kept (mcp_attention_small_lse): one elementwise pass for D = dO . O, then the
 * dQ and dK / dV kernels.  Same workspace size. */
int mcp_attention_small_grad_lse(int bf, int nq, int nk, int heads, int hd, const float *q, int q_stride, const float *k, int k_stride, const float *v,
                                 int v_stride, float scale, float drop_p, unsigned seed, const float *out, const float *grad_out, const float *lse,
                                 float *grad_q, float *grad_kv, void *workspace, size_t workspace_bytes, mcp_stream_t stream);

/* mcp_attention_wide (hd in {32, 64, 256}) as a training forward: the same kernels (the key-split form of head width 256 under the same
 * dispatch rule, the same merge order) with the rows' log-sum-exp written (log2 domain; lse (BF, heads, Nq) floats) and, at drop_p > 0,
 * attention dropout under the mask of mcp_attention_small_dropout: the same hash of (seed, (bf * heads + head) * nq + query, key), applied
 * to P in P.V only (row sums before the mask), kept entries scaled by 1 / (1 - drop_p).  out (BF,Nq,heads*hd) is dense.  drop_p = 0: the
 * result of mcp_attention_wide bit for bit.  mcp_attention_wide_dropout is the same call without lse.  lse (and the backward's workspace)
 * are touched by scalar float accesses only: 4-byte alignment suffices for them, the other pointers are 16-byte aligned. */
int mcp_attention_wide_dropout(int bf, int nq, int nk, int heads, int hd, const float *q, int q_stride, const float *k, int k_stride, const float *v,
                               int v_stride, float scale, float drop_p, unsigned seed, float *out, mcp_stream_t stream);
int mcp_attention_wide_lse(int bf, int nq, int nk, int heads, int hd, const float *q, int q_stride, const float *k, int k_stride, const float *v,
                           int v_stride, float scale, float drop_p, unsigned seed, float *out, float *lse, mcp_stream_t stream);

/* Backward of mcp_attention_wide_lse (hd in {32, 64, 256}); arguments and layouts as mcp_attention_small_grad_lse: out / grad_out dense,
 * grad_q (BF,Nq,heads*hd), grad_kv (BF,Nk,2*heads*hd) laid out [dK | dV].  One elementwise pass for D = dO . O, a query-stationary dQ
 * kernel and a key-stationary dK / dV kernel, every product on fp32 MFMA; at head width 256 the four waves of a workgroup each take
 * 64 channels of one block of 32 rows and merge their partial score tiles through LDS in wave order.  Nothing of size Nq x Nk is written,
 * no atomics: results repeat bit for bit.  workspace: mcp_attention_wide_grad_workspace_bytes(bf, nq, nk, heads, hd) bytes (0 for
 * non-positive sizes). */
size_t mcp_attention_wide_grad_workspace_bytes(int bf, int nq, int nk, int heads, int hd);
int mcp_attention_wide_grad_lse(int bf, int nq, int nk, int heads, int hd, const float *q, int q_stride, const float *k, int k_stride, const float *v,
                                int v_stride, float scale, float drop_p, unsigned seed, const float *out, const float *grad_out, const float *lse,
                                float *grad_q, float *grad_kv, void *workspace, size_t workspace_bytes, mcp_stream_t stream);

/* ---- attention over a padded batch whose elements have their own lengths ----
 * qlen, klen: (BF) int32 device arrays; either may be NULL (that side is full).  The kernels read them and clamp to [0, nq] / [0, nk]
 * themselves; the host never reads them back, so a call causes no synchronisation.  klen is indexed by the key / value tensor's own
 * batch element: with a rotation, the queries of element b use klen[(b + kv_batch_shift) mod BF].  nq and nk stay the padded sizes:
 * they give the batch strides and, under dropout, the rows and columns of the hash (a length changes which entries exist, not their
 * mask).  With ql, kl the clamped lengths of an element:
 *     query rows i <  ql   softmax_{j < kl}(q_i . k_j scale) v_j; lse that row's log-sum-exp (log2 domain);
 *     query rows i >= ql   out = 0, lse = 0 (the rows are written: the caller need not clear out);
 *     kl = 0               every row of out and lse is 0; nothing is NaN or inf.
 * Backward: grad_q is 0 in rows >= ql and everywhere in an element with kl = 0; grad_kv (both halves) is 0 in rows >= kl and everywhere
 * in an element with ql = 0; live rows hold the gradients of the function above.  No value of q, k, v, out or grad_out at or beyond a
 * length reaches an output (padding may hold NaN or inf); the backward's D = dO . O pass covers the padded tensor, but its values at
 * rows >= ql are never read.  Key loops end at kl and a workgroup whose rows all lie beyond the length writes its zeros and returns:
 * the cost follows the live part.  A live row is computed by the same instruction sequence as the plain call on the element's sliced
 * prefixes (head widths 8 - 64: bit for bit; width 256: the key-split dispatch is decided from the PADDED sizes, and the key stages
 * are then shared out over the waves from the element's own kl).  Both arrays NULL: the plain call, forwarded.  Status codes as the
 * plain calls; qlen / klen need 4-byte alignment.
 *
 * mcp_attention_lengths: mcp_attention (hd in {8, 16, 32, 64, 256}, rotation, row strides) with lengths. */
int mcp_attention_lengths(int bf, int nq, int nk, int heads, int hd, const float *q, int q_stride, const float *k, int k_stride,
                          const float *v, int v_stride, int kv_batch_shift, float scale, const int *qlen, const int *klen, float *out,
                          int out_stride, mcp_stream_t stream);
/* The training forwards mcp_attention_small_lse (hd 8 / 16) and mcp_attention_wide_lse (hd 32 / 64 / 256) with lengths; lse may be NULL. */
int mcp_attention_small_lse_lengths(int bf, int nq, int nk, int heads, int hd, const float *q, int q_stride, const float *k, int k_stride,
                                    const float *v, int v_stride, float scale, float drop_p, unsigned seed, float *out, float *lse,
                                    const int *qlen, const int *klen, mcp_stream_t stream);
int mcp_attention_wide_lse_lengths(int bf, int nq, int nk, int heads, int hd, const float *q, int q_stride, const float *k, int k_stride,
                                   const float *v, int v_stride, float scale, float drop_p, unsigned seed, float *out, float *lse,
                                   const int *qlen, const int *klen, mcp_stream_t stream);
/* The backwards mcp_attention_small_grad_lse and mcp_attention_wide_grad_lse with lengths (out, lse: the length forward's); workspace as
 * the plain calls (mcp_attention_small_grad_workspace_bytes / mcp_attention_wide_grad_workspace_bytes). */
int mcp_attention_small_grad_lse_lengths(int bf, int nq, int nk, int heads, int hd, const float *q, int q_stride, const float *k, int k_stride,
                                         const float *v, int v_stride, float scale, float drop_p, unsigned seed, const float *out,
                                         const float *grad_out, const float *lse, float *grad_q, float *grad_kv, void *workspace,
                                         size_t workspace_bytes, const int *qlen, const int *klen, mcp_stream_t stream);
int mcp_attention_wide_grad_lse_lengths(int bf, int nq, int nk, int heads, int hd, const float *q, int q_stride, const float *k, int k_stride,
                                        const float *v, int v_stride, float scale, float drop_p, unsigned seed, const float *out,
                                        const float *grad_out, const float *lse, float *grad_q, float *grad_kv, void *workspace,
                                        size_t workspace_bytes, const int *qlen, const int *klen, mcp_stream_t stream);

/* Row normalisation with the additions in front of it (nn.LayerNorm semantics: biased variance, eps inside the root):
 *     z = x[r] (+ y[r]) (+ bias);   out[r] = (z - mean z) * rsqrt(var z + eps) (* gamma + beta)
 * x, y, out (rows, c) with row strides in floats; y, bias, gamma, beta may be NULL; c <= 1024.  Replaces the LayerNorm launches
 * of EI_Crossformer (mocopci.py:100-145: query_norm / feat_norm / ffn_norm) -- their affine parts fold into the Linear behind
 * them -- and the residual additions in front of ffn_norm. */
int mcp_add_layernorm(long long rows, int c, const float *x, long long x_stride, const float *y, long long y_stride,
                      const float *bias, const float *gamma, const float *beta, float eps, float *out, long long out_stride,
                      mcp_stream_t stream);

/* Inputs of Multi_Frame_Att (mocopci.py:200-208, :551-557) in one pass: per output row r (a (sample, frame) pair),
 *     x[r]  = fea[src_self[r]] + te_self[r]                    the flow embedding plus its time code
 *     xn[r] = scale * x[r] + shift                             norm1 in eval mode (per-channel affine)
 *     xr[r] = scale * (fea[src_partner[r]] + te_partner[r]) + shift     the attention partner, frame R-1-f of the flipped stack
 * fea (members, n, c) holds the computed members in any order; src_* (rows) index it; te_* (rows, c); x / xn / xr (rows, n, c).
 * c a multiple of 4, pointers 16-byte aligned. */
int mcp_mfa_prepare(int rows, int n, int c, const float *fea, const int *src_self, const int *src_partner, const float *te_self,
                    const float *te_partner, const float *scale, const float *shift, float *x, float *xn, float *xr, mcp_stream_t stream);

/* chamfer_loss (models/utils.py:36-45 -> pytorch3d chamfer_distance defaults): per-point squared
 * nearest distance both ways.  x (B,N,3), y (B,M,3) -> dxy (B,N), dyx (B,M); the caller takes the means. */
int mcp_chamfer_nn(int b, int n, int m, const float *x, const float *y, float *dxy, float *dyx, mcp_stream_t stream);

/* mcp_chamfer_nn over the valid prefixes of a padded batch (pytorch3d chamfer_distance's x_lengths / y_lengths): xlen, ylen (B)
 * int32 device arrays as in mcp_knn_lengths (NULL = every row valid; both NULL = mcp_chamfer_nn).  dxy[bb,i] for i < xlen[bb] is
 * the squared distance to the nearest of y[bb, 0 .. ylen[bb]-1] (0 if there is none), and symmetrically dyx; padded rows
 * receive 0, so the caller's sums over whole rows are sums over the valid ones. */
int mcp_chamfer_nn_lengths(int b, int n, int m, const float *x, const float *y, const int *xlen, const int *ylen, float *dxy,
                           float *dyx, mcp_stream_t stream);

/* Per-point Linear (1x1 convolution) with fused epilogue for the tall-skinny shapes of the caller graph (Conv1d wrapper
 * mocopci.py:1111-1127, the Linear layers of :438-468 / :821-1059, and the concatenations in front of them, :186-187, :846-847):
 *     out[r, 0:n] = act( sum_i W_i . x_i[r] + b ) [+ res[r]],   act(v) = v > 0 ? v : slope * v   (slope 1: none, 0: ReLU, 0.1: LeakyReLU)
 * The input is given as nseg <= 3 pieces x[i] (rows, k_seg[i]) with row strides x_stride[i] (floats; 16-byte aligned rows,
 * k_seg[i] a multiple of 4): the pieces of what the reference concatenates, read in place.  W is (n, sum k_seg) row-major over
 * the concatenated K axis; n <= 128, or 129..192, or 193..256, or wider in column blocks of 128 (n <= 2048, ceil(n/32) a multiple of 4).  mcp_linear_pack prepares (W, b) once into
 * mcp_linear_packed_floats(n, nseg, k_seg) caller-owned floats (0 = unsupported shape); b may be NULL. */
int mcp_linear_packed_floats(int n, int nseg, const int *k_seg);
/* Narrow-output Linear with the activation on its input: out[r, 0:n] = b + W . act(x[r]), act(v) = v > 0 ? v : in_slope v; n <= 4,
 * k in {256, 512, 1024}; W (n, k) row-major, x rows 16-byte aligned with stride x_stride floats.  The tail of Mlp_T where only the
 * flow is read (PReLU, then fc2 and mapping_xyz folded into one 4C -> 3 map, mocopci.py:1561-1565 with :566-567 / :510-511). */
int mcp_linear_narrow(long long rows, int k, int n, const float *x, int x_stride, const float *w, const float *b, float in_slope,
                      float *out, int out_stride, mcp_stream_t stream);
int mcp_linear_pack(int n, int nseg, const int *k_seg, const float *w, const float *b, float *packed, mcp_stream_t stream);
int mcp_linear(long long rows, int n, int nseg, const float *const *x, const int *x_stride, const int *k_seg, float slope,
               const float *packed, const float *res, int res_stride, float *out, int out_stride, mcp_stream_t stream);
/* mcp_linear with the kernel chosen as for `policy_rows` rows (the few-row split-K form sums K in another order than the full-K
 * form): a caller that computes a SUBSET of the rows of a tall product -- the sampled rows of a PointConvD whose every candidate
 * row another code path computes (mocopci_amd/model.py: speculative / deferred forms of one forward) -- gets the same bits. */
int mcp_linear_as(long long rows, long long policy_rows, int n, int nseg, const float *const *x, const int *x_stride, const int *k_seg,
                  float slope, const float *packed, const float *res, int res_stride, float *out, int out_stride, mcp_stream_t stream);

/* Weight and bias gradient of a tall Linear y = act(x W^T + b) (autograd over mocopci.py:1111-1127 and the per-point Linears of the
 * caller graph under train.py:162): dw (n,k) = gz^T x, db (n) = column sums of gz, for gz (rows,n) = gy * act'(z) formed by the
 * caller and x (rows,k), both row-major with the given row strides (floats).  The rows are
 * the contraction axis of f32-input MFMAs; workgroup partials are added in workgroup order (bit-reproducible; the number of
 * workgroups depends on `rows` alone).  n <= 256 and ceil(n/32) ceil(k/32) <= 64 (widths that are not multiples of 32, odd strides:
 * read element by element, zero-padded); otherwise MCP_ERR_UNSUPPORTED / a workspace size of 0.  db may be NULL.  workspace: mcp_linear_wgrad_workspace_bytes(rows, n, k) caller-owned bytes. */
size_t mcp_linear_wgrad_workspace_bytes(long long rows, int n, int k);
int mcp_linear_wgrad(long long rows, int n, int k, const float *gz, int gz_stride, const float *x, int x_stride, float *dw, float *db,
                     void *workspace, size_t workspace_bytes, mcp_stream_t stream);

/* PReLU (one slope) followed by dropout on the hidden activation of Mlp_T under net.train() (mocopci.py:1558-1565, :1592-1595: `self.act`
 * then `self.drop`), and its backward, as one elementwise pass each:
 *     out[i]    = m_i * (z[i] > 0 ? z[i] : a z[i]),      m_i = 1 / (1 - drop_p) for a kept element, 0 for a dropped one
 *     grad_z[i] = grad_out[i] m_i (z[i] > 0 ? 1 : a),    grad_slope[0] = sum_i grad_out[i] m_i min(z[i], 0)
 * `slope` points at the layer's slope ON THE DEVICE (the live parameter).  The mask is a counter-based hash of (seed, i): the caller
 * draws `seed` from its generator per call and passes the same seed to the backward, which regenerates the mask -- only z is kept
 * between the passes (the reference keeps z, the mask and the dropped activation).  Same distribution as the reference's mask, not the
 * same draws for a given torch seed (see mcp_attention_small_dropout).  grad_slope is summed in a fixed order (workgroup count a
 * function of `total` alone): bit-reproducible.  drop_p outside [0, 1): MCP_ERR_BAD_ARG.
 * workspace: mcp_prelu_dropout_grad_workspace_bytes(total) caller-owned bytes. */
int mcp_prelu_dropout(long long total, const float *z, const float *slope, float drop_p, unsigned seed, float *out, mcp_stream_t stream);
size_t mcp_prelu_dropout_grad_workspace_bytes(long long total);
int mcp_prelu_dropout_grad(long long total, const float *z, const float *slope, const float *grad_out, float drop_p, unsigned seed,
                           float *grad_z, float *grad_slope, void *workspace, size_t workspace_bytes, mcp_stream_t stream);

/* Fused two-layer per-point MLP (Mlp_T of Multi_Frame_Att, mocopci.py:1558-1565 inside :551-575, and the flow heads
 * trans_block / trans_block_2 -> mapping_xyz, :566-567 / :510-511):
 *     out[r, 0:cout] = (res ? res[r] : 0) + b2 + W2 . act(W1 . x[r] + b1),   act(v) = v > 0 ? v : slope * v   (PReLU with one slope)
 * x (rows, cin) with row stride x_stride floats (16-byte aligned rows), W1 (hidden, cin), W2 (cout, hidden); the (rows, hidden)
 * activation is never written.  Supported (the shapes where it beats the BLAS chain): cin 64 (cout <= 64), cin 128 (cout <= 32 or 97..128);
 * hidden a multiple of 32.  The weights are prepared once by mcp_mlp2_pack into mcp_mlp2_packed_floats(cin, hidden, cout) caller-owned
 * floats (0 = unsupported shape).  Depthwise k=1 convolutions and eval-mode BatchNorms around the first layer are affine and are
 * folded into (W1, b1) by the caller. */
int mcp_mlp2_packed_floats(int cin, int hidden, int cout);
int mcp_mlp2_pack(int cin, int hidden, int cout, const float *w1, const float *b1, const float *w2, const float *b2, float *packed,
                  mcp_stream_t stream);
int mcp_mlp2(long long rows, int cin, int hidden, int cout, float slope, const float *x, int x_stride, const float *res, int res_stride,
             const float *packed, float *out, int out_stride, mcp_stream_t stream);

/* Point-Transformer vector attention (TransformerBlock.forward, models/pointT_layer2.py:58-77; d_model 64, k 16) after the
 * neighbour search and the q/k/v projections: xyz (B,N,3), q/kf/vf (B,N,64) channel-last (16-byte aligned) with a common row
 * stride of qkv_stride floats (64 for separate tensors, 192 when they are slices of one packed projection), idx (B,N,16)
 * -> out (B,N,64) = sum_j softmax_j(fc_gamma(q_i - k_j + delta_j) / 8) * (v_j + delta_j), delta_j = fc_delta(xyz_i - xyz_j).
 * fc_delta = Linear(3,64) ReLU Linear(64,64) as (wd1,bd1,wd2,bd2); fc_gamma = Linear(64,64) ReLU Linear(64,64) as
 * (wg1,bg1,wg2,bg2); packed once per block by mcp_ptblock_pack (mcp_ptblock_packed_floats() floats, caller-owned). */
int mcp_ptblock_packed_floats(void);
int mcp_ptblock_pack(const float *wd1, const float *bd1, const float *wd2, const float *bd2, const float *wg1, const float *bg1,
                     const float *wg2, const float *bg2, float *packed, mcp_stream_t stream);
int mcp_ptblock_attention(int b, int n, int c, int k, int qkv_stride, const float *xyz, const float *q, const float *kf,
                          const float *vf, const int *idx, const float *packed, float *out, mcp_stream_t stream);

/* Backward of mcp_ptblock_attention for a block given by its own weights wd1 (64,3), bd1, wd2 (64,64), bd2 (fc_delta), wg1, bg1, wg2,
 * bg2 (fc_gamma) (the reference differentiates pointT_layer2.py:64-75 with autograd over five (B,N,16,64) tensors).  xyz, q, kf,
 * vf, idx, qkv_stride as mcp_ptblock_attention; grad_out (B,N,64).  Writes
 *   grad_q (B,N,64); grad_xyz_c (B,N,3): the centre's share of dL/dxyz;
 *   grad_xyz_rows (B,N,16,3), grad_k_rows, grad_v_rows (B,N,16,64): per gathered neighbour, for the caller's deterministic scatter
 *       (mcp_group_rows_grad_sorted) into dL/dxyz, dL/dk, dL/dv;
 *   grad_weights: mcp_ptblock_grad_floats() floats = dWd1 (64,3) | dbd1 | dWd2 (64,64) | dbd2 | dWg1 | dbg1 | dWg2 | dbg2.
 * The block is re-evaluated in the kernel; all sums run in fixed orders.  workspace: mcp_ptblock_grad_workspace_bytes(b, n),
 * 16-byte aligned.  c = 64, k = 16. */
int mcp_ptblock_grad_floats(void);
size_t mcp_ptblock_grad_workspace_bytes(int b, int n);
int mcp_ptblock_grad(int b, int n, int c, int k, int qkv_stride, const float *xyz, const float *q, const float *kf, const float *vf, const int *idx,
                     const float *wd1, const float *bd1, const float *wd2, const float *bd2, const float *wg1, const float *bg1, const float *wg2,
                     const float *bg2, const float *grad_out, float *grad_xyz_c, float *grad_xyz_rows, float *grad_q, float *grad_k_rows,
                     float *grad_v_rows, float *grad_weights, void *workspace, size_t workspace_bytes, mcp_stream_t stream);

/* Approximate Earth Mover's Distance (metric of test.py:90): approxmatch + matchcost of
 * models/EMD/cuda/emd_kernel.cu:29-162, :204-247 (emd_cuda.approxmatch_forward / matchcost_forward, emd.py:11-12).
 * xyz1 (B,N,3), xyz2 (B,M,3) -> cost (B) = sum_{l,k} match[l][k] |xyz2[l]-xyz1[k]|^2.  match (B,M,N) is written
 * only if non-NULL (the cost is accumulated while the transfers are produced).  workspace: B*(3N+2M) floats. */
int mcp_emd(int b, int n, int m, const float *xyz1, const float *xyz2, float *match, float *cost, float *workspace,
            mcp_stream_t stream);

/* EMD backward (emd_cuda.matchcost_backward, emd.py:16-21; emd_kernel.cu matchcostgrad1 / matchcostgrad2) without the match matrix.
 * The transport plan is a sum over the MCP_EMD_LEVELS levels, in level order j = 0..9 (level = -4^(7-j) for j = 0..8, then 0):
 *   match[l][k] = (((0 + w_0) + w_1) + ... + w_9),  w_j = __expf(level_j * d) * ratioL_j[k] * ratioR_j[l],
 *   d = |xyz2[l] - xyz1[k]|^2, ratioL_j written by pass 1 of level j, ratioR_j by pass 2.
 * mcp_emd_keep is mcp_emd (match not written; cost bit-identical) that also stores each level's ratios in `levels`,
 * mcp_emd_levels_floats(b, n, m) = B*10*(N+M) floats laid out (B, 10, N+M): levels[b][j][0..N) = ratioL_j,
 * levels[b][j][N..N+M) = ratioR_j.  workspace: B*(3N+2M) floats as mcp_emd.
 * mcp_emd_grad rebuilds match[l][k] pair by pair from `levels` (same expression and order as the forward) and writes, with
 * the match held constant as the reference does,
 *   grad1 (B,N,3): grad1[k] = (sum_l (xyz1[k] - xyz2[l]) * match[l][k]) * 2 grad_cost[b]
 *   grad2 (B,M,3): grad2[l] = (sum_k (xyz2[l] - xyz1[k]) * match[l][k]) * 2 grad_cost[b]
 * grad_cost (B).  Each sum runs over the other set in tiles of 512 entries: entry t of every tile goes to partial sum t/64, each
 * partial ascends, and the eight partials are added in order: no atomics, bit-reproducible.  A level whose level*d is below -128 for every lane of a wave is skipped (its __expf is exactly 0).
 * grad1 or grad2 may be NULL (not computed). */
#define MCP_EMD_LEVELS 10
size_t mcp_emd_levels_floats(int b, int n, int m);
int mcp_emd_keep(int b, int n, int m, const float *xyz1, const float *xyz2, float *cost, float *levels, float *workspace,
                 mcp_stream_t stream);
int mcp_emd_grad(int b, int n, int m, const float *grad_cost, const float *xyz1, const float *xyz2, const float *levels, float *grad1,
                 float *grad2, mcp_stream_t stream);

/* mcp_emd / mcp_emd_keep / mcp_emd_grad on a padded batch of clouds of different sizes: element bb is the metric of its two
 * prefixes xyz1[bb, 0 .. len1[bb]-1] and xyz2[bb, 0 .. len2[bb]-1].  len1, len2: (B) int32 DEVICE arrays, read by the kernels (no
 * synchronisation) and clamped there to [0,N] / [0,M]; either may be NULL = every row of that side valid, and with both NULL the
 * call IS mcp_emd / mcp_emd_keep / mcp_emd_grad (same launches, same bits).  Layouts keep the padded strides: xyz1 (B,N,3),
 * xyz2 (B,M,3), match (B,M,N), workspace B*(3N+2M) floats, levels (B,10,N+M), grad1 (B,N,3), grad2 (B,M,3).
 *   cost[bb]: bit for bit what mcp_emd(1, len1[bb], len2[bb], ...) returns on contiguous copies of the two prefixes (the mass
 *             ratio multiL / multiR of emd_kernel.cu:32-38 is the integer division of the element's own counts);
 *   match:    block [0..len2[bb]) x [0..len1[bb]) of match[bb] as that call writes it, exact zeros elsewhere;
 *   levels:   the live entries of each level's ratios; entries beyond a length are left unwritten and never read;
 *   grad1/2:  rows below the lengths bit for bit mcp_emd_grad's on the prefixes (same wave slices, same wave-order sum); rows at
 *             or beyond a length are exact zeros;
 *   an element with an empty side (len1[bb] == 0 or len2[bb] == 0): cost 0, match 0, gradients 0, nothing of it is loaded.
 * Rows beyond a length are never read: their contents influence no output bit.  The launches are those of the length-free calls
 * (grids over the padded N / M); a workgroup whose rows are all padding returns at once.  Errors as mcp_emd / mcp_emd_keep /
 * mcp_emd_grad (nothing is launched). */
int mcp_emd_lengths(int b, int n, int m, const float *xyz1, const float *xyz2, const int *len1, const int *len2, float *match,
                    float *cost, float *workspace, mcp_stream_t stream);
int mcp_emd_keep_lengths(int b, int n, int m, const float *xyz1, const float *xyz2, const int *len1, const int *len2, float *cost,
                         float *levels, float *workspace, mcp_stream_t stream);
int mcp_emd_grad_lengths(int b, int n, int m, const float *grad_cost, const float *xyz1, const float *xyz2, const int *len1,
                         const int *len2, const float *levels, float *grad1, float *grad2, mcp_stream_t stream);

/* emd_cuda.matchcost_forward / matchcost_backward on a caller's match (B,M,N) (emd_kernel.cu:204-247, matchcostgrad1/2).
 * mcp_matchcost: cost[b] = sum_{l,k} match[l][k] |xyz2[l]-xyz1[k]|^2; one workgroup per batch element, lane t sums
 *   k = t, t+1024, ... each over ascending l (float products, double sums), then a fixed-shape tree over the 1024 lanes.
 * mcp_matchcost_grad: grad1 (B,N,3), grad2 (B,M,3) as mcp_emd_grad, from the given match.  grad1: one lane per k (match rows
 *   read along k), the l sum in eight contiguous eighths added in order; grad2: a workgroup per 8 rows l, lane t sums
 *   k = t, t+256, ..., then a fixed-shape tree over the 256 lanes.  No atomics.  grad1 or grad2 may be NULL. */
int mcp_matchcost(int b, int n, int m, const float *xyz1, const float *xyz2, const float *match, float *cost, mcp_stream_t stream);
int mcp_matchcost_grad(int b, int n, int m, const float *grad_cost, const float *xyz1, const float *xyz2, const float *match,
                       float *grad1, float *grad2, mcp_stream_t stream);

/* ---------------- Instrumentation (bench.py roofline leg) --------------------------- */
/* mcp_prof_enable(mask): every launch of a kernel whose id bit (1 << MCP_KERNEL_*) is set in mask is bracketed
 * by hipEvents recorded on the launch stream; mask 0 disables and clears.  mcp_prof_collect(id, ...) synchronises
 * that kernel's events and returns its launch count and total milliseconds.  Off by default. */
#define MCP_KERNEL_FPS 1
#define MCP_KERNEL_KNN 2
#define MCP_KERNEL_GROUP_ROWS 3
#define MCP_KERNEL_INTERP3 4
#define MCP_KERNEL_KNN_COSINE 5
#define MCP_KERNEL_FUSION 6
#define MCP_KERNEL_CROSS 7
#define MCP_KERNEL_POINTCONV 8
#define MCP_KERNEL_ATTENTION 9
#define MCP_KERNEL_PTBLOCK 10
#define MCP_KERNEL_MLP 11
#define MCP_KERNEL_LINEAR 12
int mcp_prof_enable(int kernel_mask);
int mcp_prof_collect(int kernel_id, int *launches, float *total_ms);

#ifdef __cplusplus
}
#endif
#endif /* MOCOPCI_HIP_H */
