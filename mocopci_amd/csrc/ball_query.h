// ball_query.h -- what the exhaustive ball query (pointnet2_ops.hip) and the box-pruned one (ball_query_pruned.hip) share: the
// wave-per-centre geometry, the per-cloud lengths and the zero row.
//
// Result definition of every length-aware entry point (mcp_ball_query_lengths, mcp_query_and_group_lengths, mcp_ball_query_pruned):
// for element b, rl = clamp(rlen[b], 0, N) and ql = clamp(qlen[b], 0, M); a NULL length array means every row is live.  A live centre
// p < ql gets the first nsample indices k < rl, ascending, with mcp_sqdist3(centre, xyz[b,k]) < radius * radius -- what mcp_ball_query
// returns for the two prefixes on a pre-zeroed idx: slots beyond the hit count hold the first hit, no hit (or rl == 0) gives zeros.
// A padded centre p >= ql gets zeros.  cnt[b,p] = min(hits, nsample), 0 for padded centres.  Every slot is written by the kernel,
// and no row at or beyond a length is read.
#pragma once
#include "common.h"

constexpr int BQ_WAVES = 4;   // centres (waves) per workgroup

// the row of a centre without a hit, or of a padded centre
__device__ __forceinline__ void bq_zero_row(int lane, int nsample, int *__restrict__ o, int *__restrict__ cnt_slot) {
    for (int l = lane; l < nsample; l += 64) o[l] = 0;
    if (cnt_slot && lane == 0) *cnt_slot = 0;
}
