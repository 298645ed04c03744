// ball_query_pruned.hip -- ball query over a Morton-sorted cloud with tile boxes (gfx950): the result of mcp_ball_query_lengths,
// bit for bit (definition: ball_query.h), reading only the tiles a ball can touch.
//
// The cloud is the one the pruned KNN search uses (knn_pruned.hip: mcp_build_cloud[_lengths], or mcp_morton_codes[_lengths] + a
// stable sort + mcp_tile_boxes[_lengths]): ref_sorted (B,N,3), rperm (B,N) = original index of each sorted row, boxes
// (B,ceil(N/64),6) = (lo xyz, hi xyz) of each tile of 64 sorted rows; under lengths the live rows are the first rl sorted rows.
// Centres come in the caller's order, unsorted.  A wave owns a centre:
//
//   1. Box test.  Lane l takes tiles l, l + 64, ... (at most 16: N <= 65536) and keeps a tile when a lower bound of the squared
//      distance from the centre to the tile's box is below radius2.  The bound is exact, no slack term: per axis the gap is
//      g = max(lo - q, q - hi, 0), and the three gaps go through mcp_sqdist3's own chain, fma(gz,gz, fma(gy,gy, gx*gx)).  For a
//      point r of the box, lo <= r <= hi on every axis, so |q - r| >= g in exact arithmetic; a float subtraction is the exact
//      difference rounded, and rounding is monotone, so the computed |q - r| >= the computed g (both sides of a subtraction only
//      change sign when swapped).  Squares, products and fmas of non-negative terms are monotone under rounding as well, so the
//      bound <= the computed mcp_sqdist3(q, r) of EVERY point in the box.  A hit needs d < radius2 strictly; a tile with
//      bound >= radius2 therefore holds no hit and is skipped.  (A NaN bound fails `bound < radius2` like a NaN distance does.)
//   2. Scan.  The kept tiles are visited in ascending tile order; lane l tests sorted row 64 t + l < rl with mcp_sqdist3 in the
//      exhaustive kernel's argument order.  A hit's candidate is its ORIGINAL index rperm[64 t + l].  The next kept tile's loads
//      are issued before the current one is merged.
//   3. Selection.  The answer is the nsample smallest original indices among all hits, ascending.  Tiles are not index-ordered, so
//      every kept tile is visited and the wave keeps a sorted list, one entry per lane (nsample <= 64; INT_MAX = empty).  A hit
//      at or above the list's nsample-th entry can never be selected and is dropped; the others are merged by rank counting:
//      original indices are distinct, so an element's place in the merged order is the number of smaller elements on both sides,
//      counted with ballots; entries move to their places through one LDS row per wave.  Slots beyond the hit count hold the
//      smallest hit (the exhaustive scan's first hit); cnt = hits capped at nsample.
// No workgroup barrier: a wave's LDS row is its own.
#include <limits.h>

#include "ball_query.h"

namespace {

constexpr int PT = 64;        // rows per tile: mcp_knn_tile_size()
constexpr int MAX_TPL = 16;   // tiles per lane

__global__ __launch_bounds__(64 * BQ_WAVES) void ball_query_pruned_kernel(int n, int m, int tiles, float radius2, int nsample,
                                                                          const float *__restrict__ new_xyz, const float *__restrict__ ref,
                                                                          const int *__restrict__ rperm, const float *__restrict__ boxes,
                                                                          const int *__restrict__ qlen, const int *__restrict__ rlen,
                                                                          int *__restrict__ idx, int *__restrict__ cnt_out) {
    __shared__ int s_list[BQ_WAVES][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.y;
    const int p = blockIdx.x * BQ_WAVES + wave;
    if (p >= m) return;  // whole wave; no workgroup barriers below
    const int ql = mcp_clamped_len(qlen, b, m), rl = mcp_clamped_len(rlen, b, n);
    int *o = idx + ((size_t)b * m + p) * nsample;
    int *co = cnt_out ? cnt_out + (size_t)b * m + p : nullptr;
    if (p >= ql || rl == 0) {  // wave-uniform: a padded centre, or nothing to search -- before any load of a coordinate or a box
        bq_zero_row(lane, nsample, o, co);
        return;
    }
    const float *q = new_xyz + ((size_t)b * m + p) * 3;
    const float qx = q[0], qy = q[1], qz = q[2];
    ref += (size_t)b * n * 3;
    rperm += (size_t)b * n;
    boxes += (size_t)b * tiles * 6;

    // 1. the tiles whose box the ball can reach: bit u of `keep` = tile lane + 64 u
    const int live_tiles = (rl + PT - 1) / PT, groups = (live_tiles + 63) / 64;   // groups <= MAX_TPL
    unsigned keep = 0;
    for (int u = 0; u < groups; ++u) {
        const int t = lane + 64 * u;
        if (t < live_tiles) {
            const float *bx = boxes + (size_t)t * 6;
            const float gx = fmaxf(fmaxf(bx[0] - qx, qx - bx[3]), 0.f);
            const float gy = fmaxf(fmaxf(bx[1] - qy, qy - bx[4]), 0.f);
            const float gz = fmaxf(fmaxf(bx[2] - qz, qz - bx[5]), 0.f);
            const float bound = __builtin_fmaf(gz, gz, __builtin_fmaf(gy, gy, gx * gx));
            if (bound < radius2) keep |= 1u << u;
        }
    }
    // kept tiles in ascending order: group by group, lane by lane; -1 when none is left
    int grp = -1;
    unsigned long long rem = 0;
    auto next_tile = [&]() -> int {
        while (!rem) {
            if (++grp >= groups) return -1;
            rem = __builtin_amdgcn_ballot_w64((keep >> grp) & 1u);
        }
        const int t = (int)__builtin_ctzll(rem) + 64 * grp;
        rem &= rem - 1ull;
        return t;
    };
    struct Row { float x, y, z; int orig; bool live; };
    auto fetch = [&](int t) -> Row {
        Row r;
        const int s = t * PT + lane;
        r.live = s < rl;
        const int ss = r.live ? s : t * PT;   // the tile's first row is live: t < live_tiles
        r.x = ref[(size_t)ss * 3 + 0];
        r.y = ref[(size_t)ss * 3 + 1];
        r.z = ref[(size_t)ss * 3 + 2];
        r.orig = rperm[ss];
        return r;
    };

    int mine = INT_MAX;    // lane j: the j-th smallest original index among the hits so far
    int thr = INT_MAX;     // the nsample-th smallest: a hit at or above it is never selected
    int t = next_tile();
    Row cur = {0.f, 0.f, 0.f, 0, false};
    if (t >= 0) cur = fetch(t);
    while (t >= 0) {
        const int t2 = next_tile();
        Row nxt = cur;
        if (t2 >= 0) nxt = fetch(t2);
        // 2. the tile's hits
        const bool hit = cur.live && mcp_sqdist3(qx, qy, qz, cur.x, cur.y, cur.z) < radius2;
        const int cand = (hit && cur.orig < thr) ? cur.orig : INT_MAX;
        unsigned long long todo = __builtin_amdgcn_ballot_w64(cand != INT_MAX);
        if (todo) {
            // 3. merge by rank counting: pos = new place of this lane's list entry, rank = place of this lane's candidate
            int pos = lane, rank = 64;
            while (todo) {
                const int src = (int)__builtin_ctzll(todo);
                todo &= todo - 1ull;
                const int c = __builtin_amdgcn_readlane(cand, src);
                const int r = (int)__builtin_popcountll(__builtin_amdgcn_ballot_w64(mine < c)) +
                              (int)__builtin_popcountll(__builtin_amdgcn_ballot_w64(cand < c));
                pos += c < mine ? 1 : 0;   // empty entries (INT_MAX) move up too, behind every real one
                if (lane == src) rank = r;
            }
            __builtin_amdgcn_wave_barrier();
            if (pos < 64) s_list[wave][pos] = mine;
            if (rank < 64) s_list[wave][rank] = cand;
            __builtin_amdgcn_wave_barrier();
            mine = s_list[wave][lane];
            __builtin_amdgcn_wave_barrier();
            thr = __builtin_amdgcn_readlane(mine, nsample - 1);
        }
        t = t2;
        cur = nxt;
    }
    const bool have = mine != INT_MAX && lane < nsample;
    const int found = (int)__builtin_popcountll(__builtin_amdgcn_ballot_w64(have));
    const int first = __builtin_amdgcn_readlane(mine, 0);
    if (lane < nsample) o[lane] = found ? (have ? mine : first) : 0;
    if (co && lane == 0) *co = found;
}

}  // namespace

MCP_EXPORT int mcp_ball_query_pruned(int b, int n, int m, float radius, int nsample, const float *new_xyz, const float *ref_sorted,
                                     const int *rperm, const float *boxes, const int *qlen, const int *rlen, int *idx, int *cnt,
                                     mcp_stream_t stream) {
    MCP_CHECK_ARGS(b > 0 && n > 0 && m > 0 && nsample > 0 && new_xyz && ref_sorted && rperm && boxes && idx);
    const int tiles = (n + PT - 1) / PT;
    if (nsample > 64 || tiles > 64 * MAX_TPL) return MCP_ERR_UNSUPPORTED;
    const float radius2 = radius * radius;  // as mcp_ball_query
    hipLaunchKernelGGL(ball_query_pruned_kernel, dim3(mcp_divup(m, BQ_WAVES), b), dim3(64 * BQ_WAVES), 0, (hipStream_t)stream, n, m, tiles,
                       radius2, nsample, new_xyz, ref_sorted, rperm, boxes, qlen, rlen, idx, cnt);
    return mcp_launch_status();
}
