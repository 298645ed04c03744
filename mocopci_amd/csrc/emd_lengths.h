// emd_lengths.h -- the per-cloud lengths of the EMD kernels (emd.hip, emd_grad.hip), as knn_scan.h's LEN.
//
// LEN == false: every one of the n rows of xyz1 and m rows of xyz2 of a batch element is valid; len1 / len2 are never touched.
// LEN == true: element b works on its prefixes xyz1[b, :nl], xyz2[b, :ml] only, and computes bit for bit what the LEN == false
// kernels compute on contiguous copies of the two prefixes:
//   * both lengths are read on the device, one wave-uniform load each per workgroup, and clamped to [0,n] / [0,m]; a NULL array
//     means every row of that side is valid;
//   * every streamed loop and every live test is bounded by the lengths, tiles still start at 0, so each per-lane sum runs over
//     the same entries in the same order as on the prefix; strides stay the padded n / m;
//   * an element with an empty side has no transport plan: both counts become 0, which every kernel treats as "all padding"
//     (cost 0, match 0, gradients 0), and nothing of that element is loaded;
//   * rows beyond a length -- of the clouds, of the workspace and of the kept levels -- are never read.
#pragma once

template <bool LEN>
__device__ __forceinline__ void emd_counts(const int *__restrict__ len1, const int *__restrict__ len2, int b, int n, int m, int &nl,
                                           int &ml) {
    nl = n;
    ml = m;
    if (LEN) {
        if (len1) {
            const int v = len1[b];  // b is the workgroup's batch element: one scalar load
            nl = v < 0 ? 0 : (v > n ? n : v);
        }
        if (len2) {
            const int v = len2[b];
            ml = v < 0 ? 0 : (v > m ? m : v);
        }
        if (nl == 0 || ml == 0) nl = ml = 0;
    }
}
