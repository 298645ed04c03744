// fusion_lengths.hip -- the eval-graph fusion layer (fusion.hip) and its backward (fusion_grad.hip) on a padded batch of clouds of
// different sizes: point p of element bb is live iff p < len[bb] (clamped to [0, n] in the kernels; the host never reads a length).
// No kernel text lives here: the forward kernel is fusion_tile.h's under FUS_LEN 1, the backward kernel fusion_grad_tile.h's under
// FGR_LEN 1 (there: what a padded point costs and what is written for it), launched by those headers' fusion_split_run / fgr_run.
// Those are the functions the dense units call, deciding from the PADDED shape, so the grids, the deal of points to workgroups and
// waves and the order of every sum are the dense units', and a call with every length n gives the dense call's bits.  len == NULL is
// the dense entry point itself.  Nothing here allocates or uses an atomic.
#define FUS_LEN 1
#define FGR_LEN 1
#include "fusion_tile.h"
#include "fusion_grad_tile.h"

// mcp_fusion with per-cloud lengths (include/mocopci_hip.h)
MCP_EXPORT int mcp_fusion_lengths(int b, int n, int nb, const float *p1, const float *p2, const int *idx, const int *idx2, const int *len, const float *w1,
                                  const float *b1, const float *w2, const float *b2, const float *w3, const float *b3, float *out, mcp_stream_t stream) {
    if (!len) return mcp_fusion(b, n, nb, p1, p2, idx, idx2, w1, b1, w2, b2, w3, b3, out, stream);
    MCP_CHECK_ARGS(b > 0 && n > 0 && p1 && p2 && idx && w1 && b1 && w2 && b2 && w3 && b3 && out);
    if (nb != NB) return MCP_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    const long long total = (long long)b * n;
    mcp_prof_begin(MCP_KERNEL_FUSION, s);
    const int rc = fusion_split_run(total, n, p1, p2, idx, idx2, w1, b1, w2, b2, w3, b3, out, fusion_grid(total, FUS_GRID_CAP), s, len);
    mcp_prof_end(MCP_KERNEL_FUSION, s);
    return rc;
}

// mcp_fusion_grad with per-cloud lengths (workspace: mcp_fusion_grad_workspace_bytes, as for the dense call)
MCP_EXPORT int mcp_fusion_grad_lengths(int b, int n, int nb, const float *p1, const float *p2, const int *idx, const int *idx2, const int *len,
                                       const float *w1, const float *b1, const float *w2, const float *b2, const float *w3, const float *b3,
                                       const float *grad_out, float *grad_p1, float *grad_nb, float *grad_weights, void *workspace,
                                       size_t workspace_bytes, mcp_stream_t stream) {
    if (!len)
        return mcp_fusion_grad(b, n, nb, p1, p2, idx, idx2, w1, b1, w2, b2, w3, b3, grad_out, grad_p1, grad_nb, grad_weights, workspace, workspace_bytes,
                               stream);
    return fgr_run(b, n, nb, p1, p2, idx, idx2, w1, b1, w2, b2, w3, b3, grad_out, grad_p1, grad_nb, grad_weights, workspace, workspace_bytes,
                   (hipStream_t)stream, len);
}
