"""Float64 statement of the set-abstraction layer (csrc/group_mlp.hip: grouping, shared MLP, pool over the neighbours) with its running
error bound, under the rules of tests/fused_reference.py (whose product_stage it reuses).  A plain module: test_group_mlp_cpu.py
checks it against the fp32 composition, test_group_mlp_gpu.py checks the kernel against it.

group_mlp_reference returns (exact, bound), float64 of shape (centres, widths[-1]); `bound` is in units of 2^-24.  Stage by stage:
  * a coordinate difference carries one rounding of its own magnitude; gathered features are exact;
  * every layer is a product stage over its whole input row (coordinates, features and, in the FlowEmbedding form, the centre's own
    features concatenated to every neighbour -- the kernel receives that part as row_bias, a product of its own that the stage's
    sqrt(K) term covers);
  * ReLU and the maximum over the neighbours pass the bound on (the maximum: the largest bound among the slots);
  * the mean adds sqrt(J) roundings of the summed magnitude, and one more for the division, to the mean of the slots' bounds.
cut, sel: as in fused_reference.

group_mlp_inputs builds a case's data by that file's recipe: clustered clouds, centres that are points of the cloud, neighbour lists
that are members of the centre's cluster (so relative coordinates come from a cancellation), features and weights with a positive mean."""
import math

import torch

from tests import fused_reference as fr


def group_mlp_reference(xyz, new_xyz, features, idx, weights, use_xyz=True, pool="max", centre=None, sel=None, cut=None, block=256):
    """xyz (B,N,3), new_xyz (B,M,3), features (B,N,C) or None, idx (B,M,J), weights [(W, b), ...] with W (out, in) over the row
    [xyz_j - new_xyz (use_xyz) | features_j | centre (B,M,C2) if given]."""
    B, M, _ = new_xyz.shape

    def blk(b, i):
        j = idx[b, i].long()                                              # (P, J)
        parts, bounds = [], []
        if use_xyz:
            d = xyz[b[:, None], j].double() - new_xyz[b, i].double()[:, None]
            parts.append(d)
            bounds.append(d.abs())
        if features is not None:
            f = features[b[:, None], j].double()
            parts.append(f)
            bounds.append(torch.zeros_like(f))
        if centre is not None:
            cf = centre[b, i].double()[:, None].expand(-1, j.shape[1], -1)
            parts.append(cf)
            bounds.append(torch.zeros_like(cf))
        x, xb = torch.cat(parts, -1), torch.cat(bounds, -1)
        for w, bias in weights:
            z, xb = fr.product_stage(x, xb, w, bias, cut)
            x = torch.relu(z)
        if pool == "max":
            return x.amax(1), xb.amax(1)
        J = x.shape[1]
        return x.mean(1), xb.mean(1) + (math.sqrt(J) + 1.0) * x.abs().mean(1)

    return fr._run(blk, B * M, M, sel, block)


def mlp_weights(g, cin, widths):
    """[(W, b)] of the shared MLP: positive-mean weights scaled so that every layer's ReLU sees both signs."""
    out = []
    for w in widths:
        out.append(fr.positive_weights(g, w, cin, 2.0, -0.2))
        cin = w
    return out


CLUSTER = 32


def group_mlp_inputs(case):
    """xyz (b, n, 3), new_xyz (b, m, 3), features (b, n, c) or None, idx (b, m, nsample), centre features (b, m, c2) or None,
    [(W, b), ...].  case: b, n, m, c, nsample, widths, use_xyz (True), c2 (0)."""
    b, n, m, c, ns = case["b"], case["n"], case["m"], case["c"], case["nsample"]
    use_xyz, c2 = case.get("use_xyz", True), case.get("c2", 0)
    g = torch.Generator().manual_seed(b * 7919 + n * 31 + m + 131 * c + ns)
    xyz = fr.clustered_cloud(g, b, n, CLUSTER, case.get("extent", False))
    home = torch.arange(m) * n // m
    new_xyz = xyz[:, home].contiguous()
    feats = (torch.randn(b, n, c, generator=g) + 0.5) if c else None
    idx = fr.cluster_neighbours(g, b, m, n, ns, CLUSTER, home)
    centre = (torch.randn(b, m, c2, generator=g) + 0.5) if c2 else None
    ws = mlp_weights(g, (3 if use_xyz else 0) + c + c2, case["widths"])
    return xyz, new_xyz, feats, idx, centre, ws


def composition(xyz, new_xyz, features, idx, weights, use_xyz=True, pool="max", centre=None):
    """The layer as the modules compose it in fp32 torch: grouped tensor (B, C_in, M, J), 1x1 convolutions with ReLU, pool."""
    F = torch.nn.functional
    bi = torch.arange(xyz.shape[0], device=xyz.device)[:, None, None]
    j = idx.long()
    parts = []
    if use_xyz:
        parts.append(xyz[bi, j] - new_xyz[:, :, None])
    if features is not None:
        parts.append(features[bi, j])
    if centre is not None:
        parts.append(centre[:, :, None].expand(-1, -1, j.shape[2], -1))
    h = torch.cat(parts, -1).permute(0, 3, 1, 2).contiguous()            # (B, C_in, M, J)
    for w, bias in weights:
        h = torch.relu(F.conv2d(h, w[:, :, None, None], bias))
    h = h.amax(3) if pool == "max" else h.mean(3)
    return h.transpose(1, 2)                                             # (B, M, C_out)
