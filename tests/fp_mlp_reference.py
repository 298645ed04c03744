"""Float64 statement of the feature-propagation layer (csrc/fp_mlp.hip: three-neighbour blend, skip concatenation, shared MLP) with its
running error bound, under the rules of tests/fused_reference.py (whose product_stage it reuses).  A plain module: test_fp_mlp_cpu.py
checks it against the fp32 composition, test_fp_mlp_gpu.py checks the kernel against it.

fp_mlp_reference returns (exact, bound), float64 of shape (rows, widths[-1]); `bound` is in units of 2^-24.  The fp32 distances, the
features and (rule "given") the weights are exact inputs; the weights of the two computed rules are evaluated in float64 from the fp32
distances, with the fp32 values of the constants 1e-8 and 1e-10.  Stage by stage:
  * the blend x = (w0 f0 + w1 f1) + w2 f2 carries K_rule roundings of sum_j |w_j f_j|, counted from the fp32 operations:
      "pointnet2": den_j = dist_j + 1e-8 (1), r_j = 1 / den_j (1): r_j carries 2; S = (r0 + r1) + r2 carries the 2 of its positive
                   terms and one per addition: 4; w_j = r_j / S: 2 + 4 + 1 = 7; the product w_j f_j (1) and the two additions of
                   partial sums no larger than sum_j |w_j f_j| (2): K = 10;
      "flownet3d": den_j = dist_j * dist_j (1), raised to 1e-10 (a maximum: passes the rounding on), then as above: K = 10;
      "given":     the three products and the two additions: K = 3;
    a slot whose distance is +inf has weight exactly 0 and its row is not read (it enters as zeros, whatever the row holds); with
    three such slots the blend is exact zeros;
  * the skip columns are exact;
  * every layer is a product stage over its whole input row; ReLU passes the bound on.
cut, sel: as in fused_reference.

fp_mlp_inputs builds a case's data by that file's recipe: a clustered known cloud, unknown points scattered about known points (three
unequal non-zero distances) except one that coincides with a known point (dist = 0: the 1e-8 / 1e-10 floors), idx / dist from a float64
brute-force search rounded to fp32, features and weights with a positive mean."""
import functools

import torch

from tests import fused_reference as fr
from tests import group_mlp_reference as gr

RULES = ("given", "pointnet2", "flownet3d")
BLEND_ROUNDINGS = {"given": 3.0, "pointnet2": 10.0, "flownet3d": 10.0}
EPS_POINTNET2 = float(torch.tensor(1e-8, dtype=torch.float32).double())
FLOOR_FLOWNET3D = float(torch.tensor(1e-10, dtype=torch.float32).double())
CLUSTER = 16
COINCIDENT = 7   # this unknown point of every element lies on a known point


def blend_weights(dist, rule, w3=None):
    """(w, used) in the precision of `dist` (fp32: the torch statement of the kernel's rule; float64: the exact weights): weights
    (B,n,3) and which slots' rows are read."""
    if rule == "given":
        return w3.to(dist.dtype), torch.ones_like(dist, dtype=torch.bool)
    used = torch.isfinite(dist)
    if rule == "pointnet2":
        den = dist + (EPS_POINTNET2 if dist.dtype == torch.float64 else 1e-8)
    elif rule == "flownet3d":
        den = (dist * dist).clamp_min(FLOOR_FLOWNET3D if dist.dtype == torch.float64 else 1e-10)
    else:
        raise ValueError(rule)
    recip = torch.where(used, 1.0 / den, torch.zeros_like(den))
    norm = (recip[..., 0:1] + recip[..., 1:2]) + recip[..., 2:3]
    some = norm > 0
    return torch.where(some, recip / torch.where(some, norm, torch.ones_like(norm)), torch.zeros_like(recip)), used


def fp_mlp_reference(known_feats, skip, idx, dist, weights, rule="pointnet2", w3=None, sel=None, cut=None, block=256):
    """known_feats (B,m,C2), skip (B,n,C1) or None, idx (B,n,3), dist (B,n,3) fp32 (None under "given"), weights [(W, b), ...] with
    W (out, in) over the row [blend (C2) | skip (C1)], w3 (B,n,3) under "given"."""
    B, n, _ = idx.shape
    w_all, used_all = blend_weights(w3.double() if rule == "given" else dist.double(), rule, w3)

    def blk(b, i):
        j = idx[b, i].long()                                              # (P, 3)
        w, used = w_all[b, i], used_all[b, i]
        f = known_feats[b[:, None], j].double()                           # (P, 3, C2)
        f = torch.where(used[..., None], f, torch.zeros_like(f))
        terms = w[..., None] * f
        x = (terms[:, 0] + terms[:, 1]) + terms[:, 2]
        xb = BLEND_ROUNDINGS[rule] * terms.abs().sum(1)
        if skip is not None and skip.shape[-1]:
            s = skip[b, i].double()
            x, xb = torch.cat([x, s], -1), torch.cat([xb, torch.zeros_like(s)], -1)
        for wl, bias in weights:
            z, xb = fr.product_stage(x, xb, wl, bias, cut)
            x = torch.relu(z)
        return x, xb

    return fr._run(blk, B * n, n, sel, block)


def three_nn_float64(unknown, known):
    """(dist (B,n,3) fp32, idx (B,n,3) int32): the three nearest known points by a float64 brute-force search, distances (square
    roots) rounded to fp32."""
    d2 = (unknown.double()[:, :, None] - known.double()[:, None]).square().sum(-1)
    val, pos = torch.topk(d2, 3, dim=2, largest=False, sorted=True)
    return val.sqrt().float().contiguous(), pos.int().contiguous()


@functools.lru_cache(maxsize=None)
def _inputs(b, n, m, c2, c1, widths):
    g = torch.Generator().manual_seed(b * 7919 + n * 31 + m + 131 * c2 + 17 * c1 + sum(widths))
    known = fr.clustered_cloud(g, b, m, CLUSTER)
    home = torch.arange(n) * m // n
    unknown = (known[:, home] + 0.3 * torch.randn(b, n, 3, generator=g)).contiguous()
    unknown[:, COINCIDENT] = known[:, home[COINCIDENT]]
    dist, idx = three_nn_float64(unknown, known)
    assert (dist[:, COINCIDENT, 0] == 0).all() and (dist[:, :, 1] > 0).all()
    known_feats = torch.randn(b, m, c2, generator=g) + 0.5
    skip = (torch.randn(b, n, c1, generator=g) + 0.5) if c1 else None
    w3 = torch.rand(b, n, 3, generator=g) + 0.1
    w3 = (w3 / w3.sum(-1, keepdim=True)).contiguous()
    ws = gr.mlp_weights(g, c2 + c1, list(widths))
    return dict(unknown=unknown, known=known, known_feats=known_feats, skip=skip, idx=idx, dist=dist, w3=w3, weights=ws)


def fp_mlp_inputs(case):
    """unknown (b,n,3), known (b,m,3), known_feats (b,m,c2), skip (b,n,c1) or None, idx / dist (b,n,3), w3 (b,n,3) (positive,
    normalised: the weights of rule "given"), weights [(W, b), ...].  case: b, n, m, c2, c1, widths.  Built once per case; the
    tensors are shared among the tests and must be left unchanged."""
    return _inputs(case["b"], case["n"], case["m"], case["c2"], case["c1"], tuple(case["widths"]))


def composition(known_feats, skip, idx, dist, weights, rule="pointnet2", w3=None):
    """The layer in fp32 torch: weights by the rule, gathered rows, rounded products in the kernel's sum order, cat, 1x1 convolutions
    with ReLU -> (B, n, C_out)."""
    F = torch.nn.functional
    w, used = blend_weights(w3 if rule == "given" else dist, rule, w3)
    bi = torch.arange(idx.shape[0], device=idx.device)[:, None, None]
    f = known_feats[bi, idx.long()]                                       # (B, n, 3, C2)
    f = torch.where(used[..., None], f, torch.zeros_like(f))
    terms = w[..., None] * f
    x = (terms[:, :, 0] + terms[:, :, 1]) + terms[:, :, 2]
    if skip is not None and skip.shape[-1]:
        x = torch.cat([x, skip], -1)
    h = x.transpose(1, 2).unsqueeze(-1).contiguous()                      # (B, C_in, n, 1)
    for wl, bias in weights:
        h = torch.relu(F.conv2d(h, wl[:, :, None, None], bias))
    return h.squeeze(-1).transpose(1, 2)
