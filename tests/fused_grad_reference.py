"""Float64 gradients of the fused point layers (csrc/fusion_grad.hip, cross_grad.hip, cross256_grad.hip, pointconv_grad.hip,
ptblock_grad.hip): the layers of tests/fused_reference.py stated once more as plain differentiable float64 torch, differentiated by
torch.autograd on the CPU in blocks of points.  A plain module: test_fused_grad_reference_cpu.py checks it against the unfused twins of
mocopci_amd/grad.py in float64, test_fused_grad_variants_gpu.py checks the backward kernels against it.

The test data of a case is fused_reference's (fusion_inputs, cross_inputs, pointconv_inputs, ptblock_inputs): clustered clouds, data
with a positive mean, and `extent` / `same` / `dup` / `packed` / `logits` as for the forward.

prepare(case) -> Prepared: the leaves (CPU fp32, in the order of LEAVES[op]), the neighbour list, the `clear` mask and the upstream
gradient g (float64, zero where not clear).  gradients(prep, sel) -> one float64 gradient per leaf of <layer(leaves), g> restricted to
the flat points `sel` (default: all) -- with sel = [p] the contribution of point p, which the parity test adds to or takes from the
whole to state a point counted twice or dropped.

clear: where the arg-max neighbour (cross), the arg-max channel (fusion) or a ReLU / LeakyReLU branch is decided by rounding, the
kernel's forward bits and float64 may choose differently; either choice is a valid subgradient, but the two gradients then differ by
O(1) in that entry.  Those points -- (point, channel) pairs in cross -- are found here in float64 by the rules test_grad_gpu.py and
test_cross256_grad_gpu.py have always used (fusion_clear, cross_clear, ptblock_clear below; those tests import them) and get a zero
upstream gradient on both sides.  PointConv has no rule (it never had one).  Equal maxima between two list positions that hold
the SAME neighbour are not unclear: the kernels give the gradient to the lowest position, amax() splits it evenly, and both send it
to the same row.  |r| = 0 in fusion takes the zero subgradient on both sides (torch's norm; fusion_grad.hip:364).
Every case must keep more than 0.9 of its mask, a case of 8 points or fewer all of it (test_fused_grad_reference_cpu.py)."""
from dataclasses import dataclass

import torch

from tests import fused_reference as fr

LEAVES = {
    "fusion": ["p1", "p2", "w1", "b1", "w2", "b2", "w3", "b3"],
    "cross": ["xyz1", "xyz2", "points1", "points2", "wpos", "bpos", "wmlp", "bmlp"],
    "pointconv_agg": ["s_xyz", "new_xyz", "points", "w0", "b0", "w1", "b1", "w2", "b2"],
    "ptblock": ["xyz", "q", "k", "v", "wd1", "bd1", "wd2", "bd2", "wg1", "bg1", "wg2", "bg2"],
}
POINT_LEAVES = {"fusion": 2, "cross": 4, "pointconv_agg": 3, "ptblock": 4}   # the first leaves are per-point tensors, the rest weights and biases
LARGEST_WEIGHT = {"fusion": "w3", "cross": "wmlp", "pointconv_agg": "w2", "ptblock": "wd2"}   # ptblock: the 64 x 64 matrix that is never zero
BLOCK = {"fusion": 1024, "cross": 256, "pointconv_agg": 1024, "ptblock": 2048}


# ---- the clear rules (moved here from test_grad_gpu.py and test_cross256_grad_gpu.py, unchanged) ---------------------------------------
def fusion_clear(x3):
    """x3 (..., 64, 128): float64 layer-3 activations of every neighbour -> (...): no neighbour's two largest channels within rounding."""
    top2 = x3.topk(2, dim=-1).values
    return ((top2[..., 0] - top2[..., 1]) > 1e-4 * (1.0 + top2[..., 0])).all(dim=-1)


def cross_clear(u, z):
    """u, z (..., K, D): float64 u and z = Wmlp LeakyReLU(u) + bmlp over K DISTINCT neighbours -> (..., D): the channel's two largest z are
    apart, its maximum is off LeakyReLU's kink, and no u of the point is on the kink."""
    top2 = z.topk(2, dim=-2).values
    clear = ((top2[..., 0, :] - top2[..., 1, :]) > 1e-4 * (1.0 + top2[..., 0, :].abs())) & (top2[..., 0, :].abs() > 1e-5)
    return clear & (u.abs().amin(dim=(-2, -1)) > 1e-5).unsqueeze(-1)


def ptblock_clear(d1, a1):
    """d1, a1 (..., 16, 64): float64 inputs of fc_delta's and fc_gamma's ReLU -> (...): none on the kink."""
    return (d1.abs().amin(dim=(-2, -1)) > 1e-5) & (a1.abs().amin(dim=(-2, -1)) > 1e-5)


# ---- the layers: block functions (leaves, idx, batch ids, point ids) -> (out (P, C), what the clear rule reads) ---------------------------
def _fusion(leaves, idx, b, i):
    p1, p2, *ws = leaves
    nb = p2[b[:, None], idx[b, i]]                                       # (P, 64, 3)
    resi = nb - p1[b, i][:, None]
    x = torch.cat([resi, torch.linalg.vector_norm(resi, dim=-1, keepdim=True)], -1)   # zero subgradient at |r| = 0
    for w, bias in zip(ws[0::2], ws[1::2]):
        x = torch.relu(x @ w.T + bias)
    out = (torch.softmax(x.amax(-1), 1).unsqueeze(-1) * nb).sum(1)
    return out, lambda: fusion_clear(x.detach()).unsqueeze(-1)


def _cross(leaves, idx, b, i):
    xyz1, xyz2, f1, f2, wpos, bpos, wmlp, bmlp = leaves
    j = idx[b, i]
    u = (f2[b[:, None], j] + f1[b, i][:, None]) + ((xyz2[b[:, None], j] - xyz1[b, i][:, None]) @ wpos.T + bpos)
    z = fr.leaky(u, 0.1) @ wmlp.T + bmlp                                # (P, 32, D)

    def clear():
        repeat = (j[:, :, None] == j[:, None, :]).tril(-1).any(-1)        # a list position that holds an earlier position's neighbour
        return cross_clear(u.detach(), z.detach().masked_fill(repeat.unsqueeze(-1), float("-inf")))
    return fr.leaky(z, 0.1).amax(1), clear


def _pointconv_agg(leaves, idx, b, i):
    s_xyz, new_xyz, pts, *wn = leaves
    j = idx[b, i]
    g = s_xyz[b[:, None], j] - new_xyz[b, i][:, None]                   # (P, 32, 3)
    w = g
    for ww, bias in zip(wn[0::2], wn[1::2]):
        w = torch.relu(w @ ww.T + bias)
    out = torch.cat([g, pts[b[:, None], j]], -1).transpose(1, 2) @ w     # (P, 3 + D, 8)
    return out.flatten(1), lambda: torch.ones(len(b), 1, dtype=torch.bool)


def _ptblock(leaves, idx, b, i):
    xyz, q, k, v, wd1, bd1, wd2, bd2, wg1, bg1, wg2, bg2 = leaves
    j = idx[b, i]
    d1 = (xyz[b, i][:, None] - xyz[b[:, None], j]) @ wd1.T + bd1        # (P, 16, 64)
    delta = torch.relu(d1) @ wd2.T + bd2
    a1 = ((q[b, i][:, None] - k[b[:, None], j]) + delta) @ wg1.T + bg1
    attn = torch.relu(a1) @ wg2.T + bg2
    out = (torch.softmax(attn / 8.0, 1) * (v[b[:, None], j] + delta)).sum(1)
    return out, lambda: ptblock_clear(d1.detach(), a1.detach()).unsqueeze(-1)


LAYER = {"fusion": _fusion, "cross": _cross, "pointconv_agg": _pointconv_agg, "ptblock": _ptblock}


def case_inputs(case):
    """(leaves in the order of LEAVES[op], neighbour list as fused_reference builds it) -- CPU fp32."""
    op = case["op"]
    if op == "fusion":
        p1, p2, idx, ws = fr.fusion_inputs(case)
        return [p1, p2, *ws], idx
    if op == "cross":
        xyz1, xyz2, f1, f2, idx, w = fr.cross_inputs(case)
        return [xyz1, xyz2, f1, f2, *w], idx
    if op == "pointconv_agg":
        s_xyz, new_xyz, pts, idx, wn, _ = fr.pointconv_inputs(case)
        return [s_xyz, new_xyz, pts, *wn], idx
    if op == "ptblock":
        xyz, q, k, v, idx, ws = fr.ptblock_inputs(case)
        return [xyz, q, k, v, *ws], idx
    raise ValueError(f"unknown op {op}")


def centres(case):
    """(batch elements, centres per element): the flat point p is centre p % n of element p // n."""
    return case["b"], case[{"fusion": "n", "cross": "n1", "pointconv_agg": "s", "ptblock": "n"}[case["op"]]]


@dataclass
class Prepared:
    case: dict
    names: list
    leaves: list          # CPU fp32
    idx: object           # a tensor, or the two halves
    clear: torch.Tensor   # (points, C or 1) bool
    g: torch.Tensor       # (points, C) float64, zero where not clear

    @property
    def total(self):
        return self.g.shape[0]

    def clear_points(self):
        """Flat indices of the points with a non-zero upstream gradient."""
        return self.clear.any(-1).nonzero().flatten()


def _leaves64(prep, grad):
    return [t.double().clone().requires_grad_(grad) for t in prep.leaves]


def prepare(case):
    leaves, idx = case_inputs(case)
    b, n = centres(case)
    prep = Prepared(case, LEAVES[case["op"]], leaves, idx, None, None)
    l64, whole, layer = _leaves64(prep, False), fr._whole(idx).long(), LAYER[case["op"]]
    clear, width = [], None
    with torch.no_grad():
        for s in fr._blocks(b * n, None, BLOCK[case["op"]]):
            out, rule = layer(l64, whole, s // n, s % n)
            clear.append(rule())
            width = out.shape[1]
    prep.clear = torch.cat(clear)
    g = torch.randn(b * n, width, generator=torch.Generator().manual_seed(99)).double()    # fp32 values: the kernels get the same numbers
    prep.g = g * prep.clear
    return prep


def gradients(prep, sel=None):
    """One float64 gradient per leaf of sum over the flat points `sel` of <layer(point), g[point]>."""
    b, n = centres(prep.case)
    l64, whole, layer = _leaves64(prep, True), fr._whole(prep.idx).long(), LAYER[prep.case["op"]]
    acc = [torch.zeros_like(t) for t in l64]
    for s in fr._blocks(b * n, sel, BLOCK[prep.case["op"]]):
        out, _ = layer(l64, whole, s // n, s % n)
        for a, x in zip(acc, torch.autograd.grad(out, l64, prep.g[s], allow_unused=True)):
            if x is not None:
                a += x
    return acc


def exact_zero(case, name):
    """Gradients that are zero in exact arithmetic (the kernels and float64 both return rounding noise there; the parity test allows
    them the project's absolute floor): fc_gamma's last bias shifts every neighbour's logit of a channel alike, so the softmax over
    the neighbours does not see it; with one neighbour 16 times (same) the softmax is uniform whatever the logits, so nothing reaches
    fc_gamma or q or k -- so too with one point that is its own 16 neighbours, where moreover every relative coordinate is zero (nothing
    for fc_delta's first matrix) and the centre's and the neighbours' coordinate gradients cancel; in fusion one point that is all of its
    own neighbours blends to that point whatever the weights and wherever p1 is."""
    if case["op"] == "ptblock":
        one = case["b"] * case["n"] == 1
        return name == "bg2" or ((one or bool(case.get("same"))) and name in ("q", "k", "wg1", "bg1", "wg2")) or (one and name in ("xyz", "wd1"))
    if case["op"] == "fusion":
        return case["b"] * case["n"] == 1 and name != "p2"
    return False


def gather(t, idx):
    """The plain row gather the twins of mocopci_amd/grad.py take as G: t (B, N, C), idx (B, ..., K) -> (B, ..., K, C)."""
    return t[torch.arange(t.shape[0]).view(-1, *([1] * (idx.dim() - 1))), idx.long()]
