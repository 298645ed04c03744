"""Float64 statement of the attentive fusion layer on BATCH statistics (csrc/fusion_bn.hip; MultiFrameEstimatier.fusion in net.train()
mode, mocopci.py:803-819 with nn.BatchNorm2d(eps 1e-3) in training mode), as plain differentiable torch over the WHOLE call -- the
statistics of a layer run over all b * n * 64 rows, so the layer cannot be evaluated in blocks of points as fused_grad_reference.py
does.  A plain module: test_fusion_bn_reference_cpu.py checks it against a composition built on torch's own batch_norm and against
the unfused path of model.fusion_batch_stats in float64, test_fusion_bn_variants_gpu.py checks the kernels against it.

layer(leaves, idx) is written once for every dtype and device: in float64 on the CPU it is the reference, in float32 on the device it
is the yardstick printed beside every figure (nothing is asserted on it).

    [r, |r|] (zero subgradient at |r| = 0: torch's norm)  ->  three times conv, BatchNorm on the batch's mean and BIASED variance, ReLU
    ->  channel maximum, softmax over the 64 neighbours, blend of the neighbour coordinates.

The data of a case is fused_reference.fusion_inputs(case) (the clouds, lists and conv weights of the eval-mode cases) plus an affine
drawn from a seeded generator, gamma = 1 + 0.2 N(0, 1), beta = 0.2 N(0, 1); the `far` case takes the weights of
test_grad_gpu.test_fusion_batch_statistics_of_a_channel_far_from_its_bias instead.

prepare(case) -> Prepared: the 14 leaves (CPU fp32, in the order of LEAVES), the list, the float64 evaluation (out, per-layer mean and
biased variance, the BatchNorm outputs the clear rule reads, the layer-3 conv output), the dead-neighbour mask, the `clear` mask and
the upstream gradient g (float64, zero where not clear).  gradients(prep, sel) builds ONE autograd graph per case and reuses it: the
gradient is linear in the upstream gradient, so the contribution of point p is the gradient of g masked to p.

clear: a point keeps its upstream gradient iff
  (a) no layer-1 or layer-2 BatchNorm output of any of its neighbours is within 1e-5 of zero (a ReLU decided by rounding), and
  (b) every neighbour either has its two largest layer-3 activations apart by fusion_clear's rule with the winner's pre-ReLU value more
      than 1e-5 from zero, or is DEAD: all 128 pre-ReLU values below -1e-5.  A dead neighbour is not ambiguous -- its score is the
      floor 0 on both sides and both sides give it a zero gradient (the kernel through its `score > 0` gate, autograd through ReLU) --
      but fusion_clear alone rejects it (0 - 0 is not apart), and with it the 3- and 5-point cases would keep nothing.
Every case must keep more than 0.85 of its points, a case of 8 points or fewer all of them (test_fusion_bn_reference_cpu.py); if a seed
falls below, the seed changes, not the cap."""
from dataclasses import dataclass, field

import torch

from tests import fused_reference as fr
from tests.fused_grad_reference import fusion_clear

LEAVES = ["p1", "p2", "w1", "b1", "w2", "b2", "w3", "b3", "gamma1", "beta1", "gamma2", "beta2", "gamma3", "beta3"]
POINT_LEAVES = 2                 # p1, p2; then the conv weights and biases, then the affine
CONV_BIASES = ("b1", "b2", "b3")  # a bias in front of a batch-statistics BatchNorm: its gradient is zero in exact arithmetic
WIDTHS = (64, 64, 128)
EPS = 1e-3


def group(name):
    return "point" if name in ("p1", "p2") else "weight" if name[0] in "wb" and not name.startswith("beta") else "affine"


@dataclass
class Evaluated:
    out: torch.Tensor     # (points, 3)
    mean: list            # per layer (C,)
    var: list             # per layer (C,), biased
    pre: list             # per layer (points, 64, C): the BatchNorm output, before the ReLU
    z3: torch.Tensor      # (points, 64, 128): the layer-3 conv output, before the BatchNorm


def layer(leaves, idx):
    """leaves in the order of LEAVES (any floating dtype, any device), idx (B, N, 64) long -> Evaluated."""
    p1, p2, *rest = leaves
    conv, aff = rest[:6], rest[6:]
    B, N, _ = p1.shape
    nb = p2[torch.arange(B, device=p1.device).view(B, 1, 1), idx]              # (B, N, 64, 3)
    r = nb - p1.unsqueeze(2)
    x = torch.cat([r, torch.linalg.vector_norm(r, dim=-1, keepdim=True)], -1)
    mean, var, pre, z = [], [], [], None
    for i in range(3):
        z = x @ conv[2 * i].T + conv[2 * i + 1]
        flat = z.reshape(-1, z.shape[-1])
        m = flat.mean(0)
        v = (flat - m).square().mean(0)
        y = (z - m) * (aff[2 * i] * torch.rsqrt(v + EPS)) + aff[2 * i + 1]
        mean.append(m)
        var.append(v)
        pre.append(y.reshape(B * N, 64, -1))
        x = torch.relu(y)
    out = (torch.softmax(x.amax(-1), -1).unsqueeze(-1) * nb).sum(2)
    return Evaluated(out.reshape(B * N, 3), mean, var, pre, z.reshape(B * N, 64, -1))


def dead_neighbours(pre3):
    """(points, 64): every layer-3 BatchNorm output of the neighbour is below -1e-5, so its score is the floor 0."""
    return (pre3 < -1e-5).all(-1)


def bn_clear(pre):
    """pre: the three float64 BatchNorm outputs (points, 64, C) -> (points,) by the rule of the module docstring."""
    relus = (pre[0].abs().amin(dim=(1, 2)) > 1e-5) & (pre[1].abs().amin(dim=(1, 2)) > 1e-5)
    x3 = torch.relu(pre[2])
    top2 = x3.topk(2, dim=-1).values
    apart = (top2[..., 0] - top2[..., 1]) > 1e-4 * (1.0 + top2[..., 0])        # fusion_clear's rule, per neighbour
    decided = apart & (pre[2].amax(-1) > 1e-5)
    return relus & (decided | dead_neighbours(pre[2])).all(-1)


def _rnd(seed, *shape, scale=1.0):   # tests/test_grad_gpu.rnd
    return torch.randn(tuple(shape), generator=torch.Generator().manual_seed(seed)) * scale


def case_inputs(case):
    """(the 14 leaves in the order of LEAVES, the two list halves) -- CPU fp32."""
    p1, p2, idx, ws = fr.fusion_inputs(case)
    if case.get("far"):
        # test_fusion_batch_statistics_of_a_channel_far_from_its_bias: positive layer-2 weights on inputs that layer 1's BatchNorm
        # (gamma 0.06, beta 1) pins near 1
        ws = [_rnd(182, 64, 4, scale=0.5), _rnd(183, 64, scale=0.3), _rnd(184, 64, 64, scale=0.125).abs(), _rnd(185, 64, scale=0.3),
              _rnd(186, 128, 64, scale=0.125), _rnd(187, 128, scale=0.3)]
        aff = [torch.full((64,), 0.06), torch.ones(64), 1 + _rnd(170, 64, scale=0.2), _rnd(171, 64, scale=0.2),
               1 + _rnd(172, 128, scale=0.2), _rnd(173, 128, scale=0.2)]
    else:
        # 7021: the first offset at which every case keeps more than 0.85 of its points, the 3- and 5-point cases have dead neighbours
        # (104 of 192 and 179 of 320 rows) and so do the two largest cases (74450 of 131136 and 123529 of 197952 rows)
        g = torch.Generator().manual_seed(7021 + 1000 * case["b"] + case["n"] + case.get("seed", 0))
        aff = [t for c in WIDTHS for t in (1.0 + 0.2 * torch.randn(c, generator=g), 0.2 * torch.randn(c, generator=g))]
    return [p1, p2, *ws, *aff], idx


@dataclass
class Prepared:
    case: dict
    names: list
    leaves: list          # CPU fp32
    idx: object           # the two halves
    ev: Evaluated         # float64, detached
    dead: torch.Tensor    # (points, 64) bool
    clear: torch.Tensor   # (points, 1) bool
    g: torch.Tensor       # (points, 3) float64, zero where not clear
    _graph: object = field(default=None, repr=False)

    @property
    def total(self):
        return self.g.shape[0]

    def clear_points(self):
        return self.clear.any(-1).nonzero().flatten()

    def release(self):
        """Drop the autograd graph (2.9 GB at 3093 points)."""
        self._graph = None


def prepare(case):
    leaves, idx = case_inputs(case)
    whole = fr._whole(idx).long()
    with torch.no_grad():
        ev = layer([t.double() for t in leaves], whole)
    clear = bn_clear(ev.pre).unsqueeze(-1)
    g = torch.randn(ev.out.shape[0], 3, generator=torch.Generator().manual_seed(99)).double()   # fp32 values: the kernels get the same numbers
    return Prepared(case, list(LEAVES), leaves, idx, ev, dead_neighbours(ev.pre[2]), clear, g * clear)


def gradients(prep, sel=None):
    """One float64 gradient per leaf of <layer(leaves), g> with g restricted to the flat points `sel` (default: all of it)."""
    if prep._graph is None:
        l64 = [t.double().clone().requires_grad_(True) for t in prep.leaves]
        prep._graph = (l64, layer(l64, fr._whole(prep.idx).long()).out)
    l64, out = prep._graph
    g = prep.g
    if sel is not None:
        g = torch.zeros_like(prep.g)
        sel = torch.as_tensor(sel, dtype=torch.long)
        g[sel] = prep.g[sel]
    return list(torch.autograd.grad(out, l64, g, retain_graph=True))


def stats3_without(prep, p):
    """(mean, biased variance) of layer 3 in float64 over every row except the 64 of point p: what a statistics pass that dropped the
    point would return."""
    keep = torch.ones(prep.total, dtype=torch.bool)
    keep[p] = False
    flat = prep.ev.z3[keep].reshape(-1, prep.ev.z3.shape[-1])
    m = flat.mean(0)
    return m, (flat - m).square().mean(0)


def far_ratio(prep):
    """Per layer-2 channel |mean - conv bias| / sigma of the conv output, in float64."""
    return (prep.ev.mean[1] - prep.leaves[5].double()).abs() / prep.ev.var[1].sqrt()


def exact_zero(case, name):
    """Gradients that are zero in exact arithmetic: the conv biases always (BatchNorm subtracts the batch mean); with one point that
    is all of its own neighbours every row of every layer is the same row, so every variance is zero, every zhat is zero, the blend is
    that point whatever the weights and wherever p1 is -- everything but p2's gradient."""
    return name in CONV_BIASES or (case["b"] * case["n"] == 1 and name != "p2")
