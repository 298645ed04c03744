"""Float64 statement of the train-mode fusion layer on a PADDED batch with per-cloud lengths (csrc/fusion_bn_lengths.hip):
fusion_bn_reference.layer restated with a live mask.  Point p of element b is live iff p < lens[b]; the statistics of every layer run
over the m = 64 * sum(lens) rows of live points only (sums divided by max(m, 1)), out is zero on padded points and so is the upstream
gradient.  A plain module: test_fusion_bn_lengths_reference_cpu.py checks it against fusion_bn_reference.layer on the compacted
clouds, test_fusion_bn_lengths_gpu.py checks the kernels against it.

The data of a case dict(b, n, lens, seed): element e with lens[e] > 0 is fused_reference.fusion_inputs(dict(b=1, n=lens[e], seed=...))
-- a cloud of its own size whose lists point into itself, so a live point's neighbours are live -- placed in rows 0 .. lens[e]-1 of
the padded tensors; padded rows hold zeros here (the GPU test poisons them).  The conv weights are those of the draw
fusion_inputs(dict(b=b, n=n, seed=...)), the affine is fusion_bn_reference's (gamma = 1 + 0.2 N(0,1), beta = 0.2 N(0,1), seeded).

The clear rule is fusion_bn_reference.bn_clear, applied to the live points; every case must keep more than 0.85 of its live points
clear and all of them at 8 live points or fewer (test_fusion_bn_lengths_reference_cpu.py); if a seed falls below, the seed changes."""
from dataclasses import dataclass, field

import torch

from tests import fused_reference as fr
from tests import fusion_bn_reference as br

LEAVES, WIDTHS, EPS = br.LEAVES, br.WIDTHS, br.EPS

# The cases of test_fusion_bn_lengths_gpu.py.  The grid caps are kernel_variants.bn_launch_grid's at 256 CUs, on the PADDED total
# b * n: the narrow passes (B2, B3) are capped at 256 workgroups = 1024 points, the wide ones at 512 = 2048 points.
CASES = [
    dict(tag="one-point", b=1, n=1, lens=(1,)),                    # m = 64: every variance zero, three dead waves
    dict(tag="empty-middle", b=3, n=40, lens=(40, 0, 17)),         # an empty element between two live ones; the second workgroup round-robin
    dict(tag="no-live-point", b=2, n=5, lens=(0, 0)),              # m = 0: divisions by max(m, 1), no shift
    dict(tag="ragged-tail", b=2, n=64, lens=(61, 64)),             # a padded tail of three points inside a workgroup's deal
    dict(tag="first-point-padded", b=2, n=9, lens=(0, 7)),         # the shift must come from element 1, not from the padded point 0
    dict(tag="over-narrow-cap", b=3, n=400, lens=(300, 0, 333)),   # padded total 1200 > 1024 (B2 / B3 capped), live total 633 below it
    dict(tag="over-both-caps", b=3, n=1100, lens=(1100, 3, 1000)), # padded 3300 and live 2103 above both caps (2048); one nearly empty element
]


def case_id(c):
    return f"fusion_bn_lengths[{c['tag']},b={c['b']},n={c['n']},lens={'-'.join(str(v) for v in c['lens'])}]"


def live_mask(case):
    b, n = case["b"], case["n"]
    return torch.arange(n).view(1, n) < torch.tensor(case["lens"]).view(b, 1).clamp(0, n)


def case_inputs(case):
    """(the 14 leaves in the order of LEAVES, padded, CPU fp32; the two list halves (b, n, 32) int32; the live mask (b, n))."""
    b, n, seed = case["b"], case["n"], case.get("seed", 0)
    _, _, _, ws = fr.fusion_inputs(dict(b=b, n=n, seed=seed))
    p1, p2 = torch.zeros(b, n, 3), torch.zeros(b, n, 3)
    ia, ib = torch.zeros(b, n, 32, dtype=torch.int32), torch.zeros(b, n, 32, dtype=torch.int32)
    for e, ln in enumerate(case["lens"]):
        if ln > 0:
            q1, q2, (ja, jb), _ = fr.fusion_inputs(dict(b=1, n=ln, seed=seed + 17 * (e + 1)))
            p1[e, :ln], p2[e, :ln], ia[e, :ln], ib[e, :ln] = q1[0], q2[0], ja[0].int(), jb[0].int()
    g = torch.Generator().manual_seed(7021 + 1000 * b + n + seed)
    aff = [t for c in WIDTHS for t in (1.0 + 0.2 * torch.randn(c, generator=g), 0.2 * torch.randn(c, generator=g))]
    return [p1, p2, *ws, *aff], (ia, ib), live_mask(case)


def layer(leaves, idx, live):
    """leaves in the order of LEAVES (any floating dtype), idx (B, N, 64) long, live (B, N) bool -> fusion_bn_reference.Evaluated with
    out (B * N, 3), zero on padded points, and pre / z3 over the LIVE points only, in padded order ((M, 64, C))."""
    p1, p2, *rest = leaves
    conv, aff = rest[:6], rest[6:]
    B, N, _ = p1.shape
    eb, ep = live.nonzero(as_tuple=True)                                       # the live points, in padded order
    nb = p2[eb.view(-1, 1), idx[eb, ep]]                                       # (M, 64, 3)
    r = nb - p1[eb, ep].unsqueeze(1)
    x = torch.cat([r, torch.linalg.vector_norm(r, dim=-1, keepdim=True)], -1)
    rows = max(64 * eb.numel(), 1)
    mean, var, pre, z = [], [], [], None
    for i in range(3):
        z = x @ conv[2 * i].T + conv[2 * i + 1]
        flat = z.reshape(-1, z.shape[-1])
        m = flat.sum(0) / rows
        v = (flat - m).square().sum(0) / rows
        y = (z - m) * (aff[2 * i] * torch.rsqrt(v + EPS)) + aff[2 * i + 1]
        mean.append(m)
        var.append(v)
        pre.append(y)
        x = torch.relu(y)
    blend = (torch.softmax(x.amax(-1), -1).unsqueeze(-1) * nb).sum(1)          # (M, 3)
    out = torch.zeros(B * N, 3, dtype=p1.dtype).index_put((eb * N + ep,), blend)
    return br.Evaluated(out, mean, var, pre, z)


@dataclass
class Prepared:
    case: dict
    names: list
    leaves: list          # CPU fp32, padded rows zero
    idx: object           # the two halves, int32
    live: torch.Tensor    # (B, N) bool
    flat: torch.Tensor    # (M,) the live points' flat indices b * N + p, in padded order
    ev: object            # float64, detached; pre / z3 over the live points
    dead: torch.Tensor    # (M, 64) bool
    clear: torch.Tensor   # (M,) bool
    g: torch.Tensor       # (B * N, 3) float64, zero on padded points and where not clear
    _graph: object = field(default=None, repr=False)

    @property
    def live_points(self):
        return int(self.flat.numel())

    def clear_points(self):
        """flat indices of the clear live points"""
        return self.flat[self.clear]

    def release(self):
        self._graph = None


def prepare(case):
    leaves, idx, live = case_inputs(case)
    whole = fr._whole(idx).long()
    with torch.no_grad():
        ev = layer([t.double() for t in leaves], whole, live)
    flat = live.reshape(-1).nonzero().flatten()
    clear = br.bn_clear(ev.pre) if flat.numel() else torch.zeros(0, dtype=torch.bool)
    dead = br.dead_neighbours(ev.pre[2]) if flat.numel() else torch.zeros(0, 64, dtype=torch.bool)
    g = torch.zeros(case["b"] * case["n"], 3, dtype=torch.float64)
    draw = torch.randn(case["b"] * case["n"], 3, generator=torch.Generator().manual_seed(99)).double()   # fp32 values
    g[flat[clear]] = draw[flat[clear]]
    return Prepared(case, list(LEAVES), leaves, idx, live, flat, ev, dead, clear, g)


def gradients(prep, sel=None):
    """One float64 gradient per leaf of <layer(leaves).out, g> with g restricted to the flat points `sel` (default: all of it)."""
    if prep._graph is None:
        l64 = [t.double().clone().requires_grad_(True) for t in prep.leaves]
        prep._graph = (l64, layer(l64, fr._whole(prep.idx).long(), prep.live).out)
    l64, out = prep._graph
    g = prep.g
    if sel is not None:
        g = torch.zeros_like(prep.g)
        sel = torch.as_tensor(sel, dtype=torch.long)
        g[sel] = prep.g[sel]
    return [torch.zeros_like(t) if r is None else r for t, r in zip(l64, torch.autograd.grad(out, l64, g, retain_graph=True, allow_unused=True))]


def _stats(z):
    flat = z.reshape(-1, z.shape[-1])
    m = flat.mean(0)
    return m, (flat - m).square().mean(0)


def stats3_without_last(prep):
    """(mean, biased variance) of layer 3 over every live row except the 64 of the LAST live point."""
    return _stats(prep.ev.z3[:-1])


def stats3_with_padded(prep, centre, neighbours):
    """(mean, biased variance) of layer 3 with the 64 rows of one PADDED point counted in: the point at `centre` (3,) with the
    neighbour coordinates `neighbours` (64, 3) (finite garbage), through layers 1 and 2 on the true statistics."""
    l = [t.double() for t in prep.leaves]
    conv, aff = l[2:8], l[8:]
    r = neighbours.double() - centre.double()
    x = torch.cat([r, torch.linalg.vector_norm(r, dim=-1, keepdim=True)], -1)
    for i in range(2):
        z = x @ conv[2 * i].T + conv[2 * i + 1]
        x = torch.relu((z - prep.ev.mean[i]) * (aff[2 * i] * torch.rsqrt(prep.ev.var[i] + EPS)) + aff[2 * i + 1])
    z3 = x @ conv[4].T + conv[5]
    return _stats(torch.cat([prep.ev.z3.reshape(-1, 128), z3], 0))


def exact_zero(prep, name):
    """fusion_bn_reference.exact_zero for the live points: conv biases always; with ONE live point that is all of its own neighbours
    everything but p2's gradient; with no live point everything."""
    return name in br.CONV_BIASES or prep.live_points == 0 or (prep.live_points == 1 and name != "p2")
