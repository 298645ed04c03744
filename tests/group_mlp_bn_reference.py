"""Float64 statement of the set-abstraction layer under a training-mode BatchNorm (csrc/group_mlp_bn.hip) and of its gradients, by
torch.autograd over float64 leaves on the CPU.  A plain module: test_group_mlp_bn_cpu.py checks it against torch's own float64
composition (F.conv2d, F.batch_norm(training=True), ReLU, F.max_pool2d / F.avg_pool2d), test_group_mlp_bn_gpu.py checks the kernels
against it.

The layer, over the live pairs R = {(p, j): p a live centre, j < nsample} (count m), k = idx[p, j]:
    x = [xyz[k] - new_xyz[p] (use_xyz) | features[k]],  z_l = W_l h_(l-1) + b_l,  mu_l = mean_R z_l,  v_l = mean_R (z_l - mu_l)^2,
    y_l = gamma_l (z_l - mu_l) / sqrt(v_l + eps_l) + beta_l,  h_l = ReLU(y_l),  out[p] = max_j h_(L,j)  or  (sum_j h_(L,j)) / nsample.
The maximum is a gather of the LOWEST slot that attains it (group_mlp_grad_reference.layer's statement of F.max_pool2d's rule).

Inputs: group_mlp_reference.group_mlp_inputs(case) for the clouds, centres, neighbour lists and features;
fp_mlp_bn_reference._parameters' recipe for W, b, gamma in [1.5, 2.5] and beta.  Batch statistics couple the pairs, so a pair near
a ReLU kink cannot be masked out: pick() walks seeds from BASE_SEED until EVERY y_l of EVERY live pair is farther than CLEAR = 1e-4
from zero in float64, and no pair is left out.  Pool near-ties among DIFFERENT points can be isolated: the upstream gradient is zeroed
per (centre, channel) by group_mlp_grad_reference.clear_mask's rule on y_L; `kept` is the share that stays (the tests hold it above
0.9).  offset: added to the features (the cancellation case); biased=False: convolutions without a bias.

Mutants (forward's keywords), each a wrong kernel that the GPU test's bound must tell from the right one: stat_pad=k (the statistics
also count k further columns per centre that repeat slot 0, as a column group's padding would), unbiased=True (variance over m - 1),
ties="all" (the maximum's gradient to every tied slot), stats_const=True (the statistics treated as constants in the backward)."""
import functools
from dataclasses import dataclass

import torch

from tests import fp_mlp_bn_reference as fbr
from tests import group_mlp_grad_reference as ggr
from tests import group_mlp_reference as gr

CLEAR = fbr.CLEAR
BASE_SEED = 1000
TRIES = 400
EPS = 1e-5
FLOOR = ggr.FLOOR
N = 200


def case(c, nsample, widths, b=3, m=7, use_xyz=True, pool="max"):
    return dict(b=b, n=N, m=m, c=c, nsample=nsample, widths=list(widths), use_xyz=use_xyz, pool=pool)


def case_id(k):
    tail = ("" if k["use_xyz"] else "-noxyz") + ("" if k["pool"] == "max" else "-mean")
    return f"c{k['c']}-ns{k['nsample']}-{'x'.join(map(str, k['widths']))}-{k['b']}x{k['m']}{tail}"


@dataclass
class Prepared:
    data: dict              # xyz, new_xyz, features, idx (CPU), use_xyz, pool
    centres: torch.Tensor   # the live flat centres
    names: list
    leaves: list            # CPU fp32: features (c > 0), xyz and new_xyz (use_xyz), then per layer W, b (when biased), gamma, beta
    biased: bool
    layers: int
    eps: list
    g: torch.Tensor         # (B * M, C_out) float64 holding fp32 values, zero in padded centres and where the pool is not clear
    kept: float             # share of the live (centre, channel) entries whose upstream gradient is kept
    seed: int
    tries: int

    def point_leaves(self):
        return (1 if self.data["features"] is not None else 0) + (2 if self.data["use_xyz"] else 0)

    def layer_leaves(self, leaves):
        """[(W, b or None, gamma, beta), ...] out of a list shaped like `leaves`."""
        per = 4 if self.biased else 3
        rest = leaves[self.point_leaves():]
        out = []
        for l in range(self.layers):
            q = rest[per * l:per * (l + 1)]
            out.append((q[0], q[1], q[2], q[3]) if self.biased else (q[0], None, q[1], q[2]))
        return out

    def pairs(self):
        return len(self.centres) * self.data["idx"].shape[2]


def gather_rows(point_leaves, d, sel):
    """x (P, J, 3 + c) over the flat centres `sel`, position columns first (the module's order)."""
    t = dict(zip((["features"] if d["features"] is not None else []) + (["xyz", "new_xyz"] if d["use_xyz"] else []), point_leaves))
    m = d["idx"].shape[1]
    b, i = sel // m, sel % m
    j = d["idx"][b, i].long()
    parts = []
    if d["use_xyz"]:
        parts.append(t["xyz"][b[:, None], j] - t["new_xyz"][b, i][:, None])
    if d["features"] is not None:
        parts.append(t["features"][b[:, None], j])
    return torch.cat(parts, -1)


def forward(x, layers, eps, pool="max", ties="lowest", stat_pad=0, unbiased=False, stats_const=False):
    """(out (P, C_out), [y_l (P, J, width_l)], [(mu_l, v_l)]) of the stack over the pairs of x (P, J, cin), every pair live."""
    h, ys, stats = x, [], []
    for (w, b, gamma, beta), e in zip(layers, eps):
        z = h @ w.T
        if b is not None:
            z = z + b
        counted = torch.cat([z, z[:, :1].expand(-1, stat_pad, -1)], 1) if stat_pad else z
        rows = counted.shape[0] * counted.shape[1]
        mu = counted.mean((0, 1))
        v = (counted - mu).square().sum((0, 1)) / (rows - 1 if unbiased else rows)
        if stats_const:
            mu, v = mu.detach(), v.detach()
        y = gamma * ((z - mu) / torch.sqrt(v + e)) + beta
        ys.append(y)
        stats.append((mu, v))
        h = torch.relu(y)
    if pool == "max":
        top = h.detach()
        hit = top == top.amax(1, keepdim=True)
        weight = (hit if ties == "all" else hit & (hit.cumsum(1) == 1)).double()   # the lowest slot that attains the maximum
    else:
        weight = torch.full_like(h, 1.0 / h.shape[1])
    return (h * weight.to(h.dtype)).sum(1), ys, stats


def evaluate(prep, grad=False, **mutant):
    """Float64 leaves and (out, ys, stats) over the live centres."""
    l64 = [t.double().clone().requires_grad_(grad) for t in prep.leaves]
    x = gather_rows(l64[:prep.point_leaves()], prep.data, prep.centres)
    return l64, forward(x, prep.layer_leaves(l64), prep.eps, prep.data["pool"], **mutant)


def clear(prep):
    """The condition of every comparison: min over layers and live pairs of |y_l| > CLEAR."""
    with torch.no_grad():
        _, (_, ys, _) = evaluate(prep)
    return min(y.abs().min().item() for y in ys) > CLEAR


def pool_clear(prep):
    """(live centres, C_out) bool: group_mlp_grad_reference.clear_mask's rule of the last layer on y_L."""
    with torch.no_grad():
        _, (_, ys, _) = evaluate(prep)
    d, m = prep.data, prep.data["idx"].shape[1]
    return ggr.clear_mask(dict(pool="max" if d["pool"] == "max" else "mean"), [ys[-1]], d["idx"][prep.centres // m, prep.centres % m].long())


@functools.lru_cache(maxsize=None)
def _pick(key, offset, biased, lengths):
    k = dict(key)
    k["widths"] = list(k["widths"])
    xyz, new_xyz, feats, idx, _, _ = gr.group_mlp_inputs({x: k[x] for x in ("b", "n", "m", "c", "nsample", "widths", "use_xyz")})
    if offset and feats is not None:
        feats = feats + offset
    use_xyz, pool = k["use_xyz"], "max" if k["pool"] == "max" else "mean"
    d = dict(xyz=xyz, new_xyz=new_xyz, features=feats, idx=idx, use_xyz=use_xyz, pool=pool)
    b, m, widths = k["b"], k["m"], k["widths"]
    centres = torch.arange(b * m) if lengths is None else torch.cat([torch.arange(min(max(u, 0), m)) + i * m for i, u in enumerate(lengths)])
    names = (["features"] if feats is not None else []) + (["xyz", "new_xyz"] if use_xyz else [])
    for l in range(len(widths)):
        names += [f"w{l + 1}"] + ([f"b{l + 1}"] if biased else []) + [f"gamma{l + 1}", f"beta{l + 1}"]
    points = ([feats] if feats is not None else []) + ([xyz, new_xyz] if use_xyz else [])
    for t in range(TRIES):
        seed = BASE_SEED + t
        params, gen = fbr._parameters(seed, k["c"] + (3 if use_xyz else 0), widths, biased)
        prep = Prepared(d, centres, names, points + params, biased, len(widths), [EPS] * len(widths), None, 0.0, seed, t + 1)
        if not clear(prep):
            continue
        keep = pool_clear(prep)
        g = torch.zeros(b * m, widths[-1], dtype=torch.float64)
        g[centres] = torch.randn(len(centres), widths[-1], generator=gen).double() * keep
        prep.g, prep.kept = g, float(keep.double().mean())
        return prep
    raise AssertionError(f"no seed among {TRIES} keeps every y_l farther than {CLEAR} from zero")


def pick(k, offset=0.0, biased=True, lengths=None):
    """The first seed's Prepared whose every y_l is clear of zero.  Built once per argument set; shared, to be left unchanged."""
    key = tuple(sorted((x, tuple(v) if isinstance(v, list) else v) for x, v in k.items()))
    return _pick(key, float(offset), bool(biased), None if lengths is None else tuple(lengths))


_EXACT = {}


def gradients(prep, **mutant):
    """(out over the live centres, stats, one float64 gradient per leaf of <out, g>), optionally of a mutant."""
    l64, (out, _, stats) = evaluate(prep, grad=True, **mutant)
    grads = torch.autograd.grad(out, l64, prep.g[prep.centres], allow_unused=True)
    return out.detach(), [(mu.detach(), v.detach()) for mu, v in stats], [torch.zeros_like(t) if x is None else x for t, x in zip(l64, grads)]


def exact(prep):
    """(out (B * M, C_out) float64 with zeros in padded centres, [(mu_l, v_l)], m = the live pairs, one float64 gradient per leaf of
    <out, g>).  Computed once per Prepared."""
    hit = _EXACT.get(id(prep))
    if hit is None:
        out, stats, grads = gradients(prep)
        full = torch.zeros(prep.g.shape[0], out.shape[1], dtype=torch.float64)
        full[prep.centres] = out
        hit = _EXACT[id(prep)] = (prep, full, stats, prep.pairs(), grads)
    return hit[1:]


running_update = fbr.running_update
ratio = ggr.ratio
