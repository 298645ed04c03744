"""Float64 gradients of the set-abstraction layer (csrc/group_mlp_grad.hip): the layer of tests/group_mlp_reference.py stated as plain
differentiable float64 torch and differentiated by torch.autograd on the CPU, in the form of tests/fp_mlp_grad_reference.py.  A plain
module: test_group_mlp_grad_cpu.py checks it against autograd over group_mlp_reference.composition, test_group_mlp_grad_gpu.py checks
the backward kernel against it.

The maximum is stated as a gather of the LOWEST slot that attains it (F.max_pool2d's rule, the kernel's rule), never as amax, which
splits the gradient among tied slots: a ball query repeats its first hit, and the two-tile cases hold every point in two slots.

Data: group_mlp_reference.group_mlp_inputs(case) (clouds, centres, neighbour lists, features, the centre's own features) with OTHER
weights.  The forward tests' weights have a positive mean and leave nearly every ReLU active, so a backward that ignored the masks
would pass; here W ~ sqrt(2 / cin) randn and b ~ 0.1 randn, which leave about half of the units of every layer active
(test_group_mlp_grad_cpu.py holds every layer of every case between 0.25 and 0.75).  In the FlowEmbedding form (c2 > 0) the columns of
W1 over the centre's features are not part of the layer: the kernel receives their product as row_bias, and so does the reference --
row_bias = centre W1[:, -c2:]^T rounded to fp32 is a leaf, W1[:, :-c2] is the first weight.

prepare(case) -> Prepared: the leaves (CPU fp32: features when c > 0, xyz and new_xyz with use_xyz, row_bias when c2 > 0, then W1,
b1, ...), the `clear` mask per (centre, channel) and the upstream gradient g (float64 holding fp32 values, zero where not clear).
gradients(prep, sel) -> one float64 gradient per leaf of the sum over the flat centres `sel` (default: all) of <layer(centre),
g[centre]>; with sel = [p] the contribution of centre p, which a test adds to or takes from the whole to state a centre counted twice
or dropped.  Mutants: masks_one=True (the backward ignores the ReLU masks: every derivative 1, forward values and winners unchanged),
ties="all" (the maximum's gradient goes to EVERY slot that attains it), pad=k (k further columns that repeat slot 0, as the kernel's
column group holds them, take part in the pool's gradient).

clear, per (centre, channel): every hidden pre-activation of every slot of the centre satisfies |z| > 1e-5 -- where a ReLU branch is
decided by rounding, the kernel's bits and float64 may choose differently -- and, at the last layer, for the maximum
fused_grad_reference.cross_clear's rule among DIFFERENT points (the top value beats the best value of every slot that holds another
point by more than 1e-4 (1 + |top|), and |top| > 1e-5; equal values in slots that repeat the winner's point are the same number on
both sides and do not make a channel unclear), for the mean |z| > 1e-5 in every slot of that channel.  The upstream gradient is zero
where not clear, on both sides."""
import functools
from dataclasses import dataclass

import torch

from tests import group_mlp_reference as gr

KINK = 1e-5
FLOOR = 2e-5          # absolute tolerance of a gradient that is zero in exact arithmetic (this project's floor)


def sign_mixed_weights(g, cin, widths):
    out = []
    for w in widths:
        out.append((torch.randn(w, cin, generator=g) * (2.0 / cin) ** 0.5, 0.1 * torch.randn(w, generator=g)))
        cin = w
    return out


@functools.lru_cache(maxsize=None)
def _inputs(key):
    case = dict(key)
    case["widths"] = list(case["widths"])
    xyz, new_xyz, feats, idx, centre, _ = gr.group_mlp_inputs(case)
    use_xyz, c, c2 = case.get("use_xyz", True), case["c"], case.get("c2", 0)
    g = torch.Generator().manual_seed(case.get("seed", 5) + sum(case["widths"]) + c + case["nsample"])
    ws = sign_mixed_weights(g, (3 if use_xyz else 0) + c + c2, case["widths"])
    row_bias = None
    if c2:
        w1, b1 = ws[0]
        row_bias = (centre.double() @ w1[:, -c2:].double().T).float().contiguous()
        ws[0] = (w1[:, :-c2].contiguous(), b1)
    return dict(xyz=xyz, new_xyz=new_xyz, features=feats, idx=idx, row_bias=row_bias, weights=ws, use_xyz=use_xyz, pool=case.get("pool", "max"))


def grad_inputs(case):
    """group_mlp_reference.group_mlp_inputs(case) with the sign-mixed weights and row_bias.  Built once per case; shared, to be left
    unchanged."""
    return _inputs(tuple(sorted((k, tuple(v) if isinstance(v, list) else v) for k, v in case.items())))


@dataclass
class Prepared:
    data: dict
    names: list
    leaves: list            # CPU fp32
    clear: torch.Tensor     # (centres, C_out) bool
    g: torch.Tensor         # (centres, C_out) float64, zero where not clear
    active: list            # per layer: fraction of (pair, unit) with z > 0
    dead: float             # max pool: fraction of pooled entries <= 0 (their winner is masked)

    def point_leaves(self):
        return sum(1 for n in self.names if n[0] not in "wb")

    def largest_weight(self):
        sizes = {k: t.numel() for k, t in zip(self.names, self.leaves) if k.startswith("w")}
        return self.names.index(max(sizes, key=sizes.get))


def leaf_names(d):
    names = (["features"] if d["features"] is not None else []) + (["xyz", "new_xyz"] if d["use_xyz"] else [])
    names += ["row_bias"] if d["row_bias"] is not None else []
    for l in range(len(d["weights"])):
        names += [f"w{l + 1}", f"b{l + 1}"]
    return names


def leaf_list(d):
    named = dict(features=d["features"], xyz=d["xyz"], new_xyz=d["new_xyz"], row_bias=d["row_bias"])
    return [named[n] for n in leaf_names(d) if n in named] + [t for pair in d["weights"] for t in pair]


def layer(leaves, d, sel, masks_one=False, ties="lowest", pad=0):
    """The layer over the flat centres `sel` from float64 leaves (in leaf_names' order) -> (out (P, C_out), [z_l (P, J, width_l)])."""
    names = leaf_names(d)
    t = dict(zip(names, leaves))
    m = d["idx"].shape[1]
    b, i = sel // m, sel % m
    j = d["idx"][b, i].long()                                            # (P, J)
    parts = []
    if d["use_xyz"]:
        parts.append(t["xyz"][b[:, None], j] - t["new_xyz"][b, i][:, None])
    if d["features"] is not None:
        parts.append(t["features"][b[:, None], j])
    x = torch.cat(parts, -1)
    zs = []
    for l in range(len(d["weights"])):
        z = x @ t[f"w{l + 1}"].T + t[f"b{l + 1}"]
        if l == 0 and d["row_bias"] is not None:
            z = z + t["row_bias"][b, i][:, None]
        zs.append(z)
        x = z + (torch.relu(z) - z).detach() if masks_one else torch.relu(z)
    J = x.shape[1]
    if d["pool"] == "max":
        h = torch.relu(zs[-1]).detach()
        hit = h == h.amax(1, keepdim=True)
        pick = hit if ties == "all" else hit & (hit.cumsum(1) == 1)      # the lowest slot that attains the maximum
        weight = pick.double()
    else:
        weight = torch.full_like(x, 1.0 / J)
    if pad:                                                              # the column group's further columns repeat slot 0
        weight = weight.clone()
        weight[:, 0] = weight[:, 0] * (1 + pad)
    return (x * weight).sum(1), zs


def _leaves64(prep, grad):
    return [t.double().clone().requires_grad_(grad) for t in prep.leaves]


def clear_mask(d, zs, j):
    """(P, C_out) from the float64 pre-activations zs [(P, J, width_l)] and the neighbour lists j (P, J)."""
    hidden = torch.ones(j.shape[0], dtype=torch.bool)
    for z in zs[:-1]:
        hidden &= (z.abs() > KINK).all(-1).all(-1)
    z = zs[-1]
    if d["pool"] == "max":
        top, arg = z.max(1)                                              # (P, C)
        win_pt = torch.gather(j[..., None].expand(-1, -1, z.shape[-1]), 1, arg[:, None]).squeeze(1)
        other = z.masked_fill(j[..., None] == win_pt[:, None], float("-inf")).amax(1)
        last = ((top - other) > 1e-4 * (1 + top.abs())) & (top.abs() > KINK)
    else:
        last = (z.abs() > KINK).all(1)
    return last & hidden[:, None]


def prepare(case=None, data=None, centres=None):
    """data: the case's grad_inputs unless given (the searched-list and lengths tests hand in their own idx); centres: the live flat
    centres (default: all) -- every other centre is left out of `clear`."""
    d = grad_inputs(case) if data is None else data
    prep = Prepared(d, leaf_names(d), leaf_list(d), None, None, None, 0.0)
    total = d["idx"].shape[0] * d["idx"].shape[1]
    sel = torch.arange(total) if centres is None else torch.as_tensor(centres, dtype=torch.long)
    with torch.no_grad():
        out, zs = layer(_leaves64(prep, False), d, sel)
    m = d["idx"].shape[1]
    clear = torch.zeros(total, out.shape[1], dtype=torch.bool)
    clear[sel] = clear_mask(d, zs, d["idx"][sel // m, sel % m].long())
    prep.clear = clear
    prep.active = [float((z > 0).double().mean()) for z in zs]
    prep.dead = float((out <= 0).double().mean()) if d["pool"] == "max" else 0.0
    g = torch.randn(total, out.shape[1], generator=torch.Generator().manual_seed(99)).double()   # fp32 values: the kernel gets the same numbers
    prep.g = g * clear
    return prep


def clear_centres(prep):
    """The flat centres with at least one clear channel."""
    return prep.clear.any(1).nonzero().flatten()


def gradients(prep, sel=None, **mutant):
    """One float64 gradient per leaf of the sum over the flat centres `sel` of <layer(centre), g[centre]>."""
    sel = clear_centres(prep) if sel is None else torch.as_tensor(sel, dtype=torch.long)
    l64 = _leaves64(prep, True)
    out, _ = layer(l64, prep.data, sel, **mutant)
    got = torch.autograd.grad(out, l64, prep.g[sel], allow_unused=True)
    return [torch.zeros_like(t) if x is None else x for t, x in zip(l64, got)]


def ratio(got, exact, c):
    """max |got - exact| / (c max |exact|); a gradient that is zero in exact arithmetic is held to FLOOR instead."""
    scale = exact.abs().max().item()
    tol = c * scale if scale > 0 else FLOOR
    return (got.double() - exact).abs().max().item() / tol
