"""Float64 gradients of the feature-propagation layer (csrc/fp_mlp_grad.hip): the layer of tests/fp_mlp_reference.py stated as plain
differentiable float64 torch and differentiated by torch.autograd on the CPU, in the form of tests/fused_grad_reference.py.  A plain
module: test_fp_mlp_grad_cpu.py checks it against autograd over fp_mlp_reference.composition, test_fp_mlp_grad_gpu.py checks the
backward kernel against it.

Data: fp_mlp_reference's inputs of the case (clouds, idx / dist, features, w3) with OTHER weights.  The forward tests' weights have a
positive mean and leave 95 - 100 % of the ReLUs active at every width >= 64, so a backward that ignored the masks would pass; here
W ~ sqrt(2 / cin) randn and b ~ 0.1 randn, which leave about half of the units of every layer active (test_fp_mlp_grad_cpu.py holds
every hidden layer of every case between 0.25 and 0.75).  A case with fewer unknown points than fp_mlp_reference can build (its
coincident point is number 7) takes the first n of 8.

prepare(case, rule) -> Prepared: the leaves (CPU fp32: known_feats, skip when C1 > 0, then W1, b1, ...), the `clear` mask over the
flat rows and the upstream gradient g (float64 holding fp32 values, zero where not clear).  gradients(prep, sel) -> one float64
gradient per leaf of the sum over the flat rows `sel` (default: all) of <layer(row), g[row]>; with sel = [p] the contribution of row
p, which a test adds to or takes from the whole to state a row counted twice or dropped.  masks_one=True states the mutant whose
backward ignores the ReLU masks (every derivative 1, forward values unchanged).

clear: a row is clear when every float64 pre-activation of every layer satisfies |z| > 1e-4; where a ReLU branch is decided by
rounding the kernel's bits and float64 may choose differently, and the two gradients then differ by O(1) in that unit.  Unclear rows
get a zero upstream gradient on both sides.  dist, w3 and the coordinates are constants: the layer gives them no gradient."""
import functools
from dataclasses import dataclass

import torch

from tests import fp_mlp_reference as fpr

CLEAR = 1e-4
FLOOR = 2e-5          # absolute tolerance of a gradient that is zero in exact arithmetic (this project's floor)
SMALLEST_N = fpr.COINCIDENT + 1


def sign_mixed_weights(g, cin, widths):
    out = []
    for w in widths:
        out.append((torch.randn(w, cin, generator=g) * (2.0 / cin) ** 0.5, 0.1 * torch.randn(w, generator=g)))
        cin = w
    return out


@functools.lru_cache(maxsize=None)
def _inputs(b, n, m, c2, c1, widths):
    d = dict(fpr.fp_mlp_inputs(dict(b=b, n=max(n, SMALLEST_N), m=m, c2=c2, c1=c1, widths=list(widths))))
    if n < SMALLEST_N:
        for k in ("unknown", "skip", "idx", "dist", "w3"):
            d[k] = None if d[k] is None else d[k][:, :n].contiguous()
    g = torch.Generator().manual_seed(5 + b * 7919 + n * 31 + m + 131 * c2 + 17 * c1 + sum(widths))
    d["weights"] = sign_mixed_weights(g, c2 + c1, list(widths))
    return d


def grad_inputs(case):
    """fp_mlp_reference.fp_mlp_inputs(case) with the sign-mixed weights.  Built once per case; shared, to be left unchanged."""
    return _inputs(case["b"], case["n"], case["m"], case["c2"], case["c1"], tuple(case["widths"]))


@dataclass
class Prepared:
    data: dict
    rule: str
    names: list
    leaves: list            # CPU fp32
    clear: torch.Tensor     # (rows,) bool
    g: torch.Tensor         # (rows, C_out) float64, zero where not clear
    active: list            # per layer: fraction of (row, unit) pairs with z > 0

    @property
    def has_skip(self):
        return self.names[1] == "skip"

    def point_leaves(self):
        return 2 if self.has_skip else 1

    def largest_weight(self):
        sizes = {k: t.numel() for k, t in zip(self.names, self.leaves) if k.startswith("w")}
        return self.names.index(max(sizes, key=sizes.get))


def leaf_names(d):
    names = ["known_feats"] + (["skip"] if d["skip"] is not None else [])
    for l in range(len(d["weights"])):
        names += [f"w{l + 1}", f"b{l + 1}"]
    return names


def layer(leaves, d, rule, sel, masks_one=False):
    """The layer over the flat rows `sel` from float64 leaves -> (out (P, C_out), [z_l (P, width_l)])."""
    has_skip = d["skip"] is not None
    feats, skip, wb = leaves[0], leaves[1] if has_skip else None, leaves[2 if has_skip else 1:]
    n = d["idx"].shape[1]
    src = d["w3"].double() if rule == "given" else d["dist"].double()
    w_all, used_all = fpr.blend_weights(src, rule, d["w3"])
    b, i = sel // n, sel % n
    w, used = w_all[b, i], used_all[b, i]
    f = feats[b[:, None], d["idx"][b, i].long()]                          # (P, 3, C2)
    f = torch.where(used[..., None], f, torch.zeros_like(f))
    terms = w[..., None] * f
    x = (terms[:, 0] + terms[:, 1]) + terms[:, 2]
    if has_skip:
        x = torch.cat([x, skip[b, i]], -1)
    zs = []
    for wl, bias in zip(wb[0::2], wb[1::2]):
        z = x @ wl.T + bias
        zs.append(z)
        x = z + (torch.relu(z) - z).detach() if masks_one else torch.relu(z)
    return x, zs


def _leaves64(prep, grad):
    return [t.double().clone().requires_grad_(grad) for t in prep.leaves]


def prepare(case=None, rule="pointnet2", data=None, rows=None):
    """data: the case's grad_inputs unless given (the lengths tests hand in searched idx / dist); rows: the live flat rows (default:
    all) -- every other row is left out of `clear`."""
    d = grad_inputs(case) if data is None else data
    leaves = [d["known_feats"]] + ([d["skip"]] if d["skip"] is not None else []) + [t for pair in d["weights"] for t in pair]
    prep = Prepared(d, rule, leaf_names(d), leaves, None, None, None)
    total = d["idx"].shape[0] * d["idx"].shape[1]
    sel = torch.arange(total) if rows is None else torch.as_tensor(rows, dtype=torch.long)
    with torch.no_grad():
        out, zs = layer(_leaves64(prep, False), d, rule, sel)
    clear = torch.zeros(total, dtype=torch.bool)
    clear[sel] = torch.stack([(z.abs() > CLEAR).all(-1) for z in zs]).all(0)
    prep.clear = clear
    prep.active = [float((z > 0).double().mean()) for z in zs]
    g = torch.randn(total, out.shape[1], generator=torch.Generator().manual_seed(99)).double()   # fp32 values: the kernel gets the same numbers
    prep.g = g * clear[:, None]
    return prep


def gradients(prep, sel=None, masks_one=False):
    """One float64 gradient per leaf of the sum over the flat rows `sel` of <layer(row), g[row]>."""
    sel = prep.clear.nonzero().flatten() if sel is None else torch.as_tensor(sel, dtype=torch.long)
    l64 = _leaves64(prep, True)
    out, _ = layer(l64, prep.data, prep.rule, sel, masks_one)
    got = torch.autograd.grad(out, l64, prep.g[sel], allow_unused=True)
    return [torch.zeros_like(t) if x is None else x for t, x in zip(l64, got)]


def ratio(got, exact, c):
    """max |got - exact| / (c max |exact|); a gradient that is zero in exact arithmetic is held to FLOOR instead."""
    scale = exact.abs().max().item()
    tol = c * scale if scale > 0 else FLOOR
    return (got.double() - exact).abs().max().item() / tol
