"""Device times of the feature-propagation layer's forward + backward under train() with BatchNorm: the composition against the
fused route with batch statistics (device events after warm-up; medians of --reps (15) alternating runs with min and max, in one
process per level).

The three levels of tools/fp_mlp_times.py at B = 8, the same clouds, features and module as tools/fp_mlp_grad_times.py, in train(),
with unknow_feats, known_feats and every parameter asking for a gradient and a fixed upstream gradient:
  a  composition   the module with bn_route = "never": three_nn, the weights in torch, three_interpolate, cat, Conv2d + BatchNorm2d
                   (batch statistics, running-statistics update) + ReLU per layer, and autograd's backward over them; timed twice
                   per rotation, as its first row and, as composition_again, as its last.  This is the parent's code and the yardstick.
  b  fused         the module with bn_route = "always": three_nn, the transpositions, the operand image, mcp_fp_mlp_bn_forward, the
                   running-statistics update, and in the backward the operand image and mcp_fp_mlp_bn_backward (the forward passes
                   again, the layer passes, scatter, weight sums)
Recorded with the numbers: fused_wins = b's median is below a's by more than a's own max - min -- the condition for a row in
ops.FP_MLP_BN_FUSED_CLASSES; and the largest relative difference of any gradient between the two routes.
`--level NAME` measures one level; `--out FILE` merges the level into that JSON document."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fp_mlp_times import DEV, LEVELS, alternate, module  # noqa: E402
from mocopci_amd import ops, synth  # noqa: E402


def measure(name, reps):
    B, n, m, c2, c1, widths = LEVELS[name]
    g = torch.Generator().manual_seed(7)
    unknown = synth.make_batch(1, B, n)[0].permute(0, 2, 1).contiguous().to(DEV)
    known = unknown[:, :m].contiguous()
    feats = (torch.randn(B, c2, m, generator=g) + 0.5).to(DEV).requires_grad_(True)
    skip = (torch.randn(B, c1, n, generator=g) + 0.5).to(DEV).requires_grad_(True)
    upstream = torch.randn(B, widths[-1], n, generator=g).to(DEV)
    mod = module(g, c2, c1, widths).train()
    leaves = [skip, feats, *mod.parameters()]
    res = {}

    def both(route, key):
        def run():
            mod.bn_route = route
            res[key] = torch.autograd.grad(mod(unknown, known, skip, feats), leaves, upstream)
        return run

    runs = {"composition": both("never", "a"), "fused": both("always", "b"), "composition_again": both("never", "a")}
    row = alternate(runs, reps)
    a, b = row["composition"], row["fused"]
    apart = max(float((x - y).abs().max() / y.abs().max().clamp_min(1e-30)) for x, y in zip(res["b"], res["a"]))
    return {"level": name, "B": B, "n": n, "m": m, "c2": c2, "c1": c1, "widths": list(widths), "reps": reps,
            "weights_in_lds": ops.fp_mlp_grad_weights_in_lds(c2, c1, widths), "tmax": ops.fp_mlp_tmax(widths), **row,
            "fused_over_composition": round(b["median_ms"] / a["median_ms"], 4),
            "composition_spread_ms": round(a["max_ms"] - a["min_ms"], 4),
            "fused_wins": b["median_ms"] < a["median_ms"] - (a["max_ms"] - a["min_ms"]),
            "max_relative_difference": apart}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--level", choices=sorted(LEVELS), action="append")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    doc = {"device": torch.cuda.get_device_name(0), "levels": {}}
    if a.out and os.path.exists(a.out):
        doc = json.load(open(a.out))
    for name in a.level or sorted(LEVELS):
        doc["levels"][name] = measure(name, a.reps)
    text = json.dumps(doc, indent=1)
    print(text, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
