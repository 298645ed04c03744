"""Device times of the set-abstraction layer's forward + backward under train() with BatchNorm: the composition against the fused
route with batch statistics (device events after warm-up; medians of --reps (15) alternating runs with min and max, in one process
per level).

The three levels of tools/group_mlp_times.py at B = 8, the same clouds, centres (the cloud's first M rows, handed in as new_xyz: no
sampling is timed), features and module as tools/group_mlp_grad_times.py, in train(), with the features and every parameter asking
for a gradient and a fixed upstream gradient:
  a  composition   the module with bn_route = "never": QueryAndGroup (ball query, one-launch grouping), Conv2d + BatchNorm2d (batch
                   statistics, running-statistics update) + ReLU per layer over the (B, 3 + C, M, nsample) tensor, the pool, and
                   autograd's backward over them; timed twice per rotation, as its first row and, as composition_again, as its last.
                   This is the parent's code and the yardstick.
  b  fused         the module with bn_route = "always": ball query, the transposition, the operand image, mcp_group_mlp_bn_forward,
                   the running-statistics update, and in the backward the operand image, the segment sort and
                   mcp_group_mlp_bn_backward (the forward passes again, the pool's backward, the layer passes, scatters, weight sums)
Recorded with the numbers: fused_wins = b's median is below a's by more than a's own max - min -- the condition for a row in
ops.GROUP_MLP_BN_FUSED_CLASSES; the largest relative difference of any gradient between the two routes; workspace_bytes of the two
entry points and, per route, the device memory the forward leaves allocated for the backward (kept_bytes).
`--level NAME` measures one level; `--out FILE` merges the level into that JSON document."""
import argparse
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from group_mlp_grad_times import module  # noqa: E402
from group_mlp_times import DEV, LEVELS, alternate  # noqa: E402
from mocopci_amd import _lib, synth  # noqa: E402


def measure(name, reps):
    B, N, M, radius, nsample, C, widths = LEVELS[name]
    g = torch.Generator().manual_seed(7)
    xyz = synth.make_batch(1, B, N)[0].permute(0, 2, 1).contiguous().to(DEV)
    centres = xyz[:, :M].contiguous()
    feats = (torch.randn(B, C, N, generator=g) + 0.5).to(DEV).requires_grad_(True)
    upstream = torch.randn(B, widths[-1], M, generator=g).to(DEV)
    mod = module(g, M, radius, nsample, C, widths).train()
    leaves = [feats, *mod.parameters()]
    res, kept = {}, {}

    def both(route, key):
        def run():
            mod.bn_route = route
            before = torch.cuda.memory_allocated()
            out = mod(xyz, feats, new_xyz=centres)[1]
            kept[key] = torch.cuda.memory_allocated() - before
            res[key] = torch.autograd.grad(out, leaves, upstream)
        return run

    runs = {"composition": both("never", "a"), "fused": both("always", "b"), "composition_again": both("never", "a")}
    row = alternate(runs, reps)
    a, b = row["composition"], row["fused"]
    apart = max(float((x - y).abs().max() / y.abs().max().clamp_min(1e-30)) for x, y in zip(res["b"], res["a"]))
    wid = (ctypes.c_int * len(widths))(*widths)
    need = [int(_lib.load().mcp_group_mlp_bn_workspace_bytes(B, M, C, nsample, 1, len(widths), wid, back)) for back in (0, 1)]
    return {"level": name, "B": B, "N": N, "M": M, "radius": radius, "nsample": nsample, "C": C, "widths": list(widths), "reps": reps, **row,
            "fused_over_composition": round(b["median_ms"] / a["median_ms"], 4),
            "composition_spread_ms": round(a["max_ms"] - a["min_ms"], 4),
            "fused_wins": b["median_ms"] < a["median_ms"] - (a["max_ms"] - a["min_ms"]),
            "max_relative_difference": apart,
            "workspace_bytes_forward": need[0], "workspace_bytes_backward": need[1],
            "kept_bytes_composition": int(kept["a"]), "kept_bytes_fused": int(kept["b"])}


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
