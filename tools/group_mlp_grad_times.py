"""Device times of the set-abstraction layer's forward + backward: the composition against the fused differentiable route (device
events after warm-up; medians of --reps (15) alternating runs with min and max, in one process per level).

The three levels of tools/group_mlp_times.py at B = 8, the same clouds, centres (the cloud's first M rows, handed in as new_xyz: no
sampling is timed) and features, through PointnetSAModule in eval() with non-trivial BatchNorm statistics; features and every
parameter ask for a gradient, the upstream gradient is fixed:
  a  composition   the module with grad_route = "never": QueryAndGroup (ball query, one-launch grouping), Conv2d + BatchNorm2d + ReLU
                   per layer over the (B, 3 + C, M, nsample) tensor, the pool, and autograd's backward over them; timed twice per
                   rotation, as its first row and, as composition_again, as its last.  This is the parent's code and the yardstick.
  b  fused         the module with grad_route = "always": ball query, the transposition, the differentiable fold, mcp_group_mlp, and
                   in the backward the operand image, mcp_group_mlp_grad (kernel, segment sort, scatters, weight sums) and autograd
                   through the fold
Recorded with the numbers: fused_wins = b's median is below a's by more than a's own max - min -- the condition for a row in
ops.GROUP_MLP_GRAD_FUSED_CLASSES; the largest relative difference of any gradient between the two routes; workspace_bytes of
mcp_group_mlp_grad (the dense per-pair intermediate the backward writes) and, per route, the device memory the forward leaves
allocated for the backward (kept_bytes: torch.cuda.memory_allocated after the forward minus before it).
`--level NAME` measures one level; `--out FILE` merges the level into that JSON document."""
import argparse
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from group_mlp_times import DEV, LEVELS, alternate  # noqa: E402
from mocopci_amd import _lib, ops, synth  # noqa: E402
from mocopci_amd.pointnet2_modules import PointnetSAModule  # noqa: E402


def module(g, M, radius, nsample, C, widths):
    mod = PointnetSAModule(mlp=[C, *widths], npoint=M, radius=radius, nsample=nsample, bn=True)
    state = {}
    for k, v in mod.state_dict().items():
        shape = list(v.shape)
        if k.endswith("conv.weight"):
            state[k] = torch.randn(shape, generator=g) * (2.0 / shape[1]) ** 0.5
        elif k.endswith("num_batches_tracked"):
            state[k] = torch.tensor(3)
        elif k.endswith("running_var") or k.endswith("bn.weight"):
            state[k] = torch.rand(shape, generator=g) + 0.5
        else:
            state[k] = torch.randn(shape, generator=g) * 0.1
    mod.load_state_dict(state, strict=True)
    return mod.to(DEV).eval()


def measure(name, reps):
    B, N, M, radius, nsample, C, widths = LEVELS[name]
    g = torch.Generator().manual_seed(7)
    xyz = synth.make_batch(1, B, N)[0].permute(0, 2, 1).contiguous().to(DEV)
    centres = xyz[:, :M].contiguous()
    feats = (torch.randn(B, C, N, generator=g) + 0.5).to(DEV).requires_grad_(True)
    upstream = torch.randn(B, widths[-1], M, generator=g).to(DEV)
    mod = module(g, M, radius, nsample, C, widths)
    leaves = [feats, *mod.parameters()]
    res, kept = {}, {}

    def both(route, key):
        def run():
            mod.grad_route = route
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
    return {"level": name, "B": B, "N": N, "M": M, "radius": radius, "nsample": nsample, "C": C, "widths": list(widths), "reps": reps,
            "weights_in_lds": ops.group_mlp_grad_weights_in_lds(C, widths), **row,
            "fused_over_composition": round(b["median_ms"] / a["median_ms"], 4),
            "composition_spread_ms": round(a["max_ms"] - a["min_ms"], 4),
            "fused_wins": b["median_ms"] < a["median_ms"] - (a["max_ms"] - a["min_ms"]),
            "max_relative_difference": apart,
            "workspace_bytes": int(_lib.load().mcp_group_mlp_grad_workspace_bytes(B, M, C, nsample, 1, len(widths), wid)),
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
