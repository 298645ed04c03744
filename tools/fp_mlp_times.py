"""Device times of the fused feature-propagation layer against the composition (device events after warm-up; medians of --reps (25)
single launches with min and max, the rows of one level alternating per repetition in one process).

Levels, each at B = 8 on the LiDAR-like box of mocopci_amd.synth (known points = the cloud's first m rows), random features, a
PointnetFPModule with non-trivial BatchNorm statistics:
  fp_top   n = 16384, m = 1024, 256 + 3   -> 256/256        (FeaturePropagation(256, 3, [256, 256]) of models/models.py)
  fp_mid   n = 1024,  m = 256,  256 + 128 -> 256/256        (a PointNet++ SSG segmentation level)
  fp_low   n = 4096,  m = 1024, 128 + 4   -> 128/128/128
Rows per level:
  a   composition        the module with route = "never" under no-grad in eval(): three_nn, the weights in torch, three_interpolate,
                         cat, Conv2d + BatchNorm2d + ReLU per layer; timed twice per rotation, as its first row and, as
                         composition_again, as its last
  b   fused              the module with route = "always": three_nn, the two (B,C,n) -> (B,n,C) transpositions, mcp_fp_mlp, the
                         transposed view of the result
  b'  fused_channel_last three_nn + mcp_fp_mlp on channel-last features (a caller that keeps them so)
  c   fp_mlp             mcp_fp_mlp alone
Recorded with the numbers: fused_wins = b's median is below a's by more than a's own max - min -- the condition for routing the
level's shape class to the fused route (ops.FP_MLP_FUSED_CLASSES); and the largest |b - a| of the two results.
`--level NAME` measures one level (each level in a process of its own, under the caller's time limit); `--out FILE` merges the level
into that JSON document."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mocopci_amd import ops, pointnet2_utils as pu, synth  # noqa: E402
from mocopci_amd.pointnet2_modules import PointnetFPModule  # noqa: E402

LEVELS = {"fp_top": (8, 16384, 1024, 256, 3, (256, 256)), "fp_mid": (8, 1024, 256, 256, 128, (256, 256)),
          "fp_low": (8, 4096, 1024, 128, 4, (128, 128, 128))}
DEV = "cuda:0"


def timed(fn):
    s, e = torch.cuda.Event(True), torch.cuda.Event(True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def stats(v):
    v = sorted(v)
    return {"median_ms": round(v[len(v) // 2], 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4)}


def alternate(runs, reps):
    for _ in range(3):
        for fn in runs.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in runs}
    for _ in range(reps):
        for name, fn in runs.items():
            times[name].append(timed(fn))
    return {name: stats(v) for name, v in times.items()}


def module(g, c2, c1, widths):
    m = PointnetFPModule(mlp=[c2 + c1, *widths])
    state = {}
    for k, v in m.state_dict().items():
        shape = list(v.shape)
        if k.endswith("conv.weight"):
            state[k] = 2.0 * (torch.randn(shape, generator=g) + 1.0) / shape[1]
        elif k.endswith("num_batches_tracked"):
            state[k] = torch.tensor(3)
        elif k.endswith("running_var") or k.endswith("bn.weight"):
            state[k] = torch.rand(shape, generator=g) + 0.5
        else:
            state[k] = torch.randn(shape, generator=g) * 0.1 - 0.1
    m.load_state_dict(state, strict=True)
    return m.to(DEV).eval()


def measure(name, reps):
    B, n, m, c2, c1, widths = LEVELS[name]
    be = ops.HipBackend()
    g = torch.Generator().manual_seed(7)
    unknown = synth.make_batch(1, B, n)[0].permute(0, 2, 1).contiguous().to(DEV)
    known = unknown[:, :m].contiguous()
    feats = (torch.randn(B, c2, m, generator=g) + 0.5).to(DEV)
    skip = (torch.randn(B, c1, n, generator=g) + 0.5).to(DEV)
    rows, srows = feats.transpose(1, 2).contiguous(), skip.transpose(1, 2).contiguous()
    mod = module(g, c2, c1, widths)
    packed, wl = mod._packed_weights(c2)
    dist, idx = pu.three_nn(unknown, known)
    res = {}

    def composition():
        mod.route = "never"
        res["a"] = mod(unknown, known, skip, feats)

    def fused():
        mod.route = "always"
        res["b"] = mod(unknown, known, skip, feats)

    def fused_channel_last():
        d, i = pu.three_nn(unknown, known)
        be.fp_mlp(rows, srows, i, d, packed, wl)

    with torch.no_grad():
        runs = {"composition": composition, "fused": fused, "fused_channel_last": fused_channel_last,
                "fp_mlp": lambda: be.fp_mlp(rows, srows, idx, dist, packed, wl)}
        runs["composition_again"] = composition
        row = alternate(runs, reps)
    a, b = row["composition"], row["fused"]
    return {"level": name, "B": B, "n": n, "m": m, "c2": c2, "c1": c1, "widths": list(widths), "reps": reps,
            "weights_in_lds": ops.fp_mlp_weights_in_lds(c2, c1, widths), "tmax": ops.fp_mlp_tmax(widths), **row,
            "fused_over_composition": round(b["median_ms"] / a["median_ms"], 4),
            "composition_spread_ms": round(a["max_ms"] - a["min_ms"], 4),
            "fused_wins": b["median_ms"] < a["median_ms"] - (a["max_ms"] - a["min_ms"]),
            "max_abs_difference": float((res["a"] - res["b"]).abs().max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
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
