"""Device times of the fused set-abstraction layer against the composition (device events after warm-up; medians of --reps (25) single
launches with min and max, the rows of one level alternating per repetition in one process).

Levels: the three set-abstraction levels of bench.py --config c4 that mcp_group_mlp supports, on the LiDAR-like box of
mocopci_amd.synth, centres = the cloud's first M rows, random features and folded weights:
  sa1   B = 8, N = 16384 -> M = 1024, radius 0.5, nsample 16, C = 4,   widths 32/32/64
  sa2   B = 8, N = 1024  -> M = 256,  radius 1,   nsample 16, C = 64,  widths 64/64/128
  sa3   B = 8, N = 256   -> M = 64,   radius 2,   nsample 8,  C = 128, widths 128/128/256
Rows per level:
  a   composition        the layer as the modules compose it: one-launch mcp_query_and_group on (B,C,N) features, three folded
                         1x1 convolutions with ReLU (library kernels), max over the neighbours; timed twice per rotation, as its
                         first row and, as composition_again, as its last
  b   fused              what the modules' fused route runs: (B,C,N) -> (B,N,C) transposition of the features, ball query,
                         mcp_group_mlp, transposition of the result
  b'  fused_channel_last ball query + mcp_group_mlp on channel-last features (a caller that keeps them so)
  c   group_mlp          mcp_group_mlp alone
Recorded with the numbers: fused_wins = b's median is below a's by more than a's own max - min -- the condition for routing the
level's shape class to the fused route (ops.GROUP_MLP_FUSED_CLASSES); and the largest |b - a| of the two results.
`--level NAME` measures one level (each level in a process of its own, under the caller's time limit); `--out FILE` merges the level
into that JSON document."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mocopci_amd import ops, pointnet2_utils as pu, synth  # noqa: E402

LEVELS = {"sa1": (8, 16384, 1024, 0.5, 16, 4, (32, 32, 64)), "sa2": (8, 1024, 256, 1.0, 16, 64, (64, 64, 128)),
          "sa3": (8, 256, 64, 2.0, 8, 128, (128, 128, 256))}
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


def measure(name, reps):
    B, N, M, radius, nsample, C, widths = LEVELS[name]
    be = ops.HipBackend()
    g = torch.Generator().manual_seed(7)
    xyz = synth.make_batch(1, B, N)[0].permute(0, 2, 1).contiguous().to(DEV)
    centres = xyz[:, :M].contiguous()
    feats = (torch.randn(B, C, N, generator=g) + 0.5).to(DEV)
    rows = feats.transpose(1, 2).contiguous()
    ws, cin = [], 3 + C
    for w in widths:
        ws.append(((2.0 * (torch.randn(w, cin, generator=g) + 1.0) / cin).to(DEV), (torch.randn(w, generator=g) * 0.1 - 0.2).to(DEV)))
        cin = w
    packed, wl = ops.group_mlp_pack_weights(ws)
    grouper = pu.QueryAndGroup(radius, nsample, use_xyz=True)
    kernels = [(w[:, :, None, None].contiguous(), b) for w, b in ws]
    idx = be.ball_query(xyz, centres, radius, nsample)
    res = {}

    def composition():
        h = grouper(xyz, centres, feats)
        for w, b in kernels:
            h = torch.relu_(torch.nn.functional.conv2d(h, w, b))
        res["a"] = h.amax(3)

    def fused():
        r = feats.transpose(1, 2).contiguous()
        i = be.ball_query(xyz, centres, radius, nsample)
        res["b"] = be.group_mlp(xyz, centres, r, i, packed, wl).transpose(1, 2).contiguous()

    def fused_channel_last():
        be.group_mlp(xyz, centres, rows, be.ball_query(xyz, centres, radius, nsample), packed, wl)

    with torch.no_grad():
        runs = {"composition": composition, "fused": fused, "fused_channel_last": fused_channel_last,
                "group_mlp": lambda: be.group_mlp(xyz, centres, rows, idx, packed, wl)}
        runs["composition_again"] = composition
        row = alternate(runs, reps)
    a, b = row["composition"], row["fused"]
    return {"level": name, "B": B, "N": N, "M": M, "radius": radius, "nsample": nsample, "C": C, "widths": list(widths), "reps": reps,
            "weights_in_lds": ops.group_mlp_weights_in_lds(C, widths), **row,
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
