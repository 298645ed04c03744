"""Device times of the batch-statistics BatchNorm of the per-point attention blocks, forward + backward, at the shapes the blocks see in
`bench.py --train-step train` (recorded from one training step of that workload: every MoCoPCI.bn_batch call of a norm1 / norm2
layer, its layer and the shape of its input).  Per shape, the median of --reps (25) single forward + backward calls with min and max,
alternating in one process (device events after warm-up):
  a  torch            today's formulation (MoCoPCI.bn_batch without lengths: mean + var + the elementwise launches, autograd's backward)
  b  kernel_null      ops.HipBackend.bn_batch with len = NULL
  c  kernel_full      ... with every length N
  d  kernel_half      ... with every length N / 2
The running-estimate update is the same small torch code on every route and is left out of all four.  Recorded with the numbers:
kernel_over_torch = b / a, full_over_null = c / b, and full_within_allowance = c is at most the larger of 1.10 x b and b's min-max
spread above b -- the standing allowance for a full-length call.

    python tools/bn_batch_times.py --out profiles/bn_batch_times.json"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fp_mlp_times import DEV, alternate  # noqa: E402
from mocopci_amd import ops, synth, training  # noqa: E402
from mocopci_amd.model import MoCoPCI  # noqa: E402

EPS = 1e-5


def step_shapes():
    """[(layer, shape)] of the bn_batch calls of the attention blocks' norm layers in one net.train() training step at B = 8, N = 8192."""
    net = MoCoPCI()
    net.load_state_dict(synth.weights_by_name(net._spec), strict=True)
    net = net.to(DEV)
    net.train(True)
    opt = torch.optim.Adam(net.parameters(), lr=1e-5)
    x1, x2, gt = synth.make_batch(2, 8, 8192, device=torch.device(DEV))
    gtc = [g.transpose(1, 2).contiguous() for g in gt]
    seen, plain = [], net.bn_batch

    def recording(x, name, eps, **kw):
        if ".norm" in name:
            seen.append((name, tuple(x.shape)))
        return plain(x, name, eps, **kw)
    net.bn_batch = recording
    training.train_step(net, opt, x1, x2, gtc)
    torch.cuda.synchronize()
    return seen


def torch_formulation(x, weight, bias, eps):
    """MoCoPCI.bn_batch's dense code without the running-estimate update."""
    G, C = x.shape[0], x.shape[-1]
    flat = x.reshape(G, -1, C)
    mean = flat.mean(dim=1)
    var = flat.var(dim=1, unbiased=False)
    shape = (G,) + (1,) * (x.dim() - 2) + (C,)
    scale = weight * torch.rsqrt(var + eps)
    return (x - mean.reshape(shape)) * scale.reshape(shape) + bias


def measure(layers, shape, reps):
    G, N, C = shape[0], shape[-2], shape[-1]
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(*shape, generator=g) * 0.7 + 0.3).to(DEV).requires_grad_(True)
    weight = (1.0 + 0.2 * torch.randn(C, generator=g)).to(DEV).requires_grad_(True)
    bias = (0.1 * torch.randn(C, generator=g)).to(DEV).requires_grad_(True)
    up = torch.randn(*shape, generator=g).to(DEV)
    be = ops.backend()
    full = torch.full((G,), N, dtype=torch.int32, device=DEV)
    half = torch.full((G,), N // 2, dtype=torch.int32, device=DEV)
    leaves = [x, weight, bias]
    res = {}

    def kernel(lengths, key):
        def run():
            res[key] = torch.autograd.grad(be.bn_batch(x, weight, bias, EPS, lengths=lengths)[0], leaves, up)
        return run

    def composition():
        res["a"] = torch.autograd.grad(torch_formulation(x, weight, bias, EPS), leaves, up)
    row = alternate({"torch": composition, "kernel_null": kernel(None, "b"), "kernel_full": kernel(full, "c"), "kernel_half": kernel(half, "d")}, reps)
    a, b, c = row["torch"], row["kernel_null"], row["kernel_full"]
    spread = b["max_ms"] - b["min_ms"]
    apart = max(float((p - q).abs().max() / q.abs().max().clamp_min(1e-30)) for p, q in zip(res["b"], res["a"]))
    return {"layers": layers, "shape": list(shape), "parts": be_parts(shape), "reps": reps, **row,
            "kernel_over_torch": round(b["median_ms"] / a["median_ms"], 4), "full_over_null": round(c["median_ms"] / b["median_ms"], 4),
            "null_spread_ms": round(spread, 4), "full_within_allowance": c["median_ms"] <= max(1.10 * b["median_ms"], b["median_ms"] + spread),
            "full_bits_equal_null": all(torch.equal(p, q) for p, q in zip(res["b"], res["c"])),
            "max_relative_difference_kernel_torch": apart}


def be_parts(shape):
    from mocopci_amd import _lib
    x4 = (shape[0], 1, *shape[1:]) if len(shape) == 3 else shape
    return _lib.load().mcp_bn_batch_parts(*x4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    calls = step_shapes()
    by_shape = {}
    for name, shape in calls:
        by_shape.setdefault(shape, []).append(name)
    print("bn_batch calls of one training step:", json.dumps([[n, list(s)] for n, s in calls]), flush=True)
    rows = []
    for shape, layers in by_shape.items():
        rows.append(measure(sorted(set(layers)), shape, args.reps))
        print(json.dumps(rows[-1]), flush=True)
    doc = {"device": torch.cuda.get_device_name(0), "workload": "bench.py --train-step train (B = 8, N = 8192)",
           "calls_per_step": [[n, list(s)] for n, s in calls], "shapes": rows}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
