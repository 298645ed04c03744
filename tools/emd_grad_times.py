"""EMD forward / backward device times at B = 8, N = M = 8192 (device events after warm-up; the two forwards alternate).

    mcp_emd (no gradient) vs mcp_emd_keep (keeps the levels); mcp_emd_grad (lean backward, both sides);
    mcp_matchcost_grad (explicit-match backward) at B = 1.
Two point sets: a LiDAR-like box (80 x 80 x 6 m, the pair 0.3 m apart) and the unit-free cube [0, 4]^3 of the tests.
Prints one JSON line per set; `--out FILE` appends them there too."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mocopci_amd import _lib, emd  # noqa: E402


def timed(fn, reps):
    s, e = torch.cuda.Event(True), torch.cuda.Event(True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def measure(name, x, y, reps):
    lib = _lib.load()
    B, N, _ = x.shape
    M = y.shape[1]
    cost = torch.empty(B, device=x.device)
    ws = torch.empty(B * (3 * N + 2 * M), device=x.device)
    levels = torch.empty(lib.mcp_emd_levels_floats(B, N, M), device=x.device)
    g = torch.linspace(0.5, 2.0, B, device=x.device)
    g1, g2 = torch.empty_like(x), torch.empty_like(y)
    p = _lib.fptr
    plain = lambda: _lib.check(lib.mcp_emd(B, N, M, p(x), p(y), None, p(cost), p(ws), _lib.stream()))
    keep = lambda: _lib.check(lib.mcp_emd_keep(B, N, M, p(x), p(y), p(cost), p(levels), p(ws), _lib.stream()))
    grad = lambda: _lib.check(lib.mcp_emd_grad(B, N, M, p(g), p(x), p(y), p(levels), p(g1), p(g2), _lib.stream()))
    grad1 = lambda: _lib.check(lib.mcp_emd_grad(B, N, M, p(g), p(x), p(y), p(levels), p(g1), None, _lib.stream()))
    for f in (plain, keep, grad):
        f()
    torch.cuda.synchronize()
    t_plain, t_keep = [], []
    for _ in range(reps):
        t_plain.append(timed(plain, 1))
        t_keep.append(timed(keep, 1))
    keep()
    t_grad = timed(grad, reps)
    t_grad1 = timed(grad1, reps)
    # explicit match at B = 1 (256 MiB match)
    x1, y1 = x[:1].contiguous(), y[:1].contiguous()
    match = emd.approxmatch_forward(x1, y1)
    h1, h2 = torch.empty_like(x1), torch.empty_like(y1)
    mgrad = lambda: _lib.check(lib.mcp_matchcost_grad(1, N, M, p(g[:1].contiguous()), p(x1), p(y1), p(match), p(h1), p(h2), _lib.stream()))
    c1 = torch.empty(1, device=x.device)
    mcost = lambda: _lib.check(lib.mcp_matchcost(1, N, M, p(x1), p(y1), p(match), p(c1), _lib.stream()))
    mgrad(); mcost()
    t_mgrad = timed(mgrad, max(2, reps // 2))
    t_mcost = timed(mcost, max(2, reps // 2))
    med = lambda v: sorted(v)[len(v) // 2]
    return {"set": name, "B": B, "N": N, "M": M, "reps": reps,
            "mcp_emd_ms": round(med(t_plain), 3), "mcp_emd_keep_ms": round(med(t_keep), 3),
            "keep_over_plain": round(med(t_keep) / med(t_plain), 4),
            "mcp_emd_grad_ms": round(t_grad, 3), "mcp_emd_grad_side1_ms": round(t_grad1, 3),
            "mcp_matchcost_grad_b1_ms": round(t_mgrad, 3), "mcp_matchcost_b1_ms": round(t_mcost, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    gen = torch.Generator().manual_seed(7)
    B, N = 8, 8192
    lidar = torch.rand(B, N, 3, generator=gen) * torch.tensor([80.0, 80.0, 6.0])
    cube = torch.rand(B, N, 3, generator=gen) * 4
    lines = []
    for name, x in (("lidar", lidar), ("cube4", cube)):
        y = x[:, torch.randperm(N, generator=gen)] + 0.3 * torch.randn(B, N, 3, generator=gen)
        r = measure(name, x.cuda().contiguous(), y.cuda().contiguous(), a.reps)
        r["device"] = torch.cuda.get_device_name(0)
        lines.append(json.dumps(r))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
