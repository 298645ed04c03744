"""Backward times of the D = 256 cost volume and of the interpolation weights: the hand-written kernels against autograd over the
unfused twins (mocopci_amd/grad.py), in one process, alternating, warm, device events around work that ends in a synchronise.

    cross, D = 256, 16 + 16 halves: the training shape (both directions stacked: B = 16, n1 = n2 = 256) and B = 3, n1 = 1237, n2 = 1500;
        (a) backward through grad.run(fused, cross_twin), (b) backward through HipBackend.cross_layer (mcp_cross256_grad + the two
        segmented scatters).  Gradients w.r.t. all eight inputs in both.
    interpolation weights of one (8192, 2048) pair at B = 8: (a) grad.run(weights, interp3_weights_twin), (b) HipBackend.interp3_search.
Each repeat builds the forward graph untimed and times only the backward.  Prints one JSON line per shape with both medians, the
spread (min, max) of each, the ratio, the repeat count and the device name; `--out FILE` appends them there too."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mocopci_amd import grad, ops  # noqa: E402


def rnd(seed, *shape, scale=1.0):
    return (torch.randn(tuple(shape), generator=torch.Generator().manual_seed(seed)) * scale).cuda()


def backward_ms(forward, leaves, g):
    """One backward of forward(*leaves) under device events; the forward is built untimed."""
    out = forward(*leaves)
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(True), torch.cuda.Event(True)
    s.record()
    with ops.segments_memo():
        torch.autograd.grad(out, leaves, g)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def alternate(fa, fb, leaves, g, reps):
    for f in (fa, fb, fa, fb):   # warm: code objects, allocator, library algorithm choices
        backward_ms(f, leaves, g)
    ta, tb = [], []
    for _ in range(reps):
        ta.append(backward_ms(fa, leaves, g))
        tb.append(backward_ms(fb, leaves, g))
    med = lambda v: sorted(v)[len(v) // 2]
    r3 = lambda v: round(v, 3)
    return {"twin_ms": r3(med(ta)), "twin_min_max_ms": [r3(min(ta)), r3(max(ta))], "hip_ms": r3(med(tb)), "hip_min_max_ms": [r3(min(tb)), r3(max(tb))],
            "twin_over_hip": round(med(ta) / med(tb), 3), "reps": reps}


def cross(b, n1, n2, reps):
    be, d = ops.backend(), 256
    xyz1, xyz2 = rnd(1, b, n1, 3, scale=5.0), rnd(2, b, n2, 3, scale=5.0)
    halves = (be.knn(xyz1, xyz2, 16), be.knn(xyz1, xyz2, 32)[..., 16:].contiguous())
    leaves = [t.requires_grad_(True) for t in (xyz1, xyz2, rnd(3, b, n1, d), rnd(4, b, n2, d), rnd(5, d, 3, scale=0.3), rnd(6, d, scale=0.1),
                                               rnd(7, d, d, scale=d ** -0.5), rnd(8, d, scale=0.1))]

    def fused(x1, x2, f1, f2, i, wp, bp, wm, bm):
        return be.cross_volume(x1.contiguous(), x2.contiguous(), f1.contiguous(), f2.contiguous(), i, be.cross_pack(wp, bp, wm, bm))
    twin = lambda *a: grad.run(fused, lambda *t: grad.cross_twin(be.group_rows, *t), *a[:4], halves, *a[4:])
    hip = lambda *a: be.cross_layer(*a[:4], halves, *a[4:])
    r = alternate(twin, hip, leaves, rnd(9, b, n1, d), reps)
    return {"layer": "cross256", "B": b, "n1": n1, "n2": n2, **r}


def weights(b, n, s, reps):
    be = ops.backend()
    leaves = [rnd(11, b, n, 3, scale=5.0).requires_grad_(True), rnd(12, b, s, 3, scale=5.0).requires_grad_(True)]
    idx3 = be.interp3_search(leaves[0].detach(), leaves[1].detach())[0]
    twin = lambda d, s_: grad.run(be._interp3_weights, lambda a, c, i: grad.interp3_weights_twin(be.group_rows, a, c, i), d, s_, idx3)
    hip = lambda d, s_: be.interp3_search(d, s_)[1]
    r = alternate(twin, hip, leaves, rnd(13, b, n, 3), reps)
    return {"layer": "interp3_weights", "B": b, "n": n, "s": s, **r}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    lines = []
    for r in (cross(16, 256, 256, a.reps), cross(3, 1237, 1500, a.reps), weights(8, 8192, 2048, a.reps)):
        r["device"] = torch.cuda.get_device_name(0)
        lines.append(json.dumps(r))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
