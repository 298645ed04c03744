#!/usr/bin/env python3
"""What centre lengths cost PointConv, at the shapes the flagship forward (B = 8, N = 8192) gives its level-0 layers: alternate, in
one process, the call without lengths, with full lengths and with every length N / 2, and time each with device events.

    python tools/pointconv_lengths_times.py [--rounds 15] [--calls 10] > profiles/pointconv_lengths_times.json

Shapes: the encoder's level 0 (2B = 16 stacked clouds, D = 32, the fused Linear), the speculative all-candidates form of level 1 (16
clouds, D = 64, fused), the refinement stage's speculative PointConvD (3B = 24 clouds, D = 64, fused), and the training route of level
0 (pointconv_agg at D = 32 and its backward).  Neighbour lists come from the level-0 self search of random clouds.  A figure is the
time of `calls` back-to-back calls divided by `calls`; per variant the minimum, median and maximum over the rounds are kept, the
variants taking turns inside every round.  `full_over_none` compares medians; `allowance` is the larger of 2 % and the None call's
own spread, taken between its quartiles ((q3 - q1) / q1): the maximum is one slow first round in most shapes and says nothing about
the call.  Last, the scatter of the backward's per-neighbour rows under half lengths with the padded centres' list rows on row 0
against spread over the rows (grad.spread_padded_rows): why the autograd function spreads them."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mocopci_amd import grad, ops  # noqa: E402

DEV = "cuda:0"


def timed(fn, calls):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / calls   # microseconds per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--batch", type=int, default=8)
    a = ap.parse_args()
    be = ops.backend()
    g = torch.Generator().manual_seed(0)
    r = lambda *shape, scale=1.0: ((torch.rand(*shape, generator=g) * 2 - 1) * scale).to(DEV)
    wn = [r(8, 3, scale=0.8), r(8, scale=0.3), r(8, 8, scale=0.6), r(8, scale=0.3), r(8, 8, scale=0.6), r(8, scale=0.3)]
    N = a.n
    report = {"n": N, "batch": a.batch, "rounds": a.rounds, "calls_per_figure": a.calls, "device": torch.cuda.get_device_name(0), "shapes": {}}

    def shape(name, clouds, d, fused, backward=False):
        xyz, feat = r(clouds, N, 3), r(clouds, N, d)
        idx = be.knn(xyz, xyz, 32)
        lens = {"none": None, "full": torch.full((clouds,), N, dtype=torch.int32, device=DEV),
                "half": torch.full((clouds,), N // 2, dtype=torch.int32, device=DEV)}
        if fused:
            w, b = r(d, (d + 3) * 8, scale=0.05), r(d, scale=0.5)
            packed = be.pointconv_linear_pack(w, b)
            call = lambda l: be.pointconv_linear(xyz, xyz, feat, idx, *wn, w, b, 0.1, packed=packed, **({} if l is None else dict(centre_lengths=l)))
        elif not backward:
            call = lambda l: be.pointconv_agg(xyz, xyz, feat, idx, *wn, **({} if l is None else dict(centre_lengths=l)))
        else:
            leaves = [t.clone().requires_grad_(True) for t in (xyz, xyz, feat, *wn)]
            gout = r(clouds, N, (d + 3) * 8)

            def call(l):
                out = be.pointconv_agg(leaves[0], leaves[1], leaves[2], idx, *leaves[3:], **({} if l is None else dict(centre_lengths=l)))
                return torch.autograd.grad(out, leaves, gout)
        same = call(lens["full"])
        ref = call(None)
        equal = all(torch.equal(x, y) for x, y in zip(same, ref)) if isinstance(ref, tuple) else torch.equal(same, ref)
        for l in lens.values():   # warm every variant
            for _ in range(3):
                call(l)
        torch.cuda.synchronize()
        times = {k: [] for k in lens}
        for _ in range(a.rounds):
            for k, l in lens.items():
                times[k].append(timed(lambda: call(l), a.calls))
        def figures(v):
            q1, _, q3 = statistics.quantiles(v, n=4)
            return {"min_us": round(min(v), 2), "q1_us": round(q1, 2), "median_us": round(statistics.median(v), 2), "q3_us": round(q3, 2),
                    "max_us": round(max(v), 2)}
        row = {k: figures(v) for k, v in times.items()}
        none = row["none"]
        row["full_lengths_equal_none_bits"] = bool(equal)
        row["full_over_none"] = round(row["full"]["median_us"] / none["median_us"], 4)
        row["half_over_none"] = round(row["half"]["median_us"] / none["median_us"], 4)
        row["allowance"] = round(max(0.02, (none["q3_us"] - none["q1_us"]) / none["q1_us"]), 4)
        row["full_within_allowance"] = row["full_over_none"] - 1 <= row["allowance"]
        report["shapes"][name] = dict(clouds=clouds, d=d, **row)

    shape("encoder level 0 (fused Linear, D = 32)", 2 * a.batch, 32, True)
    shape("encoder level 1, all candidates (fused Linear, D = 64)", 2 * a.batch, 64, True)
    shape("refinement PointConvD, all candidates (fused Linear, D = 64)", 3 * a.batch, 64, True)
    shape("level 0 aggregate alone (D = 32)", 2 * a.batch, 32, False)
    shape("level 0 aggregate + backward (D = 32)", 2 * a.batch, 32, False, backward=True)

    def scatter(clouds, d):
        """the segmented scatter of grad_rows (clouds, N, 32, d) under half lengths: padded list rows on row 0 / spread"""
        xyz = r(clouds, N, 3)
        idx = be.knn(xyz, xyz, 32)
        live = grad.live_points(torch.full((clouds,), N // 2, dtype=torch.int32, device=DEV), clouds, N, DEV)
        rows = torch.where(live.view(clouds, N, 1, 1), r(clouds, N, 32, d), torch.zeros((), device=DEV))
        lists = {"padded_rows_on_row_0": torch.where(live.unsqueeze(-1), idx, torch.zeros((), dtype=idx.dtype, device=DEV)),
                 "padded_rows_spread": grad.spread_padded_rows(idx, live, N)}
        run = lambda l: ops._group_rows_grad(rows, l, N, ops._scatter_segments(l, N))
        same = torch.equal(*(run(l) for l in lists.values()))
        out = {"clouds": clouds, "d": d, "equal_bits": bool(same)}
        for k, l in lists.items():
            run(l)
            torch.cuda.synchronize()
            out[k + "_us"] = figures_of([timed(lambda: run(l), 2) for _ in range(5)])
        out["row_0_over_spread"] = round(out["padded_rows_on_row_0_us"]["median_us"] / out["padded_rows_spread_us"]["median_us"], 1)
        return out

    def figures_of(v):
        return {"min_us": round(min(v), 2), "median_us": round(statistics.median(v), 2), "max_us": round(max(v), 2)}
    report["scatter of the backward's rows, every length N / 2"] = scatter(2 * a.batch, 32)
    print(json.dumps(report, indent=1))


if __name__ == "__main__":
    main()
