"""Device times of ball query under per-cloud lengths and of the box-pruned ball query (device events after warm-up; medians of
--reps (25) single launches with min and max, the rows of one setting alternating per repetition in one process).

Shapes, on the LiDAR-like box of mocopci_amd.synth (the bench's clouds), centres = the cloud's first M rows, at the four legacy
radius / nsample pairs 0.5/16, 1/16, 2/8, 4/8:
  c4      B = 8, N = 16384, M = 2048, every row live (bench.py --config c4's standalone ball_query launches)
  ragged  B = 8, N = 40960, M = 2048, cloud lengths 33000 .. 35000 (whole scans of different sizes in one padded batch)
Rows per setting:
  a  plain              mcp_ball_query on the padded cloud (the length-free launch; pre-zeroed idx not included); timed twice per
                        rotation, as its first row and, as plain_again, as its last: what a row's place in the rotation is worth
  b  lengths_full       mcp_ball_query_lengths, every length full
  c  lengths_half       mcp_ball_query_lengths, every length halved
  x  lengths_shape      mcp_ball_query_lengths under the shape's lengths (c4: the same call as b)
  d  pruned_search      mcp_ball_query_pruned alone, on a cloud sorted beforehand under the shape's lengths
  e  pruned_with_build  HipBackend.ball_query on the pruned route outside a cloud_scope: cloud build + search
and per shape
  f  four_radii_scope   the four settings inside one cloud_scope on the pruned route (one build), against 4 launches of (a) and of (x)
Recorded with the numbers:
  * b_within_bound: b's median <= max(1.10 x a's median, a's median + a's (max - min)), and b's idx equals a's bit for bit;
  * e_wins: e's median is below x's by more than x's own max - min -- the condition for routing the shape class to the pruned search;
  * d and e return x's idx and cnt bit for bit.
Prints one JSON document; `--out FILE` writes it there."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mocopci_amd import _lib, ops, synth  # noqa: E402

SETTINGS = ((0.5, 16), (1.0, 16), (2.0, 8), (4.0, 8))
SHAPES = (("c4", 8, 16384, 2048, None), ("ragged", 8, 40960, 2048, (34000, 33000, 35000, 34500, 33500, 34000, 34900, 33100)))
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


def measure_shape(name, B, N, M, rlens, reps):
    be = ops.HipBackend()
    cls = ops.HipBackend
    cls.BALL_PRUNE_MIN_REFS, cls.BALL_PRUNE_MIN_CENTRES = 1, 1   # row e and f measure the pruned route whatever the product's rule says
    xyz = synth.make_batch(1, B, N)[0].permute(0, 2, 1).contiguous().to(DEV)
    centres = xyz[:, :M].contiguous()
    f, i = _lib.fptr, _lib.iptr
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
    full_r, full_q = i32([N] * B), i32([M] * B)
    half_r, half_q = i32([N // 2] * B), i32([M // 2] * B)
    shape_r = full_r if rlens is None else i32(list(rlens))
    sorted_cloud = be._build_cloud(xyz, shape_r)
    doc = {"shape": name, "B": B, "N": N, "M": M, "cloud_lengths": "full" if rlens is None else list(rlens), "reps": reps, "settings": []}
    for r, ns in SETTINGS:
        out = {k: (torch.empty((B, M, ns), dtype=torch.int32, device=DEV), torch.empty((B, M), dtype=torch.int32, device=DEV)) for k in "bcxd"}
        plain = torch.zeros((B, M, ns), dtype=torch.int32, device=DEV)
        res = {}

        def exhaustive(tag, ql, rl):
            o = out[tag]
            return lambda: ops._call("mcp_ball_query_lengths", xyz, B, N, M, r, ns, f(centres), f(xyz), i(ql), i(rl), i(o[0]), i(o[1]))

        def with_build():
            res["e"] = be.ball_query(xyz, centres, r, ns, xyz_lengths=shape_r, new_xyz_lengths=full_q, return_count=True)

        rs, rperm, boxes = sorted_cloud
        runs = {"plain": lambda: ops._call("mcp_ball_query", xyz, B, N, M, r, ns, f(centres), f(xyz), i(plain)),
                "lengths_full": exhaustive("b", full_q, full_r), "lengths_half": exhaustive("c", half_q, half_r),
                "lengths_shape": exhaustive("x", full_q, shape_r),
                "pruned_search": lambda: ops._call("mcp_ball_query_pruned", xyz, B, N, M, r, ns, f(centres), f(rs), i(rperm), f(boxes), i(full_q),
                                                   i(shape_r), i(out["d"][0]), i(out["d"][1])),
                "pruned_with_build": with_build}
        runs["plain_again"] = runs["plain"]
        row = {"radius": r, "nsample": ns, **alternate(runs, reps)}
        a, b, x, e = row["plain"], row["lengths_full"], row["lengths_shape"], row["pruned_with_build"]
        row["b_over_a"] = round(b["median_ms"] / a["median_ms"], 4)
        row["b_within_bound"] = b["median_ms"] <= max(1.10 * a["median_ms"], a["median_ms"] + a["max_ms"] - a["min_ms"])
        row["b_bits_equal_a"] = bool(torch.equal(out["b"][0], plain))
        row["e_over_x"] = round(e["median_ms"] / x["median_ms"], 4)
        row["d_over_x"] = round(row["pruned_search"]["median_ms"] / x["median_ms"], 4)
        row["e_wins"] = e["median_ms"] < x["median_ms"] - (x["max_ms"] - x["min_ms"])
        same = lambda p, q: bool(torch.equal(p[0], q[0]) and torch.equal(p[1], q[1]))
        row["d_e_bits_equal_x"] = same(out["d"], out["x"]) and same(res["e"], out["x"])
        doc["settings"].append(row)

    def scope():
        with be.cloud_scope():
            for r, ns in SETTINGS:
                be.ball_query(xyz, centres, r, ns, xyz_lengths=shape_r, new_xyz_lengths=full_q)

    four = alternate({"four_radii_scope": scope}, reps)["four_radii_scope"]
    plain4 = round(sum(s["plain"]["median_ms"] for s in doc["settings"]), 4)
    scans4 = round(sum(s["lengths_shape"]["median_ms"] for s in doc["settings"]), 4)
    doc["four_radii_scope"] = {**four, "four_plain_launches_ms": plain4, "scope_over_plain": round(four["median_ms"] / plain4, 4),
                               "four_lengths_shape_launches_ms": scans4, "scope_over_lengths_shape": round(four["median_ms"] / scans4, 4)}
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    doc = {"device": torch.cuda.get_device_name(0), "shapes": [measure_shape(*s, a.reps) for s in SHAPES]}
    text = json.dumps(doc, indent=1)
    print(text, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
