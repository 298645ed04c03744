"""Device times of the length-aware exhaustive KNN search against the plain one (device events after warm-up).

In one process, alternating per repetition:  mcp_knn  |  mcp_knn_lengths with every length full  |  mcp_knn_lengths with every
reference length at n / 2 (query lengths full).  Shapes (B, Q, N, K, distance form): (8, 8192, 8192, 1, direct),
(8, 8192, 8192, 32, expansion), (1, 8192, 131072, 1, direct).  Medians of --reps (25) single launches with min and max.
Two expectations are evaluated and recorded with the numbers:
  * full lengths do the same arithmetic plus one bound per tile: the median should sit within max(10 %, mcp_knn's own
    (max - min) / median) of mcp_knn's median;
  * half lengths skip half of the tiles: the median should be clearly below the full-length one (recorded as the ratio).
The full-length results are also compared with mcp_knn's bit for bit.  Prints one JSON document; `--out FILE` writes it there."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mocopci_amd import _lib  # noqa: E402

SHAPES = [(8, 8192, 8192, 1, 1), (8, 8192, 8192, 32, 0), (1, 8192, 131072, 1, 1)]


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


def measure(B, Q, N, K, mode, reps, gen):
    lib, dev = _lib.load(), "cuda:0"
    extent = torch.tensor([40.0, 40.0, 3.0])
    query = ((torch.rand(B, Q, 3, generator=gen) * 2 - 1) * extent).to(dev)
    ref = ((torch.rand(B, N, 3, generator=gen) * 2 - 1) * extent).to(dev)
    full_q = torch.full((B,), Q, dtype=torch.int32, device=dev)
    full_r = torch.full((B,), N, dtype=torch.int32, device=dev)
    half_r = torch.full((B,), N // 2, dtype=torch.int32, device=dev)
    out = {name: (torch.empty((B, Q, K), dtype=torch.int32, device=dev), torch.empty((B, Q, K), dtype=torch.float32, device=dev))
           for name in ("mcp_knn", "lengths_full", "lengths_half")}
    f, i = _lib.fptr, _lib.iptr

    def plain():
        idx, dist = out["mcp_knn"]
        _lib.check(lib.mcp_knn(B, Q, N, K, mode, f(query), f(ref), i(idx), f(dist), _lib.stream()))

    def lengths(name, rl):
        def run():
            idx, dist = out[name]
            _lib.check(lib.mcp_knn_lengths(B, Q, N, K, mode, f(query), f(ref), i(full_q), i(rl), i(idx), f(dist), _lib.stream()))
        return run

    runs = {"mcp_knn": plain, "lengths_full": lengths("lengths_full", full_r), "lengths_half": lengths("lengths_half", half_r)}
    for _ in range(3):
        for fn in runs.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in runs}
    for _ in range(reps):
        for name, fn in runs.items():
            times[name].append(timed(fn))
    r = {"B": B, "Q": Q, "N": N, "K": K, "dist_form": "direct" if mode else "expansion", "reps": reps}
    r.update({name: stats(v) for name, v in times.items()})
    base = r["mcp_knn"]
    spread = (base["max_ms"] - base["min_ms"]) / base["median_ms"]
    r["full_over_mcp_knn"] = round(r["lengths_full"]["median_ms"] / base["median_ms"], 4)
    r["allowed_full_over_mcp_knn"] = round(1 + max(0.10, spread), 4)
    r["full_within_expectation"] = r["full_over_mcp_knn"] <= r["allowed_full_over_mcp_knn"]
    r["half_over_full"] = round(r["lengths_half"]["median_ms"] / r["lengths_full"]["median_ms"], 4)
    r["full_lengths_bits_equal_mcp_knn"] = bool(torch.equal(out["mcp_knn"][0], out["lengths_full"][0])
                                                and torch.equal(out["mcp_knn"][1], out["lengths_full"][1]))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    gen = torch.Generator().manual_seed(7)
    doc = {"device": torch.cuda.get_device_name(0), "shapes": [measure(*s, a.reps, gen) for s in SHAPES]}
    text = json.dumps(doc, indent=1)
    print(text, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
